"""Stage 2 of the key scan on the CPU (include/mp3rgain_amd_key.h): the serial host twin (rg_key_from_chroma route 0) equals the
restatement of the header's definitions in Python integers (tests/key_cases.py: ref_stage2) on constructed rows, field for
field; the bounds the header states; the refusals.  No GPU."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import key_cases as kc  # noqa: E402

import mp3rgain_amd as rg  # noqa: E402
from mp3rgain_amd import _capi  # noqa: E402


@pytest.mark.parametrize("cc", kc.chroma_cases(), ids=lambda cc: cc.name)
def test_the_host_twin_equals_the_restatement(cc):
    recs = rg.key_from_chroma(None, 0, list(cc.rows), segment=cc.segment)
    at = 0
    for r, rows in zip(recs, cc.rows):
        assert kc.record_fields(r) == kc.ref_stage2(rows, cc.segment), cc.name
        assert (r.status, r.frames, r.sample_rate, r.channels, r.decim, r.decimated, r.chroma_at) == (0, 0, 0, 0, 0, 0, at)
        assert bool(r.flags & _capi.KEY_COMPLETE)
        at += len(rows)


def test_what_the_constructed_cases_are_for():
    by = {cc.name: rg.key_from_chroma(None, 0, list(cc.rows), segment=cc.segment) for cc in kc.chroma_cases()}
    C, S, NONE = _capi.KEY_COMPLETE, _capi.KEY_SHORT, _capi.KEY_NONE
    r = by["one_pitch_class"][0]
    assert (r.flags, rg.key_name(r.key), r.stable_permille, r.segments) == (C, "G major", 1000, 5) and r.correlation_permille > 500
    for name in ("flat", "zeros", "all_800_long"):
        r = by[name][0]
        assert (r.flags, r.key, r.tonic, r.mode, r.correlation_permille, r.margin_permille, r.stable_permille) == (C | NONE, 0, 0, 0, 0, 0, 0), name
    assert by["zeros"][0].silent_rows == 40 and by["flat"][0].silent_rows == 0
    r = by["rows_800_shift"][0]
    assert 300 * 800 >= 65536 and (r.flags, rg.key_name(r.key)) == (C, "D minor")
    r = by["key_change"][0]
    assert (rg.key_name(r.key), r.segments, r.stable_permille) == ("C major", 3, 666)
    assert (by["below_one_segment"][0].segments, by["below_one_segment"][0].stable_permille, by["one_segment"][0].segments, by["one_segment"][0].stable_permille) == (0, 0, 1, 1000)
    assert rg.key_name(by["one_segment"][0].key) == "A minor"
    r = by["a_silent_segment"][0]
    assert (r.segments, r.stable_permille, r.silent_rows) == (3, 1000, 32)
    assert [r.key for r in by["every_key"]] == list(range(24))
    assert [r.flags for r in by["more_rows_than_lanes"]] == [C, C | S, C]
    assert by["segments_beyond_the_lanes"][0].segments == 300 and by["n0"] == []


def test_the_bounds_of_the_header():
    """The largest sums: every intermediate of the restatement is below 2^63, and the twin equals it there too."""
    rows = np.zeros((4096 * 4, 12), np.uint16)
    rows[:, 0] = 800
    rows[:, 7] = 799
    r = rg.key_from_chroma(None, 0, [rows], segment=4096)[0]
    assert kc.record_fields(r) == kc.ref_stage2(rows, 4096) and r.segments == 4
    h = [65535] + [0] * 11
    assert 1000000 * (12 * sum(v * v for v in h) - sum(h) ** 2) < 2 ** 60 and 1000 * 65535 * 2862 < 2 ** 38


def test_refusals():
    ok = np.zeros((10, 12), np.uint16)
    for seg in (7, 4097):
        with pytest.raises(rg.ReplayGainError) as e:
            rg.key_from_chroma(None, 0, [ok], segment=seg)
        assert e.value.code == -1 and "key: segment" in str(e.value)
    bad = ok.copy()
    bad[3, 4] = 801
    with pytest.raises(rg.ReplayGainError) as e:
        rg.key_from_chroma(None, 0, [bad])
    assert e.value.code == -1 and "entry 40 is 801" in str(e.value)
    with pytest.raises(rg.ReplayGainError):
        rg.key_from_chroma(None, 2, [ok])
