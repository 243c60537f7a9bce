"""Stage 2 of the tempo scan on the CPU (include/mp3rgain_amd_tempo.h): the serial host twin (rg_tempo_from_onsets route 0)
against the header's definitions restated in numpy and Python integers (tests/tempo_cases.ref_stage2) on constructed onset
curves, field for field and sum for sum; what the constructed cases are there to show; option and argument errors.  No GPU."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import tempo_cases as tc  # noqa: E402

import mp3rgain_amd as rg  # noqa: E402
from mp3rgain_amd import _capi  # noqa: E402

RG_ERR_INVALID_ARG = -1


@pytest.fixture(scope="module")
def results():
    return {ac.name: (ac, rg.tempo_from_onsets(None, 0, list(ac.onsets), ac.rates, **ac.opts)) for ac in tc.acf_cases()}


@pytest.mark.parametrize("ac", tc.acf_cases(), ids=lambda ac: ac.name)
def test_host_twin_equals_the_restatement(results, ac):
    recs, acf = results[ac.name][1]
    assert len(recs) == len(ac.onsets)
    at = 0
    for k, (o, rate) in enumerate(zip(ac.onsets, ac.rates)):
        want, C = tc.ref_stage2(o, rate, **ac.opts)
        r = recs[k]
        assert tc.record_fields(r, ~0) == dict(want, flags=want["flags"] | _capi.TEMPO_COMPLETE), (ac.name, k)
        assert [int(v) for v in acf[k]] == C, (ac.name, k)
        assert (r.status, r.frames, r.channels, r.format, r.dropped_frames, r.nonfinite_frames, r.band_frames, r.onsets_at) == (0, 0, 0, 0, 0, 0, 0, at)
        at += len(o)


def test_what_the_cases_are_there_to_show(results):
    S, R, G, N = _capi.TEMPO_SHORT, _capi.TEMPO_RATE, _capi.TEMPO_RANGE, _capi.TEMPO_NONE
    one = lambda name, k=0: results[name][1][0][k]  # noqa: E731
    acf = lambda name, k=0: results[name][1][1][k]  # noqa: E731
    assert one("short").flags & S and one("short").windows == 0 and not acf("short").any()
    assert [one(n).windows for n in ("one_window", "hop_minus_1", "two_windows")] == [1, 1, 2]
    for name in ("zeros", "constant", "all_1023_w1024"):  # C[0] <= 0: no tempo, and no other flag
        r = one(name)
        assert r.flags & N and not r.flags & (S | R | G) and (r.period16, r.bpm_milli, r.confidence_permille, r.first_beat) == (0, 0, 0, 0)
        assert acf(name)[0] <= 0
    # the headroom: every product 1023^2 over W = 1024 is below 2^32, and c_w stays within an i32 with one onset in 97 at zero
    assert 1024 * 1023 * 1023 < 2 ** 32
    c = acf("nearly_1023_w1024")
    assert one("nearly_1023_w1024").period16 and 0 < c[0] and np.abs(c).max() < 2 * 2 ** 31
    # a period of 21.3 onsets = 340.8 sixteenths -> 341; changed to 27.9 halfway, some windows disagree
    r = one("pulses")
    assert (r.period16, r.stable_permille, r.harmonics) == (341, 1000, 3) and r.bpm_milli == round(1875 * 44100 / 341)
    assert r.confidence_permille > 500 and (r.first_beat - _capi.TEMPO_BEAT_BIAS) % 32 == 0
    assert 0 < one("tempo_change").stable_permille < 1000
    r = one("windows_300")
    assert r.windows == 300 and r.period16 == 395 and acf("windows_300")[0] > 300 * 2 ** 20  # a sum no window's i32 holds at ease
    recs = results["four_rates"][1][0]
    assert [r.harmonics for r in recs] == [3, 3, 1, 8, 3] and [r.period16 for r in recs[:4]] == [341, 368, 800, 155] and recs[4].flags & S
    assert [round(p / 16, 1) for p in (341, 368, 800, 155)] == [21.3, 23.0, 50.0, 9.7]  # 800 = the second pulse of 50.2 / 2 is out of range
    recs = results["range_w32"][1][0]
    assert recs[0].flags & G and recs[0].harmonics == 0 and recs[0].period16 == 0 and not results["range_w32"][1][1][0].any()
    assert not recs[1].flags & G and recs[1].harmonics == 2 and recs[1].period16
    r = one("rate_unsupported")
    assert r.flags & R and r.flags & S and r.onsets == 400 and r.windows == 0
    assert results["n0"][1][0] == []


def test_ties_go_to_the_smaller_period_and_phase():
    """A curve of period exactly 20 onsets: phases 312 .. 327 read the same onsets ((phi + 8) >> 4 = 20): the smallest wins."""
    o = np.zeros(600, np.uint16)
    o[20::20] = 900
    recs, _ = rg.tempo_from_onsets(None, 0, [o], [44100], **tc.SMALL)
    want, _ = tc.ref_stage2(o, 44100, **tc.SMALL)
    assert tc.record_fields(recs[0]) == want
    assert recs[0].period16 == 320 and recs[0].first_beat == 312 * 32 + _capi.TEMPO_BEAT_BIAS


def test_option_and_argument_errors():
    o = [tc.pulse_curve(300, 21.3, 1)]
    for bad in (dict(window=31), dict(window=1025), dict(window=64, hop=65), dict(min_bpm=29), dict(min_bpm=301)):
        with pytest.raises(rg.ReplayGainError) as e:
            rg.tempo_from_onsets(None, 0, o, [44100], **bad)
        assert e.value.code == RG_ERR_INVALID_ARG and "tempo: window" in str(e.value)
    with pytest.raises(rg.ReplayGainError) as e:
        rg.tempo_from_onsets(None, 2, o, [44100])
    assert e.value.code == RG_ERR_INVALID_ARG and "route 2" in str(e.value)
    with pytest.raises(rg.ReplayGainError) as e:
        rg.tempo_from_onsets(None, 0, [np.array([5, 1024, 7], np.uint16)], [44100])
    assert e.value.code == RG_ERR_INVALID_ARG and "onset 1 is 1024" in str(e.value)
    with pytest.raises(rg.ReplayGainError):
        rg.tempo_from_onsets(None, 1, o, [44100])  # the kernels need a context
    # a zero field is its default: hop = min(256, window)
    a = rg.tempo_from_onsets(None, 0, o, [44100], window=128, min_bpm=160)[0][0]
    b = rg.tempo_from_onsets(None, 0, o, [44100], window=128, hop=128, min_bpm=160)[0][0]
    assert bytes(a) == bytes(b) and a.windows == 1
