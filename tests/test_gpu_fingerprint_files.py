"""rg_same_recording on files (include/mp3rgain_amd_fingerprint.h): one piece of synthetic music as WAV, as FLAC and as a copy
degraded by the coarse MP3-like coding of tests/ancestry_cases.py with 1105 leading samples trimmed, and two unrelated pieces.
The oracle of the fingerprints is the kernels' arithmetic on the host (rg_fingerprint_arena route 2, which
tests/test_fingerprint_cpu.py holds to the float64 reference) on the PCM the files were written from; of the pairs, the serial
host match on those codes.  Both FLAC decoder routes give the same bytes, a group size that splits the list the same pairs."""
import ctypes as C
import sys
from collections import namedtuple
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import ancestry_cases as ac  # noqa: E402
import arena_layouts as al  # noqa: E402
import flacenc  # noqa: E402
from wavutil import wav_bytes  # noqa: E402

from mp3rgain_amd import _capi  # noqa: E402
from mp3rgain_amd import replaygain as rgmod  # noqa: E402

pytestmark = pytest.mark.gpu

RG_ERR_IO = -8
REC = C.sizeof(_capi.FingerprintRecord)
N = 4096 + 280 * 512  # 280 codes: a little more than the default block of 256
Tr = namedtuple("Tr", "name channels sample_rate")


@pytest.fixture()
def an(_ctx):
    _ctx.set_tuning(14, 1)
    _ctx.set_tuning(13, 0)
    _ctx.set_decoder_command(None)
    yield _ctx
    _ctx.set_tuning(14, 1)
    _ctx.set_tuning(13, 0)


def _write(tmp, name, data):
    p = tmp / name
    p.write_bytes(data)
    return p


@pytest.fixture(scope="module")
def library(tmp_path_factory):
    """[(path, Tr of the planes the arena holds)]: files 0, 1, 2 are one recording, 3 and 4 two others."""
    tmp = tmp_path_factory.mktemp("fingerprint")
    x = ac.music(N + 1105, 40)
    one = [ac.to_s16(x[:N])]
    coded = [ac.to_s16(ac.short_cut(x, 0.5)[0][1105:1105 + N] * 10 ** (-6 / 20))]  # 1057 of delay, 1105 trimmed: 48 samples early
    other = [ac.to_s16(ac.music(N, 41)), ac.to_s16(ac.music(N, 42, 1500.0))]
    third = [ac.to_s16(ac.music(N + 700, 43))]
    flac = lambda planes: flacenc.encode(np.stack(planes).astype(np.int64), 44100, 16, flacenc.Options(block_size=4096))  # noqa: E731
    return [(_write(tmp, "one.wav", wav_bytes(one, 44100, "s16")), Tr("one_wav", one, 44100)),
            (_write(tmp, "one.flac", flac(one)), Tr("one_flac", one, 44100)),
            (_write(tmp, "one_coded.flac", flac(coded)), Tr("one_coded", coded, 44100)),
            (_write(tmp, "other.flac", flac(other)), Tr("other", other, 44100)),
            (_write(tmp, "third.wav", wav_bytes(third, 44100, "s16")), Tr("third", third, 44100))]


def _twin(trs):
    arena, descs, _ = al.pack(trs, al.Layout("abut", "loud", "input"))
    recs, codes, _ = rgmod.fingerprint_arena(None, 2, list(descs)[:len(trs)], arena, bands=False)
    each = [codes[r.codes_at:r.codes_at + r.codes] for r in recs]
    return recs, each, rgmod.fingerprint_match_codes(None, 0, each, [r.sample_rate for r in recs])


def _records(raw, n):
    assert len(raw) == REC * n
    return [_capi.FingerprintRecord.from_buffer_copy(raw[REC * k:REC * k + REC]) for k in range(n)]


def _pairs(raw):
    size = C.sizeof(_capi.FingerprintPair)
    return [_capi.FingerprintPair.from_buffer_copy(raw[k:k + size]) for k in range(0, len(raw), size)]


def test_one_group_of_three_on_both_decoder_routes_and_in_groups(an, library):
    files, trs = [p for p, _ in library], [tr for _, tr in library]
    wrecs, wcodes, wpairs = _twin(trs)
    raw, praw, codes = an.same_recording_raw(files, codes_cap=sum(len(c) for c in wcodes))
    recs = _records(raw, len(files))
    for k, (r, w, tr) in enumerate(zip(recs, wrecs, trs)):
        assert (r.status, r.flags, r.frames, r.sample_rate, r.channels, r.fp_frames, r.codes, r.nonfinite_frames, r.dropped_frames) == \
            (0, _capi.FP_COMPLETE, w.frames, 44100, w.channels, w.fp_frames, w.codes, 0, 0), tr.name
        assert r.format == _capi.FMT_S16_PLANAR and r.codes >= 280
        assert codes[r.codes_at:r.codes_at + r.codes].tobytes() == wcodes[k].tobytes(), tr.name  # the kernels' codes are the host arithmetic's
    assert [(r.group, r.matches) for r in recs] == [(0, 2), (0, 2), (0, 2), (3, 0), (4, 0)]
    pairs = _pairs(praw)
    assert [(p.i, p.j) for p in pairs] == [(0, 1), (0, 2), (1, 2)]
    want = {(0, 1): wpairs[0], (0, 2): wpairs[1], (1, 2): wpairs[4]}
    for p in pairs:  # the pair records are the serial host match's on the twin's codes
        w = want[(p.i, p.j)]
        assert (p.errors, p.bits, p.lag, p.flags) == (int(w["errors"]), int(w["bits"]), int(w["lag"]), int(w["flags"])) and p.flags & _capi.FP_PAIR_MATCH
    assert (pairs[0].errors, pairs[0].bits, pairs[0].lag) == (0, 8 * 256 * 32, 0)  # WAV and FLAC of the same PCM
    assert pairs[1].lag == 0 and 0 < pairs[1].errors * 1000 < pairs[1].bits * _capi.FP_MAX_BER_PERMILLE  # 48 samples early: lag 0
    assert all(not w["flags"] & _capi.FP_PAIR_MATCH and w["errors"] * 1000 > w["bits"] * 400 for k, w in enumerate(wpairs) if k not in (0, 1, 4))
    an.set_tuning(14, 0)
    assert an.same_recording_raw(files)[:2] == an.same_recording_raw(files)[:2]
    host_dec = an.same_recording_raw(files, codes_cap=len(codes))
    assert host_dec[0] == raw and host_dec[1] == praw and host_dec[2].tobytes() == codes.tobytes()
    an.set_tuning(13, 1 << 18)  # several groups: the codes stay on the device from group to group
    split = an.same_recording_raw(files, codes_cap=len(codes))
    assert split[1] == praw
    srecs = _records(split[0], len(files))
    assert [(r.group, r.matches, r.codes, r.flags) for r in srecs] == [(r.group, r.matches, r.codes, r.flags) for r in recs]
    for r, w in zip(srecs, wcodes):
        assert split[2][r.codes_at:r.codes_at + r.codes].tobytes() == w.tobytes()
    an.set_tuning(14, 1)
    assert an.same_recording_raw(files)[1] == praw


def test_the_python_records_pairs_and_groups(an, library):
    files = [p for p, _ in library]
    recs, pairs, groups = an.same_recording(files)
    assert groups == [[0, 1, 2]] and [(p.i, p.j, p.lag_of_j) for p in pairs] == [(0, 1, 0), (0, 2, 0), (1, 2, 0)]
    assert all(r.error is None and r.complete and r.verdicts == ["ok"] for r in recs) and pairs[0].ber == 0.0 < pairs[1].ber < 0.316
    # a later copy: the third piece with its first 700 samples cut, after the other -> lag -1 (700 / 512 = 1.4) of j
    x = library[4][1].channels[0]
    late = files[0].parent / "third_cut.wav"
    late.write_bytes(wav_bytes([x[700:]], 44100, "s16"))
    recs, pairs, groups = an.same_recording([files[4], files[3], late])
    assert groups == [[0, 2]] and [(p.i, p.j, p.lag_of_j, p.probe_j) for p in pairs] == [(0, 2, -1, True)]
    recs, pairs, groups = an.same_recording(files, max_ber_permille=1)  # only the bit-identical pair is left
    assert groups == [[0, 1]] and len(pairs) == 1
    recs, pairs, groups = an.same_recording(files[:3], block=281)  # longer than any of the files' codes: nothing is compared
    assert groups == [] and pairs == [] and [r.group for r in recs] == [0, 1, 2]
    for bad in (dict(radius=2048), dict(block=5000), dict(max_ber_permille=1001)):
        with pytest.raises(rgmod.ReplayGainError) as e:
            an.same_recording(files, **bad)
        assert e.value.code == -1
    assert an.same_recording([]) == ([], [], [])
    assert an.same_recording(files[:1])[2] == []


def test_max_pairs_smaller_than_the_matches(an, library):
    files = [p for p, _ in library]
    paths, out = an._file_args(files, _capi.FingerprintRecord)
    pairs = (_capi.FingerprintPair * 2)()
    n_pairs = C.c_size_t(0)
    an._check(an._lib.rg_same_recording(an._ctx, paths, len(files), None, out, pairs, 2, C.byref(n_pairs), None, 0))
    assert n_pairs.value == 3 and [(p.i, p.j) for p in pairs] == [(0, 1), (0, 2)]
    an._check(an._lib.rg_same_recording(an._ctx, paths, len(files), None, out, None, 0, C.byref(n_pairs), None, 0))
    assert n_pairs.value == 3 and all(r.codes_at == 2 ** 64 - 1 for r in out)


def test_failing_files_fail_alone(an, tmp_path, library):
    text = _write(tmp_path, "notes.txt", b"not audio at all\n" * 40)
    missing = tmp_path / "missing.flac"
    files = [library[0][0], missing, library[2][0], text, library[3][0]]
    an.set_decoder_command("false {}")  # a decoder command is set and must not be run
    try:
        recs, pairs, groups = an.same_recording(files)
        raw = an.same_recording_raw(files)[0]
    finally:
        an.set_decoder_command(None)
    assert groups == [[0, 2]] and [(p.i, p.j) for p in pairs] == [(0, 2)]
    assert [r.error is None for r in recs] == [True, False, True, False, True] and [recs[k].group for k in (0, 2, 4)] == [0, 0, 4]
    assert recs[1].error.code == RG_ERR_IO and "Failed to open" in str(recs[1].error) and str(missing) in str(recs[1].error)
    assert str(text) in str(recs[3].error)
    for k in (1, 3):
        assert (recs[k].frames, recs[k].flags, recs[k].codes, recs[k].group, recs[k].matches) == (0, 0, 0, 0, 0)
        assert raw[REC * k + 4:REC * k + REC] == bytes(REC - 4)  # zero apart from `status`
