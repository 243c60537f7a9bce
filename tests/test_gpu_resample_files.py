"""rg_same_recording_xrate on files (include/mp3rgain_amd_resample.h): one continuous-time piece (tests/resample_cases.py) rendered
at 44100 Hz as WAV, at 48000 Hz as FLAC and at 96000 Hz as WAV, the 44100 Hz rendering again as an MPEG Layer III stream of the
project's own encoder, and an unrelated piece at 32000 Hz.  The oracle of the codes is the kernels' arithmetic on the host
(rg_xrate_fingerprint_arena route 2, which tests/test_resample_cpu.py holds to the float64 reference) on the PCM the files were
written from; of the pairs, the serial host match on those codes.  Both FLAC decoder routes give the same bytes."""
import ctypes as C
import sys
from collections import namedtuple
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "oracle"))
import arena_layouts as al  # noqa: E402
import flacenc  # noqa: E402
import resample_cases as rc  # noqa: E402
from wavutil import wav_bytes  # noqa: E402

from mp3rgain_amd import _capi  # noqa: E402
from mp3rgain_amd import replaygain as rgmod  # noqa: E402

pytestmark = pytest.mark.gpu

RG_ERR_IO = -8
REC = C.sizeof(_capi.XrateRecord)
Tr = namedtuple("Tr", "name channels sample_rate")
SECONDS = 5.0


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
    """[(path, Tr of the planes the file was written from, or None for the MP3)]: files 0 .. 3 are one recording, 4 another."""
    import mp3_encoder as E

    tmp = tmp_path_factory.mktemp("xrate")
    a, b, c = (rc.piece(r, SECONDS, seed=1) for r in (44100, 48000, 96000))
    other = rc.piece(32000, SECONDS, seed=2)
    flac = lambda planes, rate: flacenc.encode(np.stack(planes).astype(np.int64), rate, 16, flacenc.Options(block_size=4096))  # noqa: E731
    mp3 = E.encode((a.astype(np.float64) / 32768.0)[None, :], 44100, 128, seed=3, allow_ms=False, allow_short=True)
    return [(_write(tmp, "cd.wav", wav_bytes([a, a], 44100, "s16")), Tr("cd", [a, a], 44100)),
            (_write(tmp, "dl48.flac", flac([b], 48000)), Tr("dl48", [b], 48000)),
            (_write(tmp, "dl96.wav", wav_bytes([c], 96000, "s16")), Tr("dl96", [c], 96000)),
            (_write(tmp, "cd.mp3", mp3), None),
            (_write(tmp, "other.flac", flac([other], 32000)), Tr("other", [other], 32000))]


def _twin(trs):
    arena, descs, _ = al.pack(trs, al.Layout("abut", "loud", "input"))
    recs, codes, _, _ = rgmod.xrate_fingerprint_arena(None, 2, list(descs)[:len(trs)], arena, bands=False)
    return recs, [codes[r.codes_at:r.codes_at + r.codes] for r in recs]


def _records(raw, n):
    assert len(raw) == REC * n
    return [_capi.XrateRecord.from_buffer_copy(raw[REC * k:REC * k + REC]) for k in range(n)]


def test_one_group_across_rates_on_both_decoder_routes_and_in_groups(an, library):
    files = [p for p, _ in library]
    pcm = [k for k, (_, tr) in enumerate(library) if tr is not None]
    wrecs, wcodes = _twin([library[k][1] for k in pcm])
    raw, recs, praw, codes = an.same_recording_any_rate_raw(files, codes_cap=1 << 12)
    assert [(r.status, r.flags, r.dropped_frames) for r in recs] == [(0, _capi.FP_COMPLETE, 0)] * 5
    assert [(r.sample_rate, r.up, r.down) for r in recs] == [(44100, 1, 4), (48000, 147, 640), (96000, 147, 1280), (44100, 1, 4), (32000, 441, 1280)]
    for k, w, c in zip(pcm, wrecs, wcodes):
        r = recs[k]
        assert (r.frames, r.channels, r.fp_frames, r.codes, r.resampled, r.nonfinite_frames) == (w.frames, w.channels, w.fp_frames, w.codes, w.resampled, 0)
        assert r.codes >= _capi.XR_BLOCK and codes[r.codes_at:r.codes_at + r.codes].tobytes() == c.tobytes(), files[k].name  # the seam's codes
    assert [(r.group, r.matches) for r in recs] == [(0, 3), (0, 3), (0, 3), (0, 3), (4, 0)]
    size = C.sizeof(_capi.FingerprintPair)
    pairs = [_capi.FingerprintPair.from_buffer_copy(praw[k:k + size]) for k in range(0, len(praw), size)]
    assert [(p.i, p.j) for p in pairs] == [(0, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 3)]
    want = rc.match(wcodes)  # the serial host match on the twin's codes: pairs (0,1), (0,2), (0,other), (1,2), ..
    for p, w in zip([p for p in pairs if 3 not in (p.i, p.j)], [want[0], want[1], want[3]]):
        assert (p.errors, p.bits, p.lag, p.flags) == (int(w["errors"]), int(w["bits"]), int(w["lag"]), int(w["flags"])) and p.lag == 0
    assert all(not w["flags"] & _capi.FP_PAIR_MATCH for w in (want[2], want[4], want[5]))
    assert all(abs(p.lag) <= 1 and p.errors * 1000 <= p.bits * _capi.XR_MAX_BER_PERMILLE for p in pairs)  # the stream: 1057 samples of delay, half a code
    an.set_tuning(14, 0)  # the host FLAC decoder: the same bytes
    host_dec = an.same_recording_any_rate_raw(files, codes_cap=1 << 12)
    assert host_dec[0] == raw and host_dec[2] == praw and host_dec[3].tobytes() == codes.tobytes()
    an.set_tuning(14, 1)
    an.set_tuning(13, 1 << 18)  # several groups: the codes stay on the device from group to group
    split = an.same_recording_any_rate_raw(files, codes_cap=1 << 12)
    assert split[2] == praw and [(r.group, r.matches, r.codes, r.flags, r.resampled) for r in split[1]] == [(r.group, r.matches, r.codes, r.flags, r.resampled) for r in recs]
    for k, c in zip(pcm, wcodes):
        r = split[1][k]
        assert split[3][r.codes_at:r.codes_at + r.codes].tobytes() == c.tobytes()


def test_the_python_records_and_a_truncated_file(an, library, tmp_path):
    files = [p for p, _ in library]
    recs, pairs, groups = an.same_recording_any_rate(files)
    assert groups == [[0, 1, 2, 3]] and len(pairs) == 6 and all(r.error is None and r.verdicts == ["ok"] for r in recs)
    assert [r.sample_rate for r in recs] == [44100, 48000, 96000, 44100, 32000]
    # the same-rate finder on the same files: only the two 44100 Hz files can be compared
    assert an.same_recording(files, block=64, radius=128)[2] in ([[0, 3]], [])
    cut = _write(tmp_path, "cut.flac", files[1].read_bytes()[:20])  # cut inside the stream header
    missing = tmp_path / "missing.wav"
    recs, pairs, groups = an.same_recording_any_rate([files[0], cut, files[2], missing, files[4]])
    raw = an.same_recording_any_rate_raw([files[0], cut, files[2], missing, files[4]])[0]
    assert groups == [[0, 2]] and [(p.i, p.j) for p in pairs] == [(0, 2)]
    assert [r.error is None for r in recs] == [True, False, True, False, True] and recs[3].error.code == RG_ERR_IO
    for k in (1, 3):
        assert raw[REC * k + 4:REC * k + REC] == bytes(REC - 4)  # zero apart from `status`
    assert an.same_recording_any_rate(files, max_ber_permille=1)[2] == []
    with pytest.raises(rgmod.ReplayGainError) as e:
        an.same_recording_any_rate(files, radius=2048)
    assert e.value.code == -1
    assert an.same_recording_any_rate([]) == ([], [], [])


def test_a_rate_outside_the_supported_set_is_no_error(an, library, tmp_path):
    files = [p for p, _ in library]
    odd = _write(tmp_path, "odd.wav", wav_bytes([library[0][1].channels[0]], 44056, "s16"))
    recs, pairs, groups = an.same_recording_any_rate([files[0], odd, files[1]])
    assert groups == [[0, 2]] and recs[1].error is None and recs[1].unsupported_rate and recs[1].codes == 0
