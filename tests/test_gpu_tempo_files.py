"""rg_tempo on files (include/mp3rgain_amd_tempo.h): a 30 s click track at 120 BPM as WAV, as FLAC and as a stream of this tree's
MP3 encoder, a missing path and a FLAC stream with a dropped frame.  The oracle is the kernels' arithmetic on the host with the
host's stage 2 (rg_tempo_arena route 2, which tests/test_tempo_cpu.py and tests/test_tempo_acf_cpu.py hold to the restatement) on
the PCM the files were written from -- for the MP3, on the PCM the device decoder returns -- record for record and onset for
onset.  Both FLAC decoder routes and a group size that splits the list give the same bytes."""
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
import tempo_cases as tc  # noqa: E402
from wavutil import wav_bytes  # noqa: E402

from mp3rgain_amd import _capi  # noqa: E402
from mp3rgain_amd import replaygain as rgmod  # noqa: E402

pytestmark = pytest.mark.gpu

RG_ERR_IO = -8
REC = C.sizeof(_capi.TempoRecord)
RATE, BPM, SECONDS = 44100, 120, 30
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
    """(wav, flac, mp3 paths, the s16 planes the first two were written from, the MP3 stream's bytes)."""
    import mp3_encoder as E

    tmp = tmp_path_factory.mktemp("tempo")
    x = tc.click_track(BPM, RATE, SECONDS) * 0.9
    planes = [tc.fc.as_format(x * 32768.0, "s16")]
    mp3 = E.encode(x[None, :], RATE, 128, seed=3, allow_ms=False, allow_short=True)
    return (_write(tmp, "click.wav", wav_bytes(planes, RATE, "s16")),
            _write(tmp, "click.flac", flacenc.encode(np.stack(planes).astype(np.int64), RATE, 16, flacenc.Options(block_size=4096))),
            _write(tmp, "click.mp3", mp3), planes, mp3)


def _twin(trs):
    arena, descs, _ = al.pack(trs, al.Layout("abut", "loud", "input"))
    recs, onsets, _ = rgmod.tempo_arena(None, 2, list(descs)[:len(trs)], arena, bands=False)
    return recs, [onsets[r.onsets_at:r.onsets_at + r.onsets] for r in recs]


def _fields(r, skip=("band_frames", "onsets_at")):
    return {f: getattr(r, f) for f, _ in r._fields_ if f not in skip}


def test_files_match_the_host_arithmetic_on_both_decoder_routes_and_in_groups(an, library, tmp_path):
    wav, flac, mp3, planes, stream = library
    pcm, info = an.decode_mp3_device(stream)
    name, data, kept, dropped = next(v for v in flacenc.damaged_variants() if v[0] == "bitflip")
    damaged = _write(tmp_path, "damaged.flac", data)
    missing = tmp_path / "missing.flac"
    files = [wav, flac, mp3, missing, damaged]
    wrecs, wonsets = _twin([Tr("wav", planes, RATE), Tr("flac", planes, RATE), Tr("mp3", [np.ascontiguousarray(ch) for ch in pcm], int(info.sample_rate))])
    raw, recs, onsets = an.tempo_raw(files, onsets_cap=3 * len(wonsets[0]) + 4096)
    assert len(raw) == REC * len(files)
    for k in range(3):
        r, w = recs[k], wrecs[k]
        assert _fields(r) == _fields(w), (files[k].name, _fields(r), _fields(w))
        assert (r.status, r.flags, r.band_frames, r.windows, r.harmonics) == (0, _capi.TEMPO_COMPLETE, 0, (r.onsets - 2048) // 256 + 1, 8)
        assert onsets[r.onsets_at:r.onsets_at + r.onsets].tobytes() == wonsets[k].tobytes(), files[k].name
        assert abs(r.bpm_milli / 1000.0 - BPM) / BPM <= 0.02 and r.stable_permille == 1000 and r.confidence_permille > 500, files[k].name
    assert bytes(recs[0])[:REC - 8] == bytes(recs[1])[:REC - 8] and recs[1].onsets_at == recs[0].onsets  # WAV and FLAC of the same PCM
    assert (recs[2].format, recs[2].frames) == (_capi.FMT_F32_PLANAR, pcm.shape[1]) and recs[0].format == _capi.FMT_S16_PLANAR
    # a failing file fails alone, its record zero apart from `status`
    assert recs[3].status == RG_ERR_IO and raw[REC * 3 + 4:REC * 4] == bytes(REC - 4)
    # a dropped frame: a record (too short for a window), not complete
    d = recs[4]
    assert (d.status, d.dropped_frames) == (0, dropped) and not d.flags & _capi.TEMPO_COMPLETE and d.flags & _capi.TEMPO_SHORT and d.period16 == 0
    an.set_tuning(14, 0)
    host_dec = an.tempo_raw(files, onsets_cap=len(onsets))
    assert host_dec[0] == raw and host_dec[2].tobytes() == onsets.tobytes()
    an.set_tuning(13, 1 << 20)  # several groups
    split = an.tempo_raw(files, onsets_cap=len(onsets))
    assert split[0] == raw and split[2].tobytes() == onsets.tobytes()
    an.set_tuning(14, 1)
    assert an.tempo_raw(files, onsets_cap=len(onsets))[0] == raw


def test_the_python_records_options_and_the_onsets_that_do_not_fit(an, library, tmp_path):
    wav, flac, mp3, planes, _ = library
    missing = tmp_path / "missing.wav"
    res = an.tempo([wav, missing, flac])
    assert [r.error is None for r in res] == [True, False, True] and res[1].error.code == RG_ERR_IO and str(missing) in str(res[1].error)
    assert (res[1].frames, res[1].flags, res[1].onsets, res[1].period16) == (0, 0, 0, 0) and not res[1].found
    a = res[0]
    assert a.found and a.complete and a.verdicts == ["ok"] and abs(a.bpm - BPM) < 0.02 * BPM and a.steady == 1.0 and 0.5 < a.confidence <= 1.0
    # the first click lies at 0.25 s; the grid is coarse: within the spread the tool recorded and a hop
    m = tc.measured()
    period = a.period16 * 32
    off = (tc.FIRST_BEAT * RATE - a.first_beat + period / 2) % period - period / 2
    assert abs(off) <= max(m["click_offset_max"] - m["beat_bias"], m["beat_bias"] - m["click_offset_min"]) + 512
    fast = an.tempo([wav], min_bpm=100)[0]  # [100, 200): still 120
    assert abs(fast.bpm - BPM) < 0.02 * BPM
    slow = an.tempo([wav], min_bpm=50)[0]   # [50, 100): the octave convention reads 60
    assert abs(slow.bpm - BPM / 2) < 0.02 * BPM / 2
    for bad in (dict(window=31), dict(window=64, hop=65), dict(min_bpm=301)):
        with pytest.raises(rgmod.ReplayGainError) as e:
            an.tempo([wav], **bad)
        assert e.value.code == -1
    assert an.tempo([]) == []
    # room for one file's onsets only: the second has none
    raw, recs, onsets = an.tempo_raw([wav, flac], onsets_cap=recs_cap(res[0]))
    assert recs[0].onsets_at == 0 and recs[1].onsets_at == 2 ** 64 - 1 and onsets[:recs[0].onsets].any()
    raw, recs, _ = an.tempo_raw([wav, flac])
    assert all(r.onsets_at == 2 ** 64 - 1 for r in recs)


def recs_cap(r):
    return r.onsets + 5
