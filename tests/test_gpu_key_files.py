"""rg_key on files (include/mp3rgain_amd_key.h): a 20 s chord progression in A minor as WAV, as FLAC and as a stream of this tree's
MP3 encoder, a missing path and a FLAC stream with a dropped frame.  The oracle is the kernels' arithmetic on the host with the
host's stage 2 (rg_key_arena route 2, which tests/test_key_cpu.py and tests/test_key_stage2_cpu.py hold to the restatement) on the
PCM the files were written from -- for the MP3, on the PCM the device decoder returns -- record for record and row for row.  All
three read the generating key.  Both FLAC decoder routes and a group size that splits the list give the same bytes."""
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
import key_cases as kc  # noqa: E402
from wavutil import wav_bytes  # noqa: E402

from mp3rgain_amd import _capi  # noqa: E402
from mp3rgain_amd import replaygain as rgmod  # noqa: E402

pytestmark = pytest.mark.gpu

RG_ERR_IO = -8
REC = C.sizeof(_capi.KeyRecord)
RATE, KEY, SECONDS = 44100, 21, 20
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

    tmp = tmp_path_factory.mktemp("key")
    x = kc.progression(KEY, RATE, SECONDS) * 0.9
    planes = [kc.fc.as_format(x * 32768.0, "s16")]
    mp3 = E.encode(x[None, :], RATE, 128, seed=3, allow_ms=False, allow_short=True)
    return (_write(tmp, "am.wav", wav_bytes(planes, RATE, "s16")),
            _write(tmp, "am.flac", flacenc.encode(np.stack(planes).astype(np.int64), RATE, 16, flacenc.Options(block_size=4096))),
            _write(tmp, "am.mp3", mp3), planes, mp3)


def _twin(trs, segment=None):
    arena, descs, _ = al.pack(trs, al.Layout("abut", "loud", "input"))
    recs, _, _, chroma = rgmod.key_arena(None, 2, list(descs)[:len(trs)], arena, segment=segment, bands=False)
    return recs, [chroma[r.chroma_at:r.chroma_at + r.rows] for r in recs]


def _fields(r, skip=("chroma_at",)):
    return {f: getattr(r, f) for f, _ in r._fields_ if f not in skip}


def test_files_match_the_host_arithmetic_on_both_decoder_routes_and_in_groups(an, library, tmp_path):
    wav, flac, mp3, planes, stream = library
    pcm, info = an.decode_mp3_device(stream)
    name, data, kept, dropped = next(v for v in flacenc.damaged_variants() if v[0] == "bitflip")
    damaged = _write(tmp_path, "damaged.flac", data)
    missing = tmp_path / "missing.flac"
    files = [wav, flac, mp3, missing, damaged]
    wrecs, wrows = _twin([Tr("wav", planes, RATE), Tr("flac", planes, RATE), Tr("mp3", [np.ascontiguousarray(ch) for ch in pcm], int(info.sample_rate))])
    raw, recs, chroma = an.key_raw(files, chroma_cap=3 * len(wrows[0]) + 512)
    assert len(raw) == REC * len(files)
    for k in range(3):
        r, w = recs[k], wrecs[k]
        assert _fields(r) == _fields(w), (files[k].name, _fields(r), _fields(w))
        assert (r.status, r.flags, r.decim, r.key, r.tonic, r.mode) == (0, _capi.KEY_COMPLETE, 8, KEY, 9, 1), files[k].name
        assert chroma[r.chroma_at:r.chroma_at + r.rows].tobytes() == wrows[k].tobytes(), files[k].name
        assert r.correlation_permille > 700 and r.margin_permille > 50 and r.rows == (r.decimated - 4096) // 512 + 1
    assert bytes(recs[0])[:REC - 8] == bytes(recs[1])[:REC - 8] and recs[1].chroma_at == recs[0].rows  # WAV and FLAC of the same PCM
    assert (recs[2].format, recs[2].frames) == (_capi.FMT_F32_PLANAR, pcm.shape[1]) and recs[0].format == _capi.FMT_S16_PLANAR
    # a failing file fails alone, its record zero apart from `status`
    assert recs[3].status == RG_ERR_IO and raw[REC * 3 + 4:REC * 4] == bytes(REC - 4)
    # a dropped frame: a record, not complete
    d = recs[4]
    assert (d.status, d.dropped_frames) == (0, dropped) and not d.flags & _capi.KEY_COMPLETE
    an.set_tuning(14, 0)
    host_dec = an.key_raw(files, chroma_cap=len(chroma))
    assert host_dec[0] == raw and host_dec[2].tobytes() == chroma.tobytes()
    an.set_tuning(13, 1 << 20)  # several groups
    split = an.key_raw(files, chroma_cap=len(chroma))
    assert split[0] == raw and split[2].tobytes() == chroma.tobytes()
    an.set_tuning(14, 1)
    assert an.key_raw(files, chroma_cap=len(chroma))[0] == raw


def test_the_python_records_options_and_the_rows_that_do_not_fit(an, library, tmp_path):
    wav, flac, mp3, planes, _ = library
    missing = tmp_path / "missing.wav"
    res = an.key([wav, missing, flac])
    assert [r.error is None for r in res] == [True, False, True] and res[1].error.code == RG_ERR_IO and str(missing) in str(res[1].error)
    assert (res[1].frames, res[1].flags, res[1].rows, res[1].key) == (0, 0, 0, 0) and not res[1].found and res[1].name is None
    a = res[0]
    assert a.found and a.complete and a.verdicts == ["ok"] and (a.name, a.camelot, a.open_key) == ("A minor", "8A", "1m") and 0.7 < a.correlation <= 1.0
    short = an.key([wav], segment=16)[0]
    want = _twin([Tr("wav", planes, RATE)], segment=16)[0][0]
    assert (short.key, short.segments, short.stable_permille) == (KEY, a.rows // 16, want.stable_permille) and short.segments > a.segments
    for bad in (7, 4097):
        with pytest.raises(rgmod.ReplayGainError) as e:
            an.key([wav], segment=bad)
        assert e.value.code == -1
    assert an.key([]) == []
    # room for one file's rows only: the second has none
    raw, recs, chroma = an.key_raw([wav, flac], chroma_cap=a.rows + 5)
    assert recs[0].chroma_at == 0 and recs[1].chroma_at == 2 ** 64 - 1 and chroma[:recs[0].rows].any()
    raw, recs, _ = an.key_raw([wav, flac])
    assert all(r.chroma_at == 2 ** 64 - 1 for r in recs)
