"""rg_ancestry on files (include/mp3rgain_amd_ancestry.h): a decoded MP3 stream of this tree's encoder written as FLAC and as
WAV with leading samples trimmed, the same music never coded, the .mp3 itself through the MP3 route, a missing path, a non-audio
file, a 9-channel WAV and a damaged FLAC stream.  The oracle is the serial host twin (rg_ancestry_arena route 0, which
tests/test_ancestry_cpu.py holds to the float64 reference) on the PCM the files were written from, byte for byte; the expected
grid offset is known by construction.  Both FLAC decoder routes and a group size that splits the list give the same bytes."""
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

RG_ERR_IO, RG_ERR_FORMAT = -8, -9
REC = 872
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
    """[(path, Tr of the planes the arena holds, expected grid offset or None)]."""
    tmp = tmp_path_factory.mktemp("ancestry")
    out = []
    dec = ac.real_stream(128, 2, True, True)
    for k, kind in ((0, "flac"), (1, "wav"), (575, "flac"), (2000, "wav")):
        planes = [ac.to_s16(p[k:] * 32768.0) for p in dec]
        data = flacenc.encode(np.stack(planes).astype(np.int64), 44100, 16, flacenc.Options(block_size=1152)) if kind == "flac" else wav_bytes(planes, 44100, "s16")
        out.append((_write(tmp, f"coded_k{k}.{kind}", data), Tr(f"coded_k{k}", planes, 44100), ac.grid_after(k)))
    mono = ac.real_stream(64, 1, False, False)
    planes = [ac.to_s16(mono[0][31:] * 32768.0).astype(np.int32) << 16]  # 16-bit audio in a 24-bit FLAC: left-justified in 32
    out.append((_write(tmp, "coded_mono_k31_24.flac", flacenc.encode(np.stack(planes).astype(np.int64) >> 8, 44100, 24, flacenc.Options(block_size=576))),
                Tr("coded_mono_k31_24", planes, 44100), ac.grid_after(31)))
    clean = [ac.to_s16(ac.music(12000, 50)), ac.to_s16(ac.music(12000, 51))]
    out.append((_write(tmp, "clean.flac", flacenc.encode(np.stack(clean).astype(np.int64), 44100, 16, flacenc.Options(block_size=1152))), Tr("clean_flac", clean, 44100), None))
    out.append((_write(tmp, "clean.wav", wav_bytes(clean[:1], 44100, "s16")), Tr("clean_wav", clean[:1], 44100), None))
    return out


def _records(raw, n):
    assert len(raw) == REC * n
    return [_capi.AncestryRecord.from_buffer_copy(raw[REC * k:REC * k + REC]) for k in range(n)]


def _twin(trs, opts=()):
    arena, descs, _ = al.pack(trs, al.Layout("abut", "loud", "input"))
    return rgmod.ancestry_arena(None, 0, list(descs)[:len(trs)], arena, *opts)[0]


@pytest.mark.parametrize("opts", ((), (2, 3), (0, 1)), ids=("defaults", "s2_g3", "whole"))
def test_files_match_the_host_twin_on_both_decoder_routes_and_in_groups(an, library, opts):
    files, trs = [p for p, _, _ in library], [tr for _, tr, _ in library]
    raw = an.ancestry_raw(files, *opts)
    recs = _records(raw, len(files))
    for r, w, (_, tr, offset) in zip(recs, _twin(trs, opts), library):
        assert r.status == 0, (tr.name, r.status)
        assert bytes(r) == bytes(w), (tr.name, r.flags, w.flags, r.grid_offset, w.grid_offset)
        if offset is None:
            assert not r.flags & _capi.ANC_MP3_GRID and r.flags & _capi.ANC_COMPLETE, tr.name
        else:
            assert r.flags & _capi.ANC_MP3_GRID and r.grid_offset == offset, (tr.name, r.grid_offset, offset)
    an.set_tuning(14, 0)
    assert an.ancestry_raw(files, *opts) == raw
    an.set_tuning(13, 1 << 16)  # several groups
    assert an.ancestry_raw(files, *opts) == raw
    an.set_tuning(14, 1)
    assert an.ancestry_raw(files, *opts) == raw


def test_the_python_records(an, library):
    files = [p for p, tr, _ in library if tr.name in ("coded_k1", "clean_flac")]
    coded, clean = an.ancestry(files)
    assert coded.error is None and coded.mp3_grid and coded.grid_offset == 480 and coded.complete and coded.summary.startswith("mp3 grid at +480 (z ")
    assert [v.name for v in coded.views] == ["ch0", "ch1", "mid", "side"] and coded.views[coded.best_view].flagged
    assert clean.error is None and not clean.mp3_grid and clean.summary == "no grid found" and clean.best_view is None
    for bad in (dict(segments=1, granules=0), dict(z_min=-1.0)):
        with pytest.raises(rgmod.ReplayGainError) as e:
            an.ancestry(files, **bad)
        assert e.value.code == -1


def test_the_mp3_itself_is_flagged_at_481(an, tmp_path):
    """Through the MP3 route the planes are floats; the twin runs on the PCM the device decoder returns."""
    data = ac.real_stream_bytes(128, 2, True, True)
    f = _write(tmp_path, "stream.mp3", data)
    pcm, info = an.decode_mp3_device(data)
    tr = rgmod.PcmTrack([np.ascontiguousarray(ch) for ch in pcm], int(info.sample_rate))
    arena, descs = rgmod.pack_tracks([tr])
    want = rgmod.ancestry_arena(None, 0, list(descs)[:1], arena)[0][0]
    got = _capi.AncestryRecord.from_buffer_copy(an.ancestry_raw([f]))
    assert bytes(got) == bytes(want), (got.flags, want.flags, got.grid_offset, want.grid_offset)
    assert (got.format, got.channels, got.frames) == (_capi.FMT_F32_PLANAR, pcm.shape[0], pcm.shape[1])
    assert got.flags & _capi.ANC_MP3_GRID and got.flags & _capi.ANC_COMPLETE and got.grid_offset == 481


def test_failing_files_fail_alone(an, tmp_path, library):
    rng = np.random.default_rng(72)
    nine = _write(tmp_path, "nine.wav", wav_bytes([rng.integers(-100, 100, 500) for _ in range(9)], 48000, "s16"))
    text = _write(tmp_path, "notes.txt", b"not audio at all\n" * 40)
    missing = tmp_path / "missing.flac"
    good = [library[1], library[5], library[4]]
    files = [good[0][0], missing, good[1][0], nine, good[2][0], text]
    an.set_decoder_command("false {}")  # a decoder command is set and must not be run
    try:
        res = an.ancestry(files)
        raw = an.ancestry_raw(files)
    finally:
        an.set_decoder_command(None)
    recs = _records(raw, len(files))
    for r, w in zip([recs[k] for k in (0, 2, 4)], _twin([tr for _, tr, _ in good])):
        assert bytes(r) == bytes(w)
    for k, code, needle in ((1, RG_ERR_IO, "Failed to open"), (3, RG_ERR_FORMAT, "9 channels"), (5, None, "")):
        r = res[k]
        assert r.error is not None and (code is None or r.error.code == code) and needle in str(r.error) and str(files[k]) in str(r.error), (k, str(r.error))
        assert (r.frames, r.flags, r.views, r.grid_offset, r.z) == (0, 0, [], 0, 0.0) and r.best_view is None
        assert recs[k].status == r.error.code and raw[REC * k + 4:REC * k + REC] == bytes(REC - 4)  # zero apart from `status`
    assert an.ancestry([]) == []


def test_dropped_frames_clear_complete(an, tmp_path):
    from mp3rgain_amd import flacdec

    name, data, kept, dropped = next(v for v in flacenc.damaged_variants() if v[0] == "bitflip")
    _, _, host, hi = flacdec.decode(data)
    assert dropped == 1 and int(hi.dropped_frames) == 1
    p = _write(tmp_path, "damaged.flac", data)
    for key14 in (1, 0):
        an.set_tuning(14, key14)
        r = an.ancestry([p])[0]
        assert r.error is None and r.dropped_frames == 1 and not r.complete and r.frames == host.shape[1] and "incomplete" in r.verdicts
