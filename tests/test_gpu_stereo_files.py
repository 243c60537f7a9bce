"""rg_stereo on files (include/mp3rgain_amd_stereo.h): a handful of sub-second generated WAV files in mono, stereo and 5.1, FLAC
at 16 and 24 bits and an MP3 from the goldens.  The oracle is the serial host twin (rg_stereo_arena route 0, which
tests/test_stereo_cpu.py holds to the restatement) on the PCM the files were written from, byte for byte, records and lag sums;
for the MP3, the twin on the PCM the device decoder returns.  Both FLAC decoder routes and a group size that splits the list
give the same bytes.  The six-file mix of tests/test_gpu_pcm_scan_groups.py -- two clean files, one with a dropped frame, three
that fail each in its own way -- goes through the same call."""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import arena_layouts as al  # noqa: E402
import flacenc  # noqa: E402
import stereo_cases as sc  # noqa: E402
import wavutil  # noqa: E402
from wavutil import planar_for_oracle, wav_bytes  # noqa: E402

from mp3rgain_amd import _capi  # noqa: E402
from mp3rgain_amd import replaygain as rgmod  # noqa: E402

pytestmark = pytest.mark.gpu

GOLD = Path(__file__).resolve().parent / "golden"
RG_ERR_IO, RG_ERR_FORMAT = -8, -9
REC = C.sizeof(_capi.StereoRecord)
OPTS = ((None, None), (7, 1000), (255, 4097))  # (radius, block_frames)


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
    """[(path, Tr of the planes the arena holds)]: WAV of every kind in mono, stereo and 5.1, a WAV whose right channel is late, and
    two FLAC files."""
    tmp = tmp_path_factory.mktemp("stereo")
    rng = np.random.default_rng(73)
    out = []
    for k, (kind, nch) in enumerate((("u8", 2), ("s16", 2), ("s24", 6), ("s32", 2), ("f32", 1), ("f32", 2), ("s16", 1), ("s24", 2))):
        n = 9000 + 1000 * k + 7
        chans = wavutil.test_signal(kind, 48000, n, nch, 90 + k)
        if kind == "f32" and nch == 2:
            chans[0][300] = np.float32(1.5)
            chans[1][301] = np.float32(np.nan)
        out.append((_write(tmp, f"{k}_{kind}_{nch}.wav", wav_bytes(chans, 48000, kind)), sc.Tr(f"wav_{kind}_{nch}", planar_for_oracle(chans, kind), 48000)))
    x = rng.integers(-20000, 20000, size=5003).astype(np.int16)
    late = [x, sc.delayed(x, 3)]
    out.append((_write(tmp, "late.wav", wav_bytes(late, 44100, "s16")), sc.Tr("wav_late", planar_for_oracle(late, "s16"), 44100)))
    for name, bps in (("plain16", 16), ("plain24", 24)):
        n = 3 * 1152 + 301
        pcm = flacenc.test_pcm(rng, 2, n, bps)
        dt, w = (np.int16, 16) if bps <= 16 else (np.int32, 32)
        planes = [(pcm[ch].astype(np.int64) << (w - bps)).astype(dt) for ch in range(2)]
        out.append((_write(tmp, f"{name}.flac", flacenc.encode(pcm, 44100, bps, flacenc.Options(block_size=1152))), sc.Tr(f"flac_{name}", planes, 44100)))
    return out


def _records(raw, n):
    assert len(raw) == REC * n
    return [_capi.StereoRecord.from_buffer_copy(raw[REC * k:REC * k + REC]) for k in range(n)]


def _twin(trs, opts):
    arena, descs, _ = al.pack(trs, al.Layout("abut", "loud", "input"))
    return rgmod.stereo_arena(None, 0, list(descs)[:len(trs)], arena, *opts, lag_sums=True)


@pytest.mark.parametrize("opts", OPTS, ids=lambda o: f"{o[0]}-{o[1]}")
def test_files_match_the_host_twin_on_both_decoder_routes_and_in_groups(an, library, opts):
    files, trs = [p for p, _ in library], [tr for _, tr in library]
    raw, rows = an.stereo_raw(files, *opts, lag_sums=True)
    recs = _records(raw, len(files))
    want, want_rows = _twin(trs, opts)
    for r, w, tr in zip(recs, want, trs):
        assert r.status == 0, (tr.name, r.status)
        assert bytes(r) == bytes(w), (tr.name, sc.differences(sc.got(r), sc.got(w)))
        assert not sc.differences(sc.got(r), sc.want_track(tr, *opts)), tr.name
    assert rows == want_rows.tobytes()
    by_name = {tr.name: r for r, tr in zip(recs, trs)}
    assert by_name["wav_f32_2"].flags & _capi.ST_NONFINITE and by_name["wav_f32_2"].nonfinite == 1
    assert by_name["wav_f32_1"].flags == _capi.ST_COMPLETE | _capi.ST_MONO and by_name["wav_s16_1"].flags == _capi.ST_COMPLETE | _capi.ST_MONO
    assert by_name["wav_s24_6"].flags & _capi.ST_MORE_CHANNELS and by_name["wav_s24_6"].channels == 6
    assert by_name["wav_late"].flags & _capi.ST_DELAYED and by_name["wav_late"].lag == 3
    an.set_tuning(14, 0)
    assert an.stereo_raw(files, *opts, lag_sums=True) == (raw, rows)
    an.set_tuning(13, 1 << 18)  # a file or two per group
    assert an.stereo_raw(files, *opts, lag_sums=True) == (raw, rows)
    an.set_tuning(14, 1)
    assert an.stereo_raw(files, *opts, lag_sums=True) == (raw, rows)
    assert an.stereo_raw(files, *opts) == raw  # the rows are optional


def test_the_python_records_and_the_options(an, library):
    paths = {tr.name: p for p, tr in library}
    files = [paths[name] for name in ("wav_s16_2", "wav_late", "wav_f32_1")]
    res, rows = an.stereo(files, radius=5, block_frames=1000, lag_sums=True)
    raw = _records(an.stereo_raw(files, 5, 1000), 3)
    assert rows.shape == (3, 11)
    for d, r, row in zip(res, raw, rows):
        assert d.error is None and d.complete and (d.radius, d.block_frames, d.ell, d.elr, d.lag, d.correlation) == (5, 1000, r.ell, r.elr, r.lag, r.correlation)
        assert int(row[5]) == d.elr and int(row[5 + d.lag]) == d.lag_sum
    assert res[1].verdicts == ["delayed"] and res[2].verdicts == ["mono file"] and not rows[2].any()
    assert an.stereo(files, delay_permille=1000)[1].verdicts == ["stereo"]
    for bad in ({"radius": 256}, {"block_frames": sc.MAX_BLOCK + 1}, {"phase_permille": 0}, {"balance_db_limit": 1001}):
        with pytest.raises(rgmod.ReplayGainError) as e:
            an.stereo(files, **bad)
        assert e.value.code == -1


def test_an_mp3_file_matches_the_host_twin_on_the_device_decoders_pcm(an):
    f = GOLD / "mp3" / "v1_44k_ms_mixed.mp3"
    pcm, info = an.decode_mp3_device(f.read_bytes())
    tr = rgmod.PcmTrack([np.ascontiguousarray(ch) for ch in pcm], int(info.sample_rate))
    arena, descs = rgmod.pack_tracks([tr])
    for opts in ((None, None), (17, 4000)):
        want, want_rows = rgmod.stereo_arena(None, 0, list(descs)[:1], arena, *opts, lag_sums=True)
        raw, rows = an.stereo_raw([f], *opts, lag_sums=True)
        got = _capi.StereoRecord.from_buffer_copy(raw)
        assert bytes(got) == bytes(want[0]), sc.differences(sc.got(got), sc.got(want[0]))
        assert rows == want_rows.tobytes()
        assert (got.format, got.channels, got.frames) == (_capi.FMT_F32_PLANAR, pcm.shape[0], pcm.shape[1]) and got.flags & _capi.ST_COMPLETE


def _f64_wav(frames):
    """a 2-channel WAV of 64-bit floats: a sample kind the staging does not lay out"""
    import struct

    body = np.zeros(2 * frames, "<f8").tobytes()
    fmt = struct.pack("<HHIIHH", 3, 2, 44100, 44100 * 16, 16, 64)
    chunks = b"fmt " + struct.pack("<I", len(fmt)) + fmt + b"data" + struct.pack("<I", len(body)) + body
    return b"RIFF" + struct.pack("<I", 4 + len(chunks)) + b"WAVE" + chunks


def test_six_files_one_call(an, tmp_path):
    """Status, the whole text, the dropped frames and the records of the mix the other PCM scans are held to."""
    good = wavutil.test_signal("s16", 44100, 4000, 2, 5)
    _, stream, kept, dropped = next(v for v in flacenc.damaged_variants() if v[0] == "bitflip")
    assert dropped == 1
    mp3 = min((GOLD / "mp3").glob("*.mp3"), key=lambda p: (p.stat().st_size, p.name))
    files = [_write(tmp_path, "good.wav", wavutil.wav_bytes(good, 44100, "s16")), tmp_path / "missing.wav",
             _write(tmp_path, "nine.wav", wavutil.wav_bytes([np.arange(8) + c for c in range(9)], 44100, "s16")), _write(tmp_path, "doubles.wav", _f64_wav(8)),
             _write(tmp_path, "bitflip.flac", stream), mp3]
    decoded, info = an.decode_mp3_device(mp3.read_bytes())
    pcm = {0: (wavutil.planar_for_oracle(good, "s16"), 44100, 0), 4: ([kept[c].astype(np.int16) for c in range(2)], 44100, 1),
           5: ([np.ascontiguousarray(ch) for ch in decoded], int(info.sample_rate), 0)}
    an.set_decoder_command("false {}")  # a decoder command is set and must not be run
    try:
        res, rows = an.stereo(files, lag_sums=True)
        raw, raw_rows = an.stereo_raw(files, lag_sums=True)
    finally:
        an.set_decoder_command(None)
    assert rows.tobytes() == raw_rows
    recs = _records(raw, 6)
    refused = {1: (RG_ERR_IO, f"Failed to open: {files[1]}"),
               2: (RG_ERR_FORMAT, f"No stereo scan (9 channels, more than 8): {files[2]}"),
               3: (RG_ERR_FORMAT, f"No stereo scan (64-bit float, not 8, 16, 24 or 32-bit integer or 32-bit float PCM): {files[3]}")}
    for k, (code, text) in refused.items():
        assert res[k].error is not None and (res[k].error.code, str(res[k].error)) == (code, text), (k, str(res[k].error))
        assert recs[k].status == code and raw[REC * k + 4:REC * (k + 1)] == bytes(REC - 4), k
        assert res[k].dropped_frames == 0 and not rows[k].any()
    keys = sorted(pcm)
    arena, descs = rgmod.pack_tracks([rgmod.PcmTrack(pcm[k][0], pcm[k][1]) for k in keys])
    want, want_rows = rgmod.stereo_arena(None, 0, list(descs)[:len(keys)], arena, lag_sums=True)
    for k, w, wrow in zip(keys, want, want_rows):
        lost = pcm[k][2]
        assert res[k].error is None and recs[k].status == 0, (k, str(res[k].error))
        assert res[k].dropped_frames == recs[k].dropped_frames == lost, (k, recs[k].dropped_frames)
        assert (recs[k].frames, recs[k].channels, recs[k].sample_rate) == (len(pcm[k][0][0]), len(pcm[k][0]), pcm[k][1]), k
        assert w.status == 0 and w.dropped_frames == 0 and w.flags & _capi.ST_COMPLETE
        w.dropped_frames = lost
        if lost:
            w.flags &= ~_capi.ST_COMPLETE
        assert bytes(recs[k]) == bytes(w), (k, sc.differences(sc.got(recs[k]), sc.got(w)))
        assert rows[k].tobytes() == wrow.tobytes(), k
        assert res[k].complete == (lost == 0)
    assert an.stereo([]) == []
