"""rg_clicks on files (include/mp3rgain_amd_clicks.h): a handful of sub-second generated WAV files (16 and 24-bit, float; mono,
stereo and 5.1), FLAC at 16 and 24 bits, and an MP3 made by the project's own encoder.  The oracle is the serial host twin
(rg_clicks_arena route 0, which tests/test_clicks_cpu.py holds to the restatement) on the PCM the files were written from, byte
for byte, records and event lists; for the MP3, the twin on the PCM the device decoder returns.  Both FLAC decoder routes
(tuning key 14 = 1 and 0) and a group size that splits the list give the same bytes.  The six-file mix of
tests/test_gpu_pcm_scan_groups.py -- two clean files, one with a dropped frame, three that fail each in its own way -- goes
through the same call."""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "oracle"))
import arena_layouts as al  # noqa: E402
import clicks_cases as cc  # noqa: E402
import flacenc  # noqa: E402
import wavutil  # noqa: E402
from wavutil import planar_for_oracle, wav_bytes  # noqa: E402

from mp3rgain_amd import _capi  # noqa: E402
from mp3rgain_amd import replaygain as rgmod  # noqa: E402

pytestmark = pytest.mark.gpu

GOLD = Path(__file__).resolve().parent / "golden"
RG_ERR_IO, RG_ERR_FORMAT = -8, -9
REC, EV = C.sizeof(_capi.ClicksRecord), C.sizeof(_capi.ClicksEvent)
OPTS = (cc.Opts(), cc.Opts(block_samples=256, order=2, ratio_permille=6000, max_events=5), cc.Opts(block_samples=4096, order=12, max_events=0))


def _kw(o):
    return dict(block_samples=o.block_samples, order=o.order, ratio_permille=o.ratio_permille, max_events=o.max_events)


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


def _ticked(rng, n, nch, places):
    """q of a tone mix per channel, a tick at each of `places` in the channels they name."""
    chans = [cc.tonal(rng, n) for _ in range(nch)]
    for c, p, a in places:
        chans[c][p] += a
    return [np.clip(v, -32768, 32767) for v in chans]


@pytest.fixture(scope="module")
def library(tmp_path_factory):
    """[(path, Tr of the planes the arena holds)]."""
    tmp = tmp_path_factory.mktemp("clicks")
    rng = np.random.default_rng(79)
    out = []
    for k, (kind, nch) in enumerate((("s16", 2), ("s24", 6), ("f32", 1), ("f32", 2), ("s16", 1), ("s24", 2))):
        n = 5000 + 700 * k + 7
        q = _ticked(rng, n, nch, [(0, 1500, 9000), (nch - 1, 1500, -8000), (0, 4000 + k, 12000)])
        if kind == "f32":
            chans = [(v / 32768.0).astype(np.float32) for v in q]
            if nch == 2:
                chans[1][301] = np.float32(np.nan)
        elif kind == "s24":
            chans = [(v * 256 + 77).astype(np.int32) for v in q]
        else:
            chans = [v.astype(np.int16) for v in q]
        out.append((_write(tmp, f"{k}_{kind}_{nch}.wav", wav_bytes(chans, 48000, kind)), cc.Tr(f"wav_{kind}_{nch}", planar_for_oracle(chans, kind), 48000)))
    for name, bps in (("plain16", 16), ("plain24", 24)):
        n = 3 * 1152 + 301
        q = _ticked(rng, n, 2, [(1, 2000, 10000)])
        pcm = np.stack([v << (bps - 16) for v in q]).astype(np.int64)
        dt, w = (np.int16, 16) if bps <= 16 else (np.int32, 32)
        planes = [(pcm[ch] << (w - bps)).astype(dt) for ch in range(2)]
        out.append((_write(tmp, f"{name}.flac", flacenc.encode(pcm, 44100, bps, flacenc.Options(block_size=1152))), cc.Tr(f"flac_{name}", planes, 44100)))
    return out


def _records(raw, n):
    assert len(raw) == REC * n
    return [_capi.ClicksRecord.from_buffer_copy(raw[REC * k:REC * k + REC]) for k in range(n)]


def _twin(trs, o):
    arena, descs, _ = al.pack(trs, al.Layout("abut", "loud", "input"))
    return rgmod.clicks_arena(None, 0, list(descs)[:len(trs)], arena, **_kw(o))


@pytest.mark.parametrize("o", OPTS, ids=lambda o: f"b{o.block_samples}-p{o.order}-k{o.max_events}")
def test_files_match_the_host_twin_on_both_decoder_routes_and_in_groups(an, library, o):
    files, trs = [p for p, _ in library], [tr for _, tr in library]
    raw, rows = an.clicks_raw(files, **_kw(o))
    recs = _records(raw, len(files))
    want, want_rows = _twin(trs, o)
    K = o.max_events
    for k, (r, w, tr) in enumerate(zip(recs, want, trs)):
        assert r.status == 0, (tr.name, r.status)
        assert bytes(r) == bytes(w), (tr.name, cc.got(r, []), cc.got(w, []))
        row = (_capi.ClicksEvent * max(1, K)).from_buffer_copy(rows[EV * K * k:EV * K * (k + 1)].ljust(EV * max(1, K), b"\0"))
        assert not cc.differences(cc.got(r, list(row)[:K]), cc.want_track(tr, o)), tr.name
    assert rows == bytes(want_rows)[:len(files) * K * EV]
    by_name = {tr.name: r for r, tr in zip(recs, trs)}
    assert by_name["wav_f32_2"].flags & _capi.CK_NONFINITE and by_name["wav_f32_2"].nonfinite == 1
    assert by_name["wav_s24_6"].channels == 6 and by_name["wav_s24_6"].ch[5].clicks >= 1 and by_name["wav_s24_6"].ch[2].clicks == 0
    assert by_name["flac_plain24"].ch[1].clicks >= 1
    assert by_name["flac_plain24"].ch[0].flagged == 0 or o.ratio_permille < 8000  # (the second option set flags at 6 x the scale)
    an.set_tuning(14, 0)
    assert an.clicks_raw(files, **_kw(o)) == (raw, rows)
    an.set_tuning(13, 1 << 18)  # a file or two per group
    assert an.clicks_raw(files, **_kw(o)) == (raw, rows)
    an.set_tuning(14, 1)
    assert an.clicks_raw(files, **_kw(o)) == (raw, rows)


def test_the_python_records_and_the_options(an, library):
    paths = {tr.name: p for p, tr in library}
    files = [paths[name] for name in ("wav_s16_2", "wav_f32_1", "flac_plain16")]
    res = an.clicks(files, max_events=4)
    raw = _records(an.clicks_raw(files, max_events=4)[0], 3)
    for d, r in zip(res, raw):
        assert d.error is None and d.complete and (d.max_events, d.block_samples, d.events_total, d.listed) == (4, 1024, r.events, r.listed)
        assert [c.clicks for c in d.ch] == [r.ch[c].clicks for c in range(r.channels)] and len(d.events) == d.listed
    assert res[0].clicks == 3 and res[0].first_click[0] in range(1491, 1510) and [e.channel for e in res[0].events[:2]] == [0, 1]
    assert res[2].clicks == 1 and res[2].events[0].channel == 1 and res[2].events[0].kind == "click"
    assert an.clicks(files, ratio_permille=1000000)[0].clicks == 0
    for bad in ({"block_samples": 1000}, {"order": 3}, {"ratio_permille": 10}, {"gap": 0}, {"max_width": 5000}, {"floor": 0}):
        with pytest.raises(rgmod.ReplayGainError) as e:
            an.clicks(files, **bad)
        assert e.value.code == -1


def test_an_mp3_of_the_projects_encoder_matches_the_host_twin_on_the_device_decoders_pcm(an, tmp_path):
    import mp3_encoder as E

    rng = np.random.default_rng(7)
    x = cc.tonal(rng, 6000).astype(np.float64)
    x[3000] += 12000.0
    f = _write(tmp_path, "ticked.mp3", E.encode(np.stack([x, x[::-1]]) / 32768.0, 44100, 128, seed=3))
    pcm, info = an.decode_mp3_device(f.read_bytes())
    tr = rgmod.PcmTrack([np.ascontiguousarray(ch) for ch in pcm], int(info.sample_rate))
    arena, descs = rgmod.pack_tracks([tr])
    for o in (cc.Opts(), cc.Opts(block_samples=512, order=4, ratio_permille=8000, max_events=7)):
        want, want_rows = rgmod.clicks_arena(None, 0, list(descs)[:1], arena, **_kw(o))
        raw, rows = an.clicks_raw([f], **_kw(o))
        got = _capi.ClicksRecord.from_buffer_copy(raw)
        assert bytes(got) == bytes(want[0]), (cc.got(got, []), cc.got(want[0], []))
        assert rows == bytes(want_rows)[:o.max_events * EV]
        assert (got.format, got.channels, got.frames) == (_capi.FMT_F32_PLANAR, pcm.shape[0], pcm.shape[1]) and got.flags & _capi.CK_COMPLETE


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
        res = an.clicks(files)
        raw, rows = an.clicks_raw(files)
    finally:
        an.set_decoder_command(None)
    recs = _records(raw, 6)
    K = _capi.CK_DEFAULT_MAX_EVENTS
    refused = {1: (RG_ERR_IO, f"Failed to open: {files[1]}"),
               2: (RG_ERR_FORMAT, f"No click scan (9 channels, more than 8): {files[2]}"),
               3: (RG_ERR_FORMAT, f"No click scan (64-bit float, not 8, 16, 24 or 32-bit integer or 32-bit float PCM): {files[3]}")}
    for k, (code, text) in refused.items():
        assert res[k].error is not None and (res[k].error.code, str(res[k].error)) == (code, text), (k, str(res[k].error))
        assert recs[k].status == code and raw[REC * k + 4:REC * (k + 1)] == bytes(REC - 4), k
        assert res[k].dropped_frames == 0 and rows[EV * K * k:EV * K * (k + 1)] == bytes(EV * K)
    keys = sorted(pcm)
    arena, descs = rgmod.pack_tracks([rgmod.PcmTrack(pcm[k][0], pcm[k][1]) for k in keys])
    want, want_rows = rgmod.clicks_arena(None, 0, list(descs)[:len(keys)], arena)
    for j, (k, w) in enumerate(zip(keys, want)):
        lost = pcm[k][2]
        assert res[k].error is None and recs[k].status == 0, (k, str(res[k].error))
        assert res[k].dropped_frames == recs[k].dropped_frames == lost, (k, recs[k].dropped_frames)
        assert (recs[k].frames, recs[k].channels, recs[k].sample_rate) == (len(pcm[k][0][0]), len(pcm[k][0]), pcm[k][1]), k
        assert w.status == 0 and w.dropped_frames == 0 and w.flags & _capi.CK_COMPLETE
        w.dropped_frames = lost
        if lost:
            w.flags &= ~_capi.CK_COMPLETE
        assert bytes(recs[k]) == bytes(w), (k, cc.got(recs[k], []), cc.got(w, []))
        assert rows[EV * K * k:EV * K * (k + 1)] == bytes(want_rows)[EV * K * j:EV * K * (j + 1)], k
        assert res[k].complete == (lost == 0)
    assert an.clicks([]) == []
