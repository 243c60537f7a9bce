"""rg_pcm_stats on files (include/mp3rgain_amd_stats.h): generated WAV files of every kind the library reads, FLAC at 16 and 24
bits, an MP3 from the goldens, a missing path and a 9-channel WAV among them.  The oracle is the numpy restatement
(tests/pcm_stats_cases.py) on the PCM the files were written from; for the MP3, the serial host twin on the PCM the device
decoder returns.  Both FLAC decoder routes and a group size that splits the list give the same bytes."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import flacenc  # noqa: E402
import pcm_stats_cases as pc  # noqa: E402
import wavutil  # noqa: E402
from wavutil import planar_for_oracle, wav_bytes  # noqa: E402

from mp3rgain_amd import _capi  # noqa: E402
from mp3rgain_amd import replaygain as rgmod  # noqa: E402

pytestmark = pytest.mark.gpu

GOLD = Path(__file__).resolve().parent / "golden"
RG_ERR_IO, RG_ERR_FORMAT = -8, -9
REC = 48 + 8 * 72


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
    """[(path, Tr of the planes the arena holds)]: WAV of every kind in mono, stereo and 5.1, and four FLAC files."""
    tmp = tmp_path_factory.mktemp("stats")
    rng = np.random.default_rng(51)
    c, t, f = pc.shape()
    out = []
    for k, (kind, bits, nch) in enumerate((("u8", 8, 1), ("s16", 16, 2), ("s24", 24, 6), ("s32", 32, 2), ("f32", 32, 1), ("f32", 32, 6), ("s16", 16, 6),
                                           ("u8", 8, 2), ("s24", 24, 1))):
        n = t + 1000 * k + 7
        chans = wavutil.test_signal(kind, 48000, n, nch, 60 + k)
        full = {"u8": 255, "s16": 32767, "s24": 8388607, "s32": 2147483647, "f32": np.float32(1.0)}[kind]
        zero = 128 if kind == "u8" else 0
        chans[0][100:105] = full                 # a clip run
        chans[-1][2000:2000 + 70] = zero         # a dropout in one channel
        for ch in chans:                         # edge silence in every channel
            ch[:11] = zero
            ch[-6:] = zero
        if kind == "f32":
            chans[0][300] = np.float32(1.5)
            chans[0][301] = np.float32(np.nan)
        out.append((_write(tmp, f"{k}_{kind}_{nch}.wav", wav_bytes(chans, 48000, kind)), pc.Tr(f"wav_{kind}_{nch}", planar_for_oracle(chans, kind), 48000, bits)))
    for name, bps, held, gap in (("plain16", 16, 16, 0), ("plain24", 24, 24, 0), ("padded", 24, 16, 0), ("gap", 16, 16, 2000)):
        n = 3 * 1152 + 301
        pcm = flacenc.test_pcm(rng, 2, n, held)
        if held != bps:
            pcm = pcm << (bps - held)  # 16-bit audio in a 24-bit stream
        if gap:
            pcm[:, 1500:1500 + gap] = 0
        dt, w = (np.int16, 16) if bps <= 16 else (np.int32, 32)
        planes = [(pcm[ch].astype(np.int64) << (w - bps)).astype(dt) for ch in range(2)]
        out.append((_write(tmp, f"{name}.flac", flacenc.encode(pcm, 44100, bps, flacenc.Options(block_size=1152))), pc.Tr(f"flac_{name}", planes, 44100, bps)))
    return out


def _check(recs, library):
    for r, (path, tr) in zip(recs, library):
        assert r.status == 0, (path.name, r.status)
        bad = pc.differences(pc.got(r), pc.want_track(tr, 3, 64))
        assert not bad, (path.name, bad[:4])


def test_files_match_the_restatement_on_both_decoder_routes_and_in_groups(an, library):
    files = [p for p, _ in library]
    raw = an.pcm_stats_raw(files)
    assert len(raw) == REC * len(files)
    recs = [_capi.PcmStatsRecord.from_buffer_copy(raw[REC * k:REC * k + REC]) for k in range(len(files))]
    _check(recs, library)
    by_name = {tr.name: r for r, (_, tr) in zip(recs, library)}
    assert by_name["flac_padded"].flags & _capi.STATS_PADDED and not by_name["flac_plain24"].flags & _capi.STATS_PADDED
    assert by_name["flac_gap"].flags & _capi.STATS_DROPOUT and by_name["flac_gap"].ch[0].longest_zero_run >= 2000
    assert not by_name["flac_plain16"].flags & _capi.STATS_DROPOUT
    assert by_name["wav_f32_1"].flags & _capi.STATS_NONFINITE and by_name["wav_s24_6"].flags & _capi.STATS_CLIPPED
    assert (by_name["wav_s24_6"].lead_silence_frames, by_name["wav_s24_6"].trail_silence_frames, by_name["wav_s24_6"].channels) == (11, 6, 6)
    an.set_tuning(14, 0)
    assert an.pcm_stats_raw(files) == raw
    an.set_tuning(13, 1 << 20)  # a file or two per group
    assert an.pcm_stats_raw(files) == raw
    an.set_tuning(14, 1)
    assert an.pcm_stats_raw(files) == raw
    # the Python results say the same
    res = an.pcm_stats(files)
    r = res[[tr.name for _, tr in library].index("flac_padded")]
    assert r.error is None and r.padded and not r.clipped and (r.bits, r.effective_bits) == (24, 16) and "padded" in r.verdicts
    assert all(abs(ch.dc_offset) < 1.0 and 0.0 < ch.peak <= 1.0 for ch in r.channels) and r.channels[0].dc_offset == r.channels[0].sum / r.frames / 2 ** 31


def test_options_reach_the_kernels(an, library):
    files = [p for p, tr in library if tr.name in ("wav_s16_2", "flac_gap")]
    trs = [tr for _, tr in library if tr.name in ("wav_s16_2", "flac_gap")]
    for opts in ((1, 1), (6, 2001)):
        raw = an.pcm_stats_raw(files, *opts)
        for k, tr in enumerate(trs):
            r = _capi.PcmStatsRecord.from_buffer_copy(raw[REC * k:REC * k + REC])
            assert not pc.differences(pc.got(r), pc.want_track(tr, *opts)), (tr.name, opts)
    assert not _capi.PcmStatsRecord.from_buffer_copy(an.pcm_stats_raw(files, 6, 2001)[REC:2 * REC]).flags & _capi.STATS_DROPOUT
    with pytest.raises(rgmod.ReplayGainError) as e:
        an.pcm_stats(files, 0, 64)
    assert e.value.code == -1


def test_an_mp3_file_matches_the_host_twin_on_the_device_decoders_pcm(an):
    f = GOLD / "mp3" / "v1_44k_ms_mixed.mp3"
    pcm, info = an.decode_mp3_device(f.read_bytes())
    tr = rgmod.PcmTrack([np.ascontiguousarray(ch) for ch in pcm], int(info.sample_rate))
    arena, descs = rgmod.pack_tracks([tr])
    want = rgmod.pcm_stats_arena(None, 0, list(descs)[:1], None, arena)[0]
    got = _capi.PcmStatsRecord.from_buffer_copy(an.pcm_stats_raw([f]))
    assert not pc.differences(pc.got(got), pc.got(want)) and bytes(got) == bytes(want)
    assert (got.format, got.bits, got.channels, got.frames) == (_capi.FMT_F32_PLANAR, 0, pcm.shape[0], pcm.shape[1]) and got.flags & _capi.STATS_COMPLETE


def test_failing_files_fail_alone(an, tmp_path, library):
    rng = np.random.default_rng(52)
    nine = _write(tmp_path, "nine.wav", wav_bytes([rng.integers(-100, 100, 500) for _ in range(9)], 48000, "s16"))
    missing = tmp_path / "missing.flac"
    good = [library[1], library[9], library[4]]
    files = [good[0][0], missing, good[1][0], nine, good[2][0]]
    an.set_decoder_command("false {}")  # a decoder command is set and must not be run
    try:
        res = an.pcm_stats(files)
        raw = an.pcm_stats_raw(files)
    finally:
        an.set_decoder_command(None)
    _check([_capi.PcmStatsRecord.from_buffer_copy(raw[REC * k:REC * k + REC]) for k in (0, 2, 4)], good)
    for k, code, text in ((1, RG_ERR_IO, "Failed to open"), (3, RG_ERR_FORMAT, "9 channels")):
        r = res[k]
        assert r.error is not None and r.error.code == code and text in str(r.error) and str(files[k]) in str(r.error), (k, str(r.error))
        assert (r.frames, r.flags, r.channels, r.verdicts) == (0, 0, [], ["ok"])
        rec = _capi.PcmStatsRecord.from_buffer_copy(raw[REC * k:REC * k + REC])
        assert rec.status == code and raw[REC * k + 4:REC * k + REC] == bytes(REC - 4)  # zero apart from `status`
    assert an.pcm_stats([]) == []
