"""EBU R 128 / ReplayGain 2.0 on the GPU (mp3rgain_amd/csrc/rg_r128.hip) against the float64 checker tests/r128ref.py:
EBU Tech 3341 conformance, every gating block of the parity signals (tests/r128cases.py) within a tolerance MEASURED on the
checker itself (tests/golden/r128_measured.json, tools/r128_refcheck.py: 100 x the float64 checker's worst relative block
error against np.longdouble), results, albums, edge rules, files, and the ReplayGain 1.0 path left undisturbed."""
import math
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import r128cases  # noqa: E402
import r128ref  # noqa: E402
from wavutil import wav_bytes  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = Path(__file__).parent / "golden"
TOL = 100.0 * r128cases.load_measured()["worst_relative_block_error"]
# true peak, f32 kernel: 14 roundings of 2^-24 (13 fused multiply-adds + the table's f32 rounding) x 2.31 (largest per-phase sum
# of |h|, F = 2) x max|x| <= true peak
TP_TOL = 2e-6
RG1_RATES = (96000, 88200, 64000, 48000, 44100, 32000, 24000, 22050, 16000, 12000, 11025, 8000)


@pytest.fixture()
def an(_ctx):
    _ctx.set_kernel(0)
    for key in (1, 2, 4, 10, 13):
        _ctx.set_tuning(key, 0)
    _ctx.set_tuning(14, 1)
    _ctx.set_tuning_r128(1, 0)
    _ctx.set_decoder_command(None)
    yield _ctx
    _ctx.set_tuning_r128(1, 0)
    _ctx.set_tuning(13, 0)


def _track(chans, rate):
    import mp3rgain_amd as rg

    return rg.PcmTrack(chans, rate)


def _as(chans, fmt):
    if fmt == "f32":
        return [np.asarray(c, dtype=np.float32) for c in chans]
    return [np.clip(np.round(np.asarray(c) * 32767.0), -32768, 32767).astype(np.int16) for c in chans]


# ---- conformance: EBU Tech 3341 -----------------------------------------------------------------------------------------
def test_tech3341_loudness(an):
    cases, tracks = [], []
    for rate in (44100, 48000):
        for fmt in ("f32", "s16"):
            for name, segments, want in r128ref.TECH3341_LOUDNESS:
                cases.append((name, rate, fmt, want))
                tracks.append(_track(_as(r128ref.sine_segments(rate, segments), fmt), rate))
    x = np.sin(2.0 * np.pi * 997.0 * np.arange(20 * 48000) / 48000.0)
    cases.append(("997Hz-one-channel", 48000, "f32", -3.01))
    tracks.append(_track(_as([x, np.zeros_like(x)], "f32"), 48000))
    res = an.analyze_tracks_r128(tracks)
    bad = []
    for (name, rate, fmt, want), r in zip(cases, res):
        bar = 0.05 if name.startswith("997") else 0.1
        print(f"{name} {rate} {fmt}: {r.loudness_lufs:.4f} LUFS (expected {want} +- {bar}), gain {r.gain_db:+.4f} dB")
        if not abs(r.loudness_lufs - want) <= bar or not abs(r.gain_db - (-18.0 - r.loudness_lufs)) <= 1e-12:
            bad.append((name, rate, fmt, r.loudness_lufs))
    assert not bad, bad


def test_tech3341_truepeak(an):
    cases, tracks = [], []
    for rate in (44100, 48000, 96000):
        for fmt in ("f32", "s16"):
            for name, div, phase, amp in r128ref.TECH3341_TRUEPEAK:
                cases.append((name, rate, fmt, amp))
                tracks.append(_track(_as([r128ref.truepeak_signal(rate, div, phase, amp)], fmt), rate))
    res = an.analyze_tracks_r128(tracks, true_peak=True)
    bad = []
    for (name, rate, fmt, amp), r in zip(cases, res):
        got, want = 20.0 * math.log10(r.true_peak), 20.0 * math.log10(amp)
        print(f"{name} {rate} {fmt}: {got:.3f} dBTP (expected {want:.3f} +0.2 / -0.4), sample peak {r.sample_peak:.4f}")
        if not (-0.4 <= got - want <= 0.2) or r.true_peak < r.sample_peak:
            bad.append((name, rate, fmt, got, want))
    assert not bad, bad


# ---- parity per block -----------------------------------------------------------------------------------------------------
_CACHE = {}


def _parity_set():
    if not _CACHE:
        cases = r128cases.parity_cases()
        chans = [r128cases.make(kind, rate, frames, nch, fmt, seed) for _, kind, rate, frames, nch, fmt, seed in cases]
        refs = [r128ref.analyze(ch, c[2], True) for ch, c in zip(chans, cases)]
        _CACHE["set"] = (cases, chans, refs)
    return _CACHE["set"]


def test_parity_precondition_no_block_near_a_gate():
    """On the reference alone: no block within relative 10 x tol of either threshold, so a block cannot change sides of a
    gate within the tolerance and the result comparison below is meaningful for every case (none is left out)."""
    cases, _, refs = _parity_set()
    for c, ref in zip(cases, refs):
        z = ref["z"]
        _, _, thr = r128ref.gate(z)
        for gate in (r128ref.ABS_GATE, thr):
            if len(z):
                d = float(np.min(np.abs(z - gate) / gate))
                assert d > 10.0 * TOL, (c[0], gate, d)


def _check_against_ref(cid, r, z, ref, rate):
    print(f"{cid}: {r.loudness_lufs:.6f} LUFS (ref {ref['loudness_lufs']:.6f}), blocks {r.blocks} gated {r.blocks_gated}", end="")
    zr = ref["z"]
    assert len(z) == len(zr) == r.blocks == ref["blocks"], cid
    if len(zr):
        above = zr >= r128ref.ABS_GATE
        err_above = float(np.max(np.abs(z[above] - zr[above]) / zr[above])) if np.any(above) else 0.0
        err_below = float(np.max(np.abs(z[~above] - zr[~above]))) / r128ref.ABS_GATE if np.any(~above) else 0.0
        print(f", worst block error {err_above:.2e} relative above the gate, {err_below:.2e} of the gate below it (bar {TOL:.2e})", end="")
        assert err_above <= TOL and err_below <= TOL, (cid, err_above, err_below)
    print()
    assert r.blocks_gated == ref["blocks_gated"], cid
    if ref["loudness_lufs"] == -math.inf:
        assert r.loudness_lufs == -math.inf and r.gain_db == 0.0, cid
    else:
        assert abs(r.loudness_lufs - ref["loudness_lufs"]) <= 4.343 * TOL + 1e-12, cid
        assert abs(r.gain_db - (-18.0 - r.loudness_lufs)) <= 1e-12, cid
    assert r.sample_peak == ref["sample_peak"], cid
    assert abs(r.true_peak - ref["true_peak"]) <= TP_TOL * ref["true_peak"], (cid, r.true_peak, ref["true_peak"])
    assert r.sample_rate == rate and r.flags == 0, cid


@pytest.mark.parametrize("S", [0, 1, 2, 5, 7, 64], ids=lambda s: f"S{s}")
def test_parity_per_block(an, S):
    """Every parity signal in ONE batch: tracks of eight rates and three formats share the launches; forced small and large
    hops-per-lane put lane boundaries at many offsets."""
    cases, chans, refs = _parity_set()
    an.set_tuning_r128(1, S)
    res, blocks = an.analyze_tracks_r128([_track(ch, c[2]) for ch, c in zip(chans, cases)], true_peak=True, return_blocks=True)
    for c, r, z, ref in zip(cases, res, blocks, refs):
        _check_against_ref(c[0], r, z, ref, c[2])


def test_sample_peak_equals_the_rg1_path(an):
    cases, chans, _ = _parity_set()
    pick = [i for i, c in enumerate(cases) if c[2] in RG1_RATES and c[3] > 0]
    tracks = [_track(chans[i], cases[i][2]) for i in pick]
    rg1 = an.analyze_tracks(tracks)
    r128 = an.analyze_tracks_r128(tracks)
    assert [r.sample_peak for r in r128] == [r.peak for r in rg1]


def test_single_tracks_and_mono_stereo(an):
    """One track per call (other lane shapes than in the batch), and longer tracks that several lanes share at a large S."""
    cases, chans, refs = _parity_set()
    for i in (0, 3, 12, 23):
        res, blocks = an.analyze_tracks_r128([_track(chans[i], cases[i][2])], true_peak=True, return_blocks=True)
        _check_against_ref(cases[i][0], res[0], blocks[0], refs[i], cases[i][2])
    rate = 44100
    long = r128cases.make("music", rate, 100 * rate + 1234, 2, "f32", 77)
    tracks = [_track(long, rate)] * 4
    ref = r128ref.analyze(long, rate, True)
    for S in (0, 33):
        an.set_tuning_r128(1, S)
        res, blocks = an.analyze_tracks_r128(tracks, true_peak=True, return_blocks=True)
        _check_against_ref(f"long-music-S{S}", res[0], blocks[0], ref, rate)
        assert all(np.array_equal(b, blocks[0]) for b in blocks) and len({r.loudness_lufs for r in res}) == 1


# ---- album --------------------------------------------------------------------------------------------------------------
def _album_tracks():
    rate = 48000
    rng = np.random.default_rng(0xA1B)
    loud = [(0.25 * rng.standard_normal(6 * rate)).astype(np.float32) for _ in range(2)]
    mid = [(0.08 * rng.standard_normal(4 * rate + 100)).astype(np.float32) for _ in range(2)]
    # about 26 dB under the loud track: below the album's relative gate (-10 LU), well above its own and the absolute gate
    quiet = [(0.0125 * rng.standard_normal(5 * rate)).astype(np.float32) for _ in range(2)]
    return [(loud, rate), (mid, rate), (quiet, rate)]


def test_album_is_the_union_of_blocks(an):
    tr = _album_tracks()
    ref_tracks, ref_album = r128ref.analyze_album(tr, True)
    _, _, thr = r128ref.gate(ref_album["z"])
    zq = ref_tracks[2]["z"]
    assert np.all(zq < thr) and ref_tracks[2]["blocks_gated"] == ref_tracks[2]["blocks"]  # the quiet track: out of the album, whole in itself
    for gate in (r128ref.ABS_GATE, thr):
        assert float(np.min(np.abs(ref_album["z"] - gate) / gate)) > 10.0 * TOL
    got, blocks = an.analyze_album_r128([_track(ch, rate) for ch, rate in tr], true_peak=True, return_blocks=True)
    print(f"album {got.loudness_lufs:.6f} LUFS (ref {ref_album['loudness_lufs']:.6f}), tracks {[round(t.loudness_lufs, 3) for t in got.tracks]}")
    assert abs(got.loudness_lufs - ref_album["loudness_lufs"]) <= 4.343 * TOL + 1e-12
    assert (got.blocks, got.blocks_gated) == (ref_album["blocks"], ref_album["blocks_gated"])
    assert abs(got.gain_db - (-18.0 - got.loudness_lufs)) <= 1e-12
    assert got.sample_peak == max(t.sample_peak for t in got.tracks) == ref_album["sample_peak"]
    assert got.true_peak == max(t.true_peak for t in got.tracks)
    assert abs(got.true_peak - ref_album["true_peak"]) <= TP_TOL * ref_album["true_peak"]
    mean_of_tracks = float(np.mean([t.loudness_lufs for t in got.tracks]))
    assert abs(got.loudness_lufs - mean_of_tracks) > 1.0
    for t, z, ref in zip(got.tracks, blocks, ref_tracks):
        _check_against_ref("album-track", t, z, ref, 48000)
    # the same batch twice: identical bits
    again, blocks2 = an.analyze_album_r128([_track(ch, rate) for ch, rate in tr], true_peak=True, return_blocks=True)
    assert again == got and all(np.array_equal(a, b) for a, b in zip(blocks, blocks2))
    # without the true peak: NaN there, the rest unchanged
    plain = an.analyze_album_r128([_track(ch, rate) for ch, rate in tr])
    assert math.isnan(plain.true_peak) and all(math.isnan(t.true_peak) for t in plain.tracks)
    assert (plain.loudness_lufs, plain.sample_peak, plain.peak) == (got.loudness_lufs, got.sample_peak, got.sample_peak)


def test_album_in_several_groups_equals_one_group(an, tmp_path):
    tr = _album_tracks()
    files = []
    for i, (ch, rate) in enumerate(tr):
        f = tmp_path / f"t{i}.wav"
        f.write_bytes(wav_bytes(ch, rate, "f32"))
        files.append(f)
    one = an.analyze_album_files_r128(files, true_peak=True)
    an.set_tuning(13, 1)  # groups of one file each
    many = an.analyze_album_files_r128(files, true_peak=True)
    an.set_tuning(13, 0)
    assert one == many
    pcm = an.analyze_album_r128([_track(ch, rate) for ch, rate in tr], true_peak=True)
    assert (one.loudness_lufs, one.blocks, one.blocks_gated, one.sample_peak, one.true_peak) == \
        (pcm.loudness_lufs, pcm.blocks, pcm.blocks_gated, pcm.sample_peak, pcm.true_peak)


# ---- edge rules ---------------------------------------------------------------------------------------------------------
def test_edge_rules(an):
    rate = 44100
    rng = np.random.default_rng(5)
    good = [(0.1 * rng.standard_normal(3 * rate)).astype(np.float32) for _ in range(2)]
    silence = [np.zeros(2 * rate, dtype=np.float32)] * 2
    short = [good[0][:int(0.3 * rate)].copy()]
    nan = [good[0].copy(), good[1].copy()]
    nan[1][rate + 17] = np.nan
    inf = [good[0].copy()]
    inf[0][5] = np.inf
    inf[0][2 * rate] = -np.inf
    tail_nan = [good[0].copy()]
    tail_nan[0][-3] = np.nan  # in the partial last hop, which no energy counts: the track is flagged all the same
    alone = an.analyze_tracks_r128([_track(good, rate)], true_peak=True)[0]
    res = an.analyze_tracks_r128([_track(c, rate) for c in (good, silence, short, nan, inf, tail_nan, good)], true_peak=True)
    assert res[0] == alone and res[6] == alone
    for r in res[1:3]:
        assert r.loudness_lufs == -math.inf and r.gain_db == 0.0 and r.flags == 0
    assert res[1].sample_peak == 0.0 and res[1].true_peak == 0.0 and res[2].blocks == 0
    assert res[2].sample_peak == float(np.max(np.abs(short[0])))
    for r, ch in zip(res[3:6], (nan, inf, tail_nan)):
        assert r.flags == 1 and math.isnan(r.loudness_lufs) and math.isnan(r.gain_db)
        assert r.sample_peak == r128ref.sample_peak(ch) and math.isfinite(r.true_peak) and r.true_peak > 0.0
    album = an.analyze_album_r128([_track(good, rate), _track(nan, rate)], true_peak=True)
    assert math.isnan(album.loudness_lufs) and math.isnan(album.gain_db) and album.tracks[0] == alone
    assert album.sample_peak == max(t.sample_peak for t in album.tracks)
    assert an.analyze_tracks_r128([]) == []
    import mp3rgain_amd as rg

    with pytest.raises(rg.ReplayGainError, match="Unsupported sample rate: 7999 Hz. Supported rates: 8000 to 384000"):
        an.analyze_tracks_r128([_track(good, 7999)])


# ---- files ----------------------------------------------------------------------------------------------------------------
def _flac_planar(pcm, bps):
    if bps <= 16:
        return [(c << (16 - bps)).astype(np.int16) for c in pcm]
    return [(c.astype(np.int64) << (32 - bps)).astype(np.int32) for c in pcm]


def _golden_files():
    from mp3rgain_amd import flacdec, mp3dec

    out = []
    for f in sorted((GOLDEN / "flac").glob("*.flac")):
        try:
            rate, bps, pcm, _ = flacdec.decode(f.read_bytes())
        except flacdec.FlacError:
            continue
        out.append((f, _flac_planar(list(pcm), bps), rate))
    for f in sorted((GOLDEN / "mp3").glob("*.mp3")):
        pcm, info = mp3dec.decode(f.read_bytes())
        out.append((f, [pcm[c] for c in range(int(info.channels))], int(info.sample_rate)))
    return out


def test_files_against_the_checker_on_the_host_decoders_pcm(an, tmp_path):
    import mp3rgain_amd as rg

    gold = _golden_files()
    assert any(f.name == "s16_stereo_192k.flac" for f, _, _ in gold) and len(gold) > 30
    wch = r128cases.make("music", 44100, 3 * 44100 + 5, 2, "s16", 9)
    w = tmp_path / "w.wav"
    w.write_bytes(wav_bytes(wch, 44100, "s16"))
    gold.append((w, wch, 44100))
    files = [g[0] for g in gold]
    res = an.analyze_track_files_r128(files, true_peak=True)
    for (f, ch, rate), r in zip(gold, res):
        assert not isinstance(r, Exception), (f.name, r)
        ref = r128ref.analyze(ch, rate, True)
        print(f"{f.name}: {r.loudness_lufs:.4f} LUFS (ref {ref['loudness_lufs']:.4f}) peak {r.sample_peak:.6f} true peak {r.true_peak:.6f}")
        assert (r.blocks, r.blocks_gated, r.sample_rate) == (ref["blocks"], ref["blocks_gated"], rate), f.name
        if ref["loudness_lufs"] == -math.inf:
            assert r.loudness_lufs == -math.inf, f.name
        else:
            assert abs(r.loudness_lufs - ref["loudness_lufs"]) <= 4.343 * TOL + 1e-12, f.name
        assert r.sample_peak == ref["sample_peak"], f.name
        assert abs(r.true_peak - ref["true_peak"]) <= TP_TOL * ref["true_peak"], f.name
    # the hi-res file: this path analyses it, the ReplayGain 1.0 route still refuses it with its old message
    hi = GOLDEN / "flac" / "s16_stereo_192k.flac"
    old = an.analyze_track_files([hi])[0]
    assert isinstance(old, rg.ReplayGainError) and "Unsupported sample rate: 192000 Hz. Supported rates: 96000, 88200" in str(old)
    # an album of the 44.1 kHz stereo files against the checker
    pick = [g for g in gold if g[2] == 44100 and len(g[1]) == 2][:6]
    album = an.analyze_album_files_r128([g[0] for g in pick], true_peak=True)
    _, ref_album = r128ref.analyze_album([(g[1], g[2]) for g in pick], True)
    assert abs(album.loudness_lufs - ref_album["loudness_lufs"]) <= 4.343 * TOL + 1e-12
    assert (album.blocks, album.blocks_gated, album.sample_peak) == (ref_album["blocks"], ref_album["blocks_gated"], ref_album["sample_peak"])
    assert [t.loudness_lufs for t in album.tracks] == [res[files.index(g[0])].loudness_lufs for g in pick]


def test_per_file_errors(an, tmp_path):
    import mp3rgain_amd as rg

    good = GOLDEN / "mp3" / "v1_44k_ms_mixed.mp3"
    junk = tmp_path / "junk.mp3"
    junk.write_bytes(b"ID3" + bytes(500))
    low = tmp_path / "low.wav"
    low.write_bytes(wav_bytes([np.zeros(8000, dtype=np.int16)], 7999, "s16"))
    missing = tmp_path / "missing.mp3"
    ref = an.analyze_track_files([good, missing, junk, low])
    res = an.analyze_track_files_r128([good, missing, junk, low, good], true_peak=True)
    assert res[0] == res[4] and not isinstance(res[0], Exception)
    for i in (1, 2):  # the loaders' own errors: the same texts and codes as on the ReplayGain 1.0 route
        assert isinstance(res[i], rg.ReplayGainError) and (res[i].code, str(res[i])) == (ref[i].code, str(ref[i]))
    assert res[1].code == -8 and str(res[1]).startswith("Failed to open")
    assert res[2].code == -9 and str(res[2]).startswith("Failed to probe format")
    assert res[3].code == -2 and str(res[3]) == "Unsupported sample rate: 7999 Hz. Supported rates: 8000 to 384000"
    with pytest.raises(rg.ReplayGainError, match="Failed to open") as ex:
        an.analyze_album_files_r128([good, missing, junk])
    assert ex.value.code == -8
    with pytest.raises(rg.ReplayGainError, match="Unsupported sample rate: 7999 Hz"):
        an.analyze_album_files_r128([good, low])
    assert an.analyze_album_files_r128([good], true_peak=True).tracks[0] == res[0]


# ---- nothing else moved ------------------------------------------------------------------------------------------------------
def test_rg1_results_unchanged_around_an_r128_call(an):
    cases, chans, _ = _parity_set()
    pick = [i for i, c in enumerate(cases) if c[2] in RG1_RATES and c[3] > 0][:10]
    tracks = [_track(chans[i], cases[i][2]) for i in pick]
    before, hist_before = an.analyze_tracks(tracks, return_histograms=True)
    an.analyze_tracks_r128(tracks, true_peak=True)
    an.analyze_album_r128(tracks[:3])
    after, hist_after = an.analyze_tracks(tracks, return_histograms=True)
    assert np.array_equal(hist_before, hist_after) and before == after
