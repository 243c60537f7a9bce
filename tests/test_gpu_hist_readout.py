"""The histogram read-out and the album folds on the device, on histograms and tracks built to put the 95th-percentile
crossing where real audio never puts it (hist_cases.py): the edges of an owner thread's 48-bin chunk and of a wave, bins 0
and 11999, the threshold's rounding quirk at totals that are multiples of 20, totals above 2^32, bins that wrap in a fold,
and windows dropped above bin 11999 and below bin 0.

Injected histograms go in through rg_album_reduce_gathered, which overwrites the slot's album histogram with the fold of
`world` packs from a caller's buffer, and come out through rg_album_finish (rg_album_result_kernel).  The track route
(rg_track_result_kernel, the finisher of the transient-moment kernels, rg_album_results_kernel on strided packs) gets tracks
whose window counts are chosen around the quirk, and amplitude ramps that walk off either end of the histogram."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import hist_cases as hc  # noqa: E402
from wavutil import wav_bytes  # noqa: E402

pytestmark = pytest.mark.gpu

DB_TOL = 0.1  # north_star tolerance, for the one arm of the forced-variant rule that is not exact


# ======================================== injected histograms =========================================================
@pytest.fixture()
def inject(_ctx, oracle):
    """-> run(packs uint32[world][12002]) -> (rg_album_result, folded bins as the device holds them).  One tiny album batch is
    enqueued per use of the fixture: it makes a slot current and marks its album ready; every run then overwrites that
    slot's album histogram and peak."""
    import torch

    from mp3rgain_amd import _capi

    an = _ctx
    an.set_kernel(0)
    for key in (1, 2, 4):
        an.set_tuning(key, 0)
    frames = 1000
    buf = torch.empty(2 * frames + 4, dtype=torch.float32, device="cuda:0")
    descs = (_capi.TrackDesc * 1)()
    for c in range(2):
        an.synth_fill_device(buf.data_ptr() + 4 * c * frames, 0x5EEDA000, c, 8000, 0, frames)
    descs[0].offset_bytes, descs[0].frames, descs[0].sample_rate, descs[0].channels = 0, frames, 8000, 2
    descs[0].format = _capi.FMT_F32_PLANAR
    dev = torch.empty(max(hc.WORLDS) * hc.PACK_WORDS, dtype=torch.int32, device="cuda:0")
    an.set_stream(torch.cuda.current_stream().cuda_stream)
    an.enqueue_device(descs, 1, buf.data_ptr(), buf.numel() * 4, album=True)

    def run(packs):
        packs = np.ascontiguousarray(packs, dtype=np.uint32).reshape(-1, hc.PACK_WORDS)
        world = packs.shape[0]
        dev[:world * hc.PACK_WORDS].copy_(torch.from_numpy(packs.reshape(-1).view(np.int32)))
        an.album_reduce_gathered(dev.data_ptr(), world)
        return an.album_finish(want_hist=True)

    try:
        yield run
    finally:
        an.set_stream(None)


def _check_album(alb, got_hist, hist, peak, oracle, cid):
    """Every field of the rg_album_result against the oracle's read-out of `hist`, the bins against `hist` itself.  windows
    carries the low 32 bits of the u64 total (include/mp3rgain_amd.h)."""
    L = oracle.lib()
    bad = np.flatnonzero(got_hist != hist)
    assert bad.size == 0, f"{cid}: bins {bad[:6]} are {got_hist[bad[:6]]}, not {hist[bad[:6]]}"
    loud = oracle.hist_loudness(hist)
    gain = L.rgo_gain_from_loudness(loud)
    assert alb.album_loudness_db == loud, f"{cid}: {alb.album_loudness_db} != {loud}"
    assert alb.album_gain_db == gain and alb.album_gain_steps == L.rgo_gain_steps(gain), cid
    assert alb.album_peak == peak, cid
    assert alb.windows == hc.total_of(hist) & hc.U32_MAX, cid


@pytest.mark.parametrize("wave", range(4))
def test_single_spike_in_every_bin(inject, oracle, wave):
    """One occupied bin, every bin in turn (the whole 12 000-bin sweep, a wave of owner threads per case): the read-out names
    that bin whatever its count, 1 or 0xFFFFFFFF."""
    p = hc.pack(np.zeros(hc.BINS, dtype=np.uint32), 0.0)  # reused: one bin set, then cleared
    for b in range(wave * hc.WAVE_BINS, min((wave + 1) * hc.WAVE_BINS, hc.BINS)):
        peak = 0.25 + b / 65536.0
        p[b] = hc.spike_count(b)
        p[hc.BINS:] = np.array([peak], dtype=np.float64).view(np.uint32)
        alb, got = inject(p)
        assert alb.album_loudness_db == (b - hc.OFFSET) / 100, f"spike-{b}"
        _check_album(alb, got, p[:hc.BINS], peak, oracle, f"spike-{b}")
        p[b] = 0


def test_constructed_histograms(inject, oracle):
    """Two spikes either side of chunk and wave edges with the count from the top one short of, at and one past the
    threshold; totals 1..41 and the multiples of 20 up to 400 split so that the threshold's quirk decides; uniform
    histograms; totals above 2^32; 250 random ones."""
    stops = {cid: stop for cid, _, stop in list(hc.two_spikes()) + list(hc.totals())}
    n = 0
    for cid, h in hc.constructed():
        peak = 0.5 + (n % 64) / 128.0
        alb, got = inject(hc.pack(h, peak))
        if cid in stops:
            assert alb.album_loudness_db == (stops[cid] - hc.OFFSET) / 100, cid
        assert alb.album_loudness_db == hc.scan_loudness(h), cid
        _check_album(alb, got, h, peak, oracle, cid)
        n += 1
    assert n > 400


def test_totals_above_two_to_the_32(inject, oracle):
    """The u64 total: threshold and scan use all of it, `windows` keeps its low 32 bits."""
    for (cid, h), top in zip(hc.large(), (hc.BINS - hc.CHUNK, 2 * hc.WAVE_BINS - 1, 2)):
        alb, got = inject(hc.pack(h, 0.75))
        assert hc.total_of(h) == 3 * hc.U32_MAX + (5 if "small-top" in cid else 0)
        assert alb.windows == hc.total_of(h) % (1 << 32) and hc.total_of(h) > 1 << 32
        assert alb.album_loudness_db == (top - hc.OFFSET) / 100, cid
        _check_album(alb, got, h, 0.75, oracle, cid)
    h = np.full(hc.BINS, hc.U32_MAX, dtype=np.uint32)
    alb, got = inject(hc.pack(h, 2.0))
    assert alb.windows == (hc.BINS * hc.U32_MAX) % (1 << 32)
    _check_album(alb, got, h, 2.0, oracle, "uniform-max")


def test_folds_of_many_packs(inject, oracle):
    """rg_album_reduce_gathered_kernel over 1, 2, 3, 8 and 64 packs: bins add modulo 2^32 (a bin that wraps to 1 where the
    unwrapped sum would take the crossing, one that wraps to exactly 0), the peak is the largest pack peak wherever it
    sits, a pack whose peak is 0.0 changes nothing, and the read-out is the oracle's of the folded bins."""
    from mp3rgain_amd import album

    n = 0
    for cid, packs in hc.pack_sets():
        hist, peak, _ = hc.fold(packs)
        fh, fp = album.fold_gathered(packs.reshape(-1), packs.shape[0])
        assert np.array_equal(fh, hist) and fp == peak
        alb, got = inject(packs)
        _check_album(alb, got, hist, peak, oracle, cid)
        n += 1
    assert n == 1 + 2 + 3 * 3
    # a fold is a function of its packs alone: a constructed histogram right after a 64-pack fold
    h = np.zeros(hc.BINS, dtype=np.uint32)
    h[hc.WAVE_BINS - 1], h[hc.WAVE_BINS] = 38, 2
    alb, got = inject(hc.pack(h, 0.125))
    _check_album(alb, got, h, 0.125, oracle, "after-world64")
    assert alb.album_loudness_db == (hc.WAVE_BINS - 1 - hc.OFFSET) / 100  # total 40: threshold 3, not 2


# ======================================== the track route ==============================================================
QUIRK_RATE = 8000
QUIRK_WINDOW = QUIRK_RATE // 20
QUIRK_TOTALS = (19, 20, 21, 40, 100)


def quirk_track(total, seed):
    """`total` windows of uniform noise at 8 kHz, stereo: the last ceil(total / 20) of them 30 dB louder than the rest.  The
    loud windows are as many as the 95th percentile needs on paper, so the read-out is a loud window's bin -- except at a
    multiple of 20, where the f64 threshold asks for one window more and the read-out falls to the quiet ones.  (One loud
    window alone cannot tell the quirk at 21, 40 or 100 windows: the threshold is 2 or more there with or without it.)"""
    rng = np.random.default_rng(seed)
    amp = np.full(total, 0.01)
    amp[total - (total + 19) // 20:] = 0.01 * 10.0 ** (30.0 / 20.0)
    env = np.repeat(amp, QUIRK_WINDOW)
    return [(rng.uniform(-1.0, 1.0, env.size) * env).astype(np.float32) for _ in range(2)]


@pytest.fixture(scope="module")
def quirk_tracks(oracle):
    """-> [(total, channels, oracle result, oracle histogram)], preconditions asserted on the oracle alone."""
    out = []
    for k, total in enumerate(QUIRK_TOTALS):
        ch = quirk_track(total, 0x51A0 + k)
        want, wh = oracle.analyze_pcm(ch[0], ch[1], QUIRK_RATE)
        bins = np.flatnonzero(wh)
        gap = int(np.argmax(np.diff(bins)))  # the 30 dB between the quiet and the loud windows
        loud = bins[gap + 1:]
        assert int(wh.sum()) == total and bins[gap + 1] - bins[gap] > 2000
        assert int(wh[loud].sum()) == (total + 19) // 20
        is_loud = want["loudness_db"] * 100 + hc.OFFSET >= loud[0] - 0.5
        assert is_loud == (total % 20 != 0), f"{total} windows: read-out {want['loudness_db']}, loud bins {loud}"
        out.append((total, ch, want, wh))
    return out


def test_quirk_totals_as_tracks(analyzer, oracle, quirk_tracks):
    """rg_track_result_kernel / the finishers of every kernel variant: histogram, loudness and gain steps are the oracle's."""
    import mp3rgain_amd as rg

    got, h = analyzer.analyze_tracks([rg.PcmTrack(ch, QUIRK_RATE) for _, ch, _, _ in quirk_tracks], return_histograms=True)
    for g, hh, (total, _, want, wh) in zip(got, h, quirk_tracks):
        assert np.array_equal(hh, wh), f"{total} windows: bins {np.flatnonzero(hh != wh)[:6]}"
        assert g.loudness_db == want["loudness_db"] and g.gain_db == want["gain_db"], total
        assert g.gain_steps() == want["gain_steps"] and g.peak == want["peak"] and g.windows == total, total


def test_quirk_totals_as_one_album(analyzer, oracle, quirk_tracks):
    """The same tracks as one album of 200 windows, 11 of them loud: threshold 11 (200 / 20 + 1), so the read-out is the
    lowest loud bin; rg_album_merge_kernel + rg_album_result_kernel."""
    import mp3rgain_amd as rg

    aw, awh = oracle.album_from_hists([wh for _, _, _, wh in quirk_tracks], [w["peak"] for _, _, w, _ in quirk_tracks])
    assert int(awh.sum()) == 200 and hc.threshold(200) == 11
    res, h = analyzer.analyze_album([rg.PcmTrack(ch, QUIRK_RATE) for _, ch, _, _ in quirk_tracks], return_histogram=True)
    assert np.array_equal(h, awh)
    assert res.album_loudness_db == aw["album_loudness_db"] and res.album_gain_db == aw["album_gain_db"]
    assert res.album_gain_steps() == oracle.lib().rgo_gain_steps(aw["album_gain_db"]) and res.album_peak == aw["album_peak"]
    for g, (total, _, want, _) in zip(res.tracks, quirk_tracks):
        assert g.loudness_db == want["loudness_db"] and g.gain_steps() == want["gain_steps"] and g.windows == total


def test_quirk_totals_as_three_albums_of_files(analyzer, oracle, quirk_tracks, tmp_path):
    """The tracks as WAV files, three albums in one call (rg_album_fold_kernel, rg_album_results_kernel on strided packs):
    20 windows alone; 19 + 21 = 40 windows with 3 loud (threshold 3: a loud bin, the lowest); 40 + 100 = 140 windows with 7
    loud (threshold 8: a quiet bin).  On paper the thresholds would be 1, 2 and 7."""
    by_total = {total: (ch, want, wh) for total, ch, want, wh in quirk_tracks}
    files = {}
    for total, (ch, _, _) in by_total.items():
        files[total] = tmp_path / f"quirk{total}.wav"
        files[total].write_bytes(wav_bytes(ch, QUIRK_RATE, "f32"))
    albums = [(20,), (19, 21), (40, 100)]
    assert [hc.threshold(sum(a)) for a in albums] == [2, 3, 8]
    got = analyzer.analyze_albums_files([[files[t] for t in a] for a in albums])
    for a, g in zip(albums, got):
        aw, awh = oracle.album_from_hists([by_total[t][2] for t in a], [by_total[t][1]["peak"] for t in a])
        assert not isinstance(g, Exception), g
        assert g.album_loudness_db == aw["album_loudness_db"] == hc.scan_loudness(awh), a
        assert g.album_gain_db == aw["album_gain_db"] and g.album_peak == aw["album_peak"], a
        assert g.album_gain_steps() == oracle.lib().rgo_gain_steps(aw["album_gain_db"]), a
        for t, r in zip(a, g.tracks):
            want = by_total[t][1]
            assert r.loudness_db == want["loudness_db"] and r.gain_steps() == want["gain_steps"] and r.windows == t, t


# ======================================== the ends of the histogram ===================================================
RAMP_WINDOWS = 60
RAMP_RATES = (8000, 44100, 96000)
RAMPS = [("top", "f32"), ("bottom", "f32"), ("bottom", "s32")]


def ramp_track(end, kind, rate, seed):
    """60 windows of uniform noise, stereo, the amplitude moving 0.5 dB per window: +15 ... +44.5 dB relative to full scale
    (top; float only) or -75 ... -104.5 dB (bottom), so that the later windows fall off the histogram."""
    rng = np.random.default_rng(seed)
    db = (15.0 + 0.5 * np.arange(RAMP_WINDOWS)) if end == "top" else (-75.0 - 0.5 * np.arange(RAMP_WINDOWS))
    env = np.repeat(10.0 ** (db / 20.0), rate // 20)
    chans = [rng.uniform(-1.0, 1.0, env.size) * env for _ in range(2)]
    if kind == "f32":
        return [c.astype(np.float32) for c in chans]
    return [np.round(c * 2147483648.0).astype(np.int32) for c in chans]


@pytest.fixture(scope="module")
def ramps(oracle):
    """-> [(id, rate, channels, oracle result, oracle histogram)]; each ramp keeps at least 5 windows, drops at least 5 and
    has a kept bin within 100 of its end of the histogram (asserted on the oracle alone)."""
    out = []
    for k, (end, kind) in enumerate(RAMPS):
        for rate in RAMP_RATES:
            ch = ramp_track(end, kind, rate, 0x4A30 + 16 * k + RAMP_RATES.index(rate))
            want, wh = oracle.analyze_pcm(ch[0], ch[1], rate)
            kept, bins = int(wh.sum()), np.flatnonzero(wh)
            cid = f"{end}-{kind}-{rate}"
            assert 5 <= kept <= RAMP_WINDOWS - 5, f"{cid}: {kept} windows kept"
            assert (bins[-1] >= hc.BINS - 100) if end == "top" else (bins[0] < 100), f"{cid}: bins {bins[0]}..{bins[-1]}"
            out.append((cid, rate, ch, want, wh))
    return out


def test_windows_dropped_off_either_end_auto_mode(_ctx, oracle, ramps):
    """The library's default routing: every bin the oracle's at all three rates, the dropped windows dropped."""
    import mp3rgain_amd as rg

    an = _ctx
    an.set_kernel(0)
    for key in (1, 2, 4):
        an.set_tuning(key, 0)
    got, h = an.analyze_tracks([rg.PcmTrack(ch, rate) for _, rate, ch, _, _ in ramps], return_histograms=True)
    for g, hh, (cid, rate, _, want, wh) in zip(got, h, ramps):
        assert np.array_equal(hh, wh), f"{cid}: bins {np.flatnonzero(hh != wh)[:6]}"
        assert g.loudness_db == want["loudness_db"] and g.gain_steps() == want["gain_steps"] and g.peak == want["peak"], cid
        assert g.windows == int(wh.sum()) and not g.flags & 2, cid


def test_windows_dropped_off_either_end_forced_variants(analyzer, oracle, ramps):
    """Every kernel variant, with the rule of test_gpu_parity._differential: exact at 48 kHz and below, and exact above
    unless the forced transient-moment kernels flag the track as imprecise."""
    import mp3rgain_amd as rg

    got, h = analyzer.analyze_tracks([rg.PcmTrack(ch, rate) for _, rate, ch, _, _ in ramps], return_histograms=True)
    for g, hh, (cid, rate, _, want, wh) in zip(got, h, ramps):
        assert g.peak == want["peak"], cid
        assert abs(g.loudness_db - want["loudness_db"]) <= DB_TOL, cid
        if rate <= 48000 or not (g.flags & 2):
            assert np.array_equal(hh, wh), f"{cid}: bins {np.flatnonzero(hh != wh)[:6]}"
            assert g.loudness_db == want["loudness_db"] and g.gain_steps() == want["gain_steps"], cid
            assert g.windows == int(wh.sum()), cid
        else:
            assert int(hh.sum()) in (int(wh.sum()) - 1, int(wh.sum()), int(wh.sum()) + 1), cid
