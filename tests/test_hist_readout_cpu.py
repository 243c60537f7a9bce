"""The histogram read-out on the host, over the constructed histograms of hist_cases.py: the library's rg_hist_loudness, the
oracle's and a plain Python scan agree exactly, and so do the gain and the rounded gain steps at every bin.  This keeps
the reference that test_gpu_hist_readout.py holds the kernels to honest without a GPU."""
import math
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent))
import hist_cases as hc  # noqa: E402


def test_threshold_quirk_is_what_the_cases_assume(oracle):
    """ceil(total * (1.0 - 0.95)) is total / 20 + 1 for every multiple of 20 below 2000, ceil(total / 20) for every other
    total there; the oracle's threshold is the same number."""
    L = oracle.lib()
    for total in range(1, 2000):
        want = total // 20 + 1 if total % 20 == 0 else (total + 19) // 20
        assert hc.threshold(total) == want == L.rgo_percentile_threshold(total), total
    for total in (3 * hc.U32_MAX, 3 * hc.U32_MAX + 2_000_000_000, hc.BINS * hc.U32_MAX):
        assert hc.threshold(total) == L.rgo_percentile_threshold(total)


def test_read_outs_agree_over_the_whole_family(capi, oracle):
    n = 0
    for cid, h in hc.family():
        want = hc.scan_loudness(h)
        assert oracle.hist_loudness(h) == want, cid
        assert capi.rg_hist_loudness(h.ctypes.data) == want, cid
        n += 1
    assert n >= hc.BINS + 400


def test_constructed_cases_stop_where_they_were_built_to(oracle):
    """The two-spike and the total cases carry the bin the scan must stop at: the crossing really is on the edge it names,
    and at every multiple of 20 the quirk really changes the answer."""
    for cid, h, stop in list(hc.two_spikes()) + list(hc.totals()):
        assert oracle.hist_loudness(h) == (stop - hc.OFFSET) / 100, cid
    changed = [cid for cid, h, stop in hc.totals() if cid.endswith("-paper") and h[stop] != (hc.total_of(h) + 19) // 20]
    assert changed == [f"total{t}-paper" for t in hc.quirk_totals() if t % 20 == 0]
    for (_, h), top in zip(hc.large(), (hc.BINS - hc.CHUNK, 2 * hc.WAVE_BINS - 1, 2)):
        assert hc.total_of(h) > 1 << 32 and hc.scan_loudness(h) == (top - hc.OFFSET) / 100


def test_gain_and_steps_at_every_bin(capi, oracle):
    """PINK_REF - loudness and round(gain / 1.5) at all 12 000 bins, the half-integer ties of (64.82 - L) / 1.5 among them:
    away from zero where the f64 quotient is an exact half, to the nearer side where it is not."""
    L = oracle.lib()
    ties = set(hc.tie_bins())
    assert len(ties) == 80 and 7 in ties and 8407 in ties
    exact_halves = 0
    for b in range(hc.BINS):
        loud = (b - hc.OFFSET) / 100
        gain = L.rgo_gain_from_loudness(loud)
        assert capi.rg_gain_from_loudness(loud) == gain == 64.82 - loud
        steps = L.rgo_gain_steps(gain)
        assert capi.rg_gain_steps(gain) == steps == capi.rg_db_to_steps(gain), b
        q = gain / 1.5
        if b in ties:
            assert abs(abs(q - int(q)) - 0.5) < 1e-9, b
            exact_halves += q - int(q) in (0.5, -0.5)
        whole = math.floor(abs(q))  # half away from zero on the f64 quotient (abs(q) - whole is exact)
        want = (whole + (abs(q) - whole >= 0.5)) * (1 if q >= 0 else -1)
        assert steps == want, b
    assert exact_halves > 0


def test_pack_sets_fold_like_the_host_restatement():
    """hist_cases.fold (u64 sums cut to 32 bits) is album.fold_gathered, and every set with more than one pack has a bin
    that wraps, one that wraps to exactly 0, a pack whose peak is 0.0 and its largest peak where its id says."""
    from mp3rgain_amd import album

    seen = set()
    for cid, packs in hc.pack_sets():
        world = packs.shape[0]
        seen.add(world)
        hist, peak, total = hc.fold(packs)
        fh, fp = album.fold_gathered(packs.reshape(-1), world)
        assert np.array_equal(fh, hist) and fp == peak and total == int(hist.sum(dtype=np.uint64)), cid
        peaks = packs[:, hc.BINS:].copy().view(np.float64).reshape(world)
        at = {"first": 0, "middle": world // 2, "last": world - 1}[cid.rsplit("-", 1)[1]]
        assert int(np.argmax(peaks)) == at and peak == peaks[at] and np.count_nonzero(peaks == peak) == 1, cid
        if world > 1:
            wide = packs[:, :hc.BINS].astype(np.uint64).sum(axis=0)
            assert np.count_nonzero(wide > hc.U32_MAX) >= 3 and hist[47] == 0 and hist[11000] == 1, cid
            assert 0.0 in peaks and 0 < at + 1 <= world, cid
            # the wrap decides the answer: read out of the unwrapped sums the scan would stop at bin 11000
            assert hc.scan_loudness(hist) < (11000 - hc.OFFSET) / 100, cid
    assert seen == set(hc.WORLDS)
