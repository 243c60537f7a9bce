"""Constructed histograms for the percentile read-out and the album folds (shared by test_hist_readout_cpu.py and
test_gpu_hist_readout.py; not a test).

Real audio puts a few hundred windows into a narrow band of bins, so the read-out (LoudnessHistogram::get_loudness,
src/replaygain.rs:665-682) never meets a crossing on the edge of an owner thread's 48-bin chunk or of a wave, the
threshold's rounding quirk, a total above 2^32 or a wrapping bin.  These histograms put the crossing there on purpose.

The quirk: the threshold is ceil(total as f64 * (1.0 - 0.95)), and 1.0 - 0.95 is 0.050000000000000044 in f64, so a total
that is a multiple of 20 gives total / 20 + 1 (checked by test_hist_readout_cpu.py for every such total below 2000).
"""
import math

import numpy as np

BINS = 12000
OFFSET = 2000
CHUNK = 48          # bins per owner thread of the device read-out (RG_PCT_CHUNK)
WAVE_BINS = 64 * CHUNK
PACK_WORDS = BINS + 2
U32_MAX = 0xFFFFFFFF


def threshold(total: int) -> int:
    return math.ceil(float(total) * (1.0 - 0.95))


def scan_loudness(hist) -> float:
    """The reference's sequential scan in plain Python: u64 total, threshold, bins 11999 -> 0.  Only occupied bins are
    visited: an empty bin adds nothing, and the threshold of a histogram that is not empty is at least 1."""
    h = np.asarray(hist, dtype=np.uint32)
    occupied = np.flatnonzero(h).tolist()
    total = sum(int(h[i]) for i in occupied)
    if total == 0:
        return -20.0
    thr, count = threshold(total), 0
    for i in reversed(occupied):
        count += int(h[i])
        if count >= thr:
            return (i - OFFSET) / 100
    return -20.0


def total_of(hist) -> int:
    return int(np.asarray(hist, dtype=np.uint32).sum(dtype=np.uint64))


def _hist(entries) -> np.ndarray:
    h = np.zeros(BINS, dtype=np.uint32)
    for b, c in entries:
        h[b] = c
    return h


# ---- single spikes --------------------------------------------------------------------------------------------------
def tie_bins():
    """Bins whose gain (64.82 - L) / 1.5 is a half-integer on paper: L = 64.07 - 1.5 k, bin = 8407 - 150 k."""
    return [b for b in range(BINS) if (b - 8407) % 150 == 0]


def reduced_spike_bins(seed=20261017):
    """The cut-down sweep: both sides of every chunk edge, the ends, the gain-step ties and 500 random bins."""
    bins = {0, BINS - 1}
    for k in range(BINS // CHUNK + 1):
        bins.update(b for b in (CHUNK * k - 1, CHUNK * k, CHUNK * k + 1) if 0 <= b < BINS)
    bins.update(tie_bins())
    bins.update(int(b) for b in np.random.default_rng(seed).integers(0, BINS, 500))
    return sorted(bins)


def spike_count(b: int) -> int:
    """The count a single spike at bin b carries: mostly small, some totals that are multiples of 20, some at the u32 limit."""
    if b % 97 == 0:
        return U32_MAX
    return (1, 19, 20, 21, 400, 1 + (b * 7919) % 5000)[b % 6]


def single_spikes(bins=None):
    for b in (range(BINS) if bins is None else bins):
        yield f"spike-{b}", _hist([(b, spike_count(b))])


# ---- two spikes that place the crossing -----------------------------------------------------------------------------
def edge_pairs():
    pairs = [(0, 1), (BINS - 2, BINS - 1)]
    pairs += [(CHUNK * k - 1, CHUNK * k) for k in (1, 2, 63, 64, 65, 128, 192, 249)]
    return pairs


def two_spikes():
    """Lower spike at a, upper spike at b: the count from the top on reaching b is threshold - 1 (the scan goes on to a),
    threshold or threshold + 1 (it stops at b).  -> (id, hist, bin the scan stops at)"""
    for a, b in edge_pairs():
        for total in (37, 1000):
            thr = threshold(total)
            for d in (-1, 0, 1):
                upper = thr + d
                if upper <= 0 or upper > U32_MAX or total - upper > U32_MAX:
                    continue
                yield f"pair-{a}-{b}-total{total}-thr{d:+d}", _hist([(a, total - upper), (b, upper)]), (a if d < 0 else b)
    # a total above 2^32 needs more than two bins: the mass below a is spread over bins the scan never reaches
    for a, b in edge_pairs():
        if a < 3:
            continue
        total = 3 * U32_MAX + 2_000_000_000
        thr = threshold(total)
        for d in (-1, 0, 1):
            h = _hist([(b, thr + d), (a, 2_000_000_000 - (thr + d)), (0, U32_MAX), (1, U32_MAX), (2, U32_MAX)])
            assert total_of(h) == total
            yield f"pair-{a}-{b}-total{total}-thr{d:+d}", h, (a if d < 0 else b)


# ---- totals around the quirk ----------------------------------------------------------------------------------------
def quirk_totals():
    return list(range(1, 42)) + list(range(60, 401, 20))


def totals():
    """For every total two splits: the upper spike holds ceil(total / 20) windows, the paper threshold -- the scan stops there
    unless the total is a multiple of 20, where the f64 threshold is one more -- or it holds the f64 threshold itself.
    -> (id, hist, bin the scan stops at)"""
    for total in quirk_totals():
        a, b = 100 + total, 11000 - total
        paper, thr = (total + 19) // 20, threshold(total)
        yield f"total{total}-paper", _hist([(a, total - paper), (b, paper)]), (b if paper >= thr else a)
        if thr <= total:
            yield f"total{total}-f64", _hist([(a, total - thr), (b, thr)]), b


# ---- uniform and large ----------------------------------------------------------------------------------------------
def uniform():
    yield "uniform-1", np.ones(BINS, dtype=np.uint32)
    yield "uniform-max", np.full(BINS, U32_MAX, dtype=np.uint32)


def large():
    yield "large-3", _hist([(47, U32_MAX), (WAVE_BINS, U32_MAX), (BINS - CHUNK, U32_MAX)])
    yield "large-3-under-a-small-top", _hist([(CHUNK - 1, U32_MAX), (CHUNK, U32_MAX), (2 * WAVE_BINS - 1, U32_MAX), (BINS - 1, 5)])
    yield "large-3-low", _hist([(0, U32_MAX), (1, U32_MAX), (2, U32_MAX)])


# ---- random ---------------------------------------------------------------------------------------------------------
def random_hists(sparse=200, dense=50, seed=20261017):
    rng = np.random.default_rng(seed)
    for i in range(sparse):
        h = np.zeros(BINS, dtype=np.uint32)
        k = int(rng.integers(1, 41))
        where = rng.integers(0, BINS, k)
        if i % 3 == 0:  # clustered on chunk edges
            where = (where // CHUNK) * CHUNK + rng.choice([-1, 0, CHUNK - 1], k)
            where = np.clip(where, 0, BINS - 1)
        top = int(rng.choice([3, 50, 5000, U32_MAX]))
        h[where] = rng.integers(1, top, k, endpoint=True).astype(np.uint32)
        yield f"sparse-{i}", h
    for i in range(dense):
        top = int(rng.choice([1, 3, 1000, U32_MAX]))
        h = rng.integers(0, top, BINS, endpoint=True).astype(np.uint32)
        if i % 2:
            h[rng.random(BINS) < 0.5] = 0
        yield f"dense-{i}", h


def constructed():
    """Everything but the single-spike sweep, as (id, hist)."""
    for cid, h, _ in two_spikes():
        yield cid, h
    for cid, h, _ in totals():
        yield cid, h
    yield from uniform()
    yield from large()
    yield from random_hists()
    yield "empty", np.zeros(BINS, dtype=np.uint32)


def family(spike_bins=None):
    yield from single_spikes(spike_bins)
    yield from constructed()


# ---- packs for the folds --------------------------------------------------------------------------------------------
def pack(hist, peak: float) -> np.ndarray:
    p = np.zeros(PACK_WORDS, dtype=np.uint32)
    p[:BINS] = hist
    p[BINS:] = np.array([peak], dtype=np.float64).view(np.uint32)
    return p


def fold(packs):
    """`world` packs -> (hist with bins summed modulo 2^32, largest peak, u64 total of the folded bins)."""
    packs = np.asarray(packs, dtype=np.uint32).reshape(-1, PACK_WORDS)
    wide = packs[:, :BINS].astype(np.uint64).sum(axis=0)
    hist = (wide & np.uint64(U32_MAX)).astype(np.uint32)
    peaks = [float(p[BINS:].copy().view(np.float64)[0]) for p in packs]
    return hist, max(peaks), total_of(hist)


WORLDS = (1, 2, 3, 8, 64)


def pack_sets(seed=20261018):
    """-> (id, packs uint32[world][12002]).  Every set with more than one pack has bins that sum past 2^32 (one to exactly
    2^32, i.e. 0; one high bin that would take the crossing if the sum did not wrap), a pack whose peak is 0.0, and the
    largest peak in the first, a middle or the last pack."""
    rng = np.random.default_rng(seed)
    for world in WORLDS:
        for where in (("first",) if world == 1 else ("first", "last") if world == 2 else ("first", "middle", "last")):
            hists = np.zeros((world, BINS), dtype=np.uint32)
            for r in range(world):
                k = int(rng.integers(1, 30))
                hists[r, rng.integers(3000, 9000, k)] = rng.integers(1, 400, k).astype(np.uint32)
                hists[r, 6000 + CHUNK * (r % 5)] += 7  # bins that several packs share
            peaks = [0.1 + 0.5 * float(rng.random()) for _ in range(world)]
            if world > 1:
                hists[0, 11000] = U32_MAX           # + 2 -> 1: without the wrap the scan would stop here
                hists[world - 1, 11000] = 2
                hists[0, 47] = 1 << 31              # + 2^31 -> exactly 0
                hists[world // 2 if world > 2 else 1, 47] = 1 << 31
                hists[:, 2999] = U32_MAX // world + 1  # every pack the same: the sum wraps to world - (2^32 mod world), or to 0
                peaks[{"first": 1, "middle": world - 1, "last": 0}[where]] = 0.0
            peaks[{"first": 0, "middle": world // 2, "last": world - 1}[where]] = 1.0 + 0.25 * world
            yield f"world{world}-peak-{where}", np.stack([pack(h, p) for h, p in zip(hists, peaks)])
