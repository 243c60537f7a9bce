"""The null test of two tracks (include/mp3rgain_amd_compare.h) restated with numpy and Python integers, and the cases the CPU
and GPU tests share.

The restatement follows the header's words, not the C++: q is numpy arithmetic on the stored values, a lag's sum is one int64 dot
product of two slices (|q| <= 2^15 and the cases are short, so nothing can overflow), the sums over segments and channels, T, the
determinant aa bb - ab^2 and every comparison in front of the finish are Python integers, and float(int) is their one rounding.
The case list takes the kernels' own boundaries (the frames of a piece P and of a tile T) from rg_compare_kernel_shape.  A case is
a call: the tracks and the pairs that one call measures with one set of options.  Not part of the product."""
import math
import sys
from collections import namedtuple
from functools import lru_cache
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

from mp3rgain_amd import _capi  # noqa: E402

FLOAT_FIELDS = ("lock", "gain_db", "null_unity_db", "null_db", "residual_lsb2", "worst_block_db", "gain_min_db", "gain_max_db")  # the finish
EXACT_FIELDS = tuple(f for f, _ in _capi.CompareRecord._fields_ if f not in FLOAT_FIELDS + ("reserved",))  # the same on every route
BLOCK_FIELDS = ("aa", "bb", "ab", "first_diff", "equal", "max_diff", "frames")
FINISH_RTOL = 1e-12  # the host's sqrt, division and log10 and Python's may differ in the last bits
NONE = _capi.CMP_NONE

Tr = namedtuple("Tr", "name channels sample_rate")  # .channels: planes of one dtype and length (tests/arena_layouts.pack takes these)
Call = namedtuple("Call", "name opts tracks pairs")  # opts: a dict as compare_arena takes it; pairs: (a, b, hint)

DTYPES = {_capi.FMT_F32_PLANAR: np.float32, _capi.FMT_S16_PLANAR: np.int16, _capi.FMT_S32_PLANAR: np.int32}
FMT = {np.dtype(v): k for k, v in DTYPES.items()}
TAGS = {np.dtype(np.int16): "s16", np.dtype(np.int32): "s32", np.dtype(np.float32): "f32"}
DEFAULTS = dict(radius=1024, segments=4, segment_frames=262144, block_frames=None, drift_frames=1, lock_permille=606, requant_millilsb2=18156)
RADII = (0, 1, 15, 16, 17, 255, 256, 2047)


def shape(fmt_a, fmt_b=None):
    """(P, T) of a pair of formats: frames of a piece of the moments kernel and of a tile of the lag kernel."""
    from mp3rgain_amd import compare_kernel_shape

    p, t, _, _, _ = compare_kernel_shape(fmt_a, fmt_b)
    return p, t


# ---- the definitions ----------------------------------------------------------------------------------------------------------
def quantise(x):
    """-> (q as int64, mask of the non-finite samples)."""
    if x.dtype == np.int16:
        return x.astype(np.int64), np.zeros(len(x), bool)
    if x.dtype == np.int32:
        return (x >> 16).astype(np.int64), np.zeros(len(x), bool)  # numpy shifts a signed integer arithmetically: floor
    finite = np.isfinite(x)
    q = np.zeros(len(x), np.int64)
    q[finite] = np.minimum(np.rint(np.clip(x[finite].astype(np.float64), -1.0, 1.0) * 32768.0), 32767.0).astype(np.int64)  # rint: half to even
    return q, ~finite


def lag_row(qa, qb, start, length, h, R):
    """[C_d for d = -R .. R] + [EA, EB] of one segment of one channel, Python ints."""
    nb = len(qb)
    row = []
    for d in range(-R, R + 1):
        lo, hi = max(start, -(h + d)), min(start + length, nb - h - d)
        row.append(int(np.dot(qa[lo:hi], qb[lo + h + d:hi + h + d])) if hi > lo else 0)
    seg = qa[start:start + length]
    lo, hi = max(start, -h), min(start + length, nb - h)
    win = qb[lo + h:hi + h] if hi > lo else qb[:0]
    return row + [int(np.dot(seg, seg)), int(np.dot(win, win))]


def pick(rows, R):
    """(d*, sigma, lock) of some rows taken together."""
    T = [sum(r[k] for r in rows) for k in range(2 * R + 1)]
    d = max(range(-R, R + 1), key=lambda d: (abs(T[d + R]), -abs(d), d < 0))
    ea, eb = sum(r[2 * R + 1] for r in rows), sum(r[2 * R + 2] for r in rows)
    lock = float(abs(T[d + R])) / math.sqrt(float(ea) * float(eb)) if ea and eb else 0.0
    return d, (-1 if T[d + R] < 0 else 1), lock


def _db10(num, den):
    return 10.0 * math.log10(float(num) / float(den)) if num > 0 else -math.inf


def want_pair(tracks, a, b, hint, **opts) -> dict:
    """The record of pair (a, b, hint) as a dict, with "rows" ([segment][channel] -> row) and "block_rows" (dicts)."""
    o = dict(DEFAULTS, **{k: v for k, v in opts.items() if v is not None})
    R, S, G = o["radius"], o["segments"], o["segment_frames"]
    ta, tb = tracks[a], tracks[b]
    na, nb = len(ta.channels[0]), len(tb.channels[0])
    cc = min(len(ta.channels), len(tb.channels))
    same = ta.channels[0].dtype == tb.channels[0].dtype
    w = {f: 0 for f in EXACT_FIELDS}
    w.update({f: 0.0 for f in FLOAT_FIELDS})
    w.update(a=a, b=b, frames_a=na, frames_b=nb, sample_rate=ta.sample_rate, channels=cc, format_a=FMT[ta.channels[0].dtype], format_b=FMT[tb.channels[0].dtype],
             radius=R, hint=hint, first_diff=NONE, rows=[], block_rows=[])
    flags = _capi.CMP_COMPLETE | (_capi.CMP_CHANNELS_DIFFER if len(ta.channels) != len(tb.channels) else 0)
    w["flags"] = flags
    if ta.sample_rate != tb.sample_rate:
        w["flags"] |= _capi.CMP_RATE
        return w
    B = int(o["block_frames"] or ta.sample_rate)
    w["block_frames"] = B
    n0, n1 = max(0, -hint), min(na, nb - hint)
    V = n1 - n0
    if V <= 0:
        w["flags"] |= _capi.CMP_NO_OVERLAP
        return w
    segs = [(n0, V)] if G == 0 or V <= S * G else [(n0 + (2 * s + 1) * (V - G) // (2 * S), G) for s in range(S)]
    qa, qb, nfa, nfb = [], [], [], []
    for c in range(cc):
        q, nf = quantise(ta.channels[c])
        qa.append(q)
        nfa.append(nf)
        q, nf = quantise(tb.channels[c])
        qb.append(q)
        nfb.append(nf)
    rows = [[lag_row(qa[c], qb[c], start, length, hint, R) for c in range(cc)] for start, length in segs]
    d, sigma, lock = pick([r for seg in rows for r in seg], R)
    need = o["lock_permille"] / 1000.0
    seg_lags = [hint + ds for ds, _, ls in (pick(seg, R) for seg in rows) if ls >= need]
    lag = hint + d
    m0, m1 = max(0, -lag), min(na, nb - lag)
    W = m1 - m0
    assert W > 0
    aa = bb = ab = equal = nonfinite = max_diff = differing = 0
    first = NONE
    blocks = []
    for s in range(0, W, B):
        n = min(B, W - s)
        blk = dict(aa=0, bb=0, ab=0, first_diff=NONE, equal=0, max_diff=0, frames=n)
        for c in range(cc):
            sa, sb = slice(m0 + s, m0 + s + n), slice(m0 + lag + s, m0 + lag + s + n)
            x, y = qa[c][sa], qb[c][sb]
            eq = (ta.channels[c][sa] == tb.channels[c][sb]) if same and sigma > 0 else (x == sigma * y)
            blk["aa"] += int(np.dot(x, x))
            blk["bb"] += int(np.dot(y, y))
            blk["ab"] += int(np.dot(x, y))
            blk["equal"] += int(np.count_nonzero(eq))
            blk["max_diff"] = max(blk["max_diff"], int(np.abs(x - sigma * y).max()))
            if not eq.all():
                blk["first_diff"] = min(blk["first_diff"], m0 + s + int(np.argmin(eq)))
            nonfinite += int(np.count_nonzero(nfa[c][sa])) + int(np.count_nonzero(nfb[c][sb]))
        blocks.append(blk)
        aa, bb, ab, equal = aa + blk["aa"], bb + blk["bb"], ab + blk["ab"], equal + blk["equal"]
        first, max_diff = min(first, blk["first_diff"]), max(max_diff, blk["max_diff"])
        differing += blk["equal"] < n * cc
    w.update(segments=len(segs), locked_segments=len(seg_lags), polarity=sigma, max_diff=max_diff, lag=lag, seg_lag_min=min(seg_lags, default=0),
             seg_lag_max=max(seg_lags, default=0), overlap=W, a_head=m0, a_tail=na - m1, b_head=m0 + lag, b_tail=nb - m1 - lag, blocks=len(blocks),
             differing_blocks=differing, equal=equal, first_diff=first, nonfinite=nonfinite, aa=aa, bb=bb, ab=ab, lock=lock, rows=rows, block_rows=blocks)
    # the finish
    gamma = float(ab) / float(bb) if bb else 0.0
    det = aa * bb - ab * ab
    g2 = gamma * gamma
    w["gain_db"] = 20.0 * math.log10(abs(gamma)) if ab and bb else 0.0
    w["null_unity_db"] = _db10(aa - 2 * sigma * ab + bb, aa) if aa else 0.0
    w["null_db"] = _db10(det, aa * bb) if aa and bb else 0.0
    w["residual_lsb2"] = (float(det) / float(bb) / float(W * cc) / max(g2, 1.0)) if bb else float(aa) / float(W * cc)
    worst = gains = None
    for k, blk in enumerate(blocks):
        if blk["aa"] > 0:
            res = (float(blk["aa"]) - (2.0 * gamma) * float(blk["ab"])) + g2 * float(blk["bb"])
            db = 10.0 * math.log10(res / float(blk["aa"])) if res > 0.0 else -math.inf
            if worst is None or db > worst[1]:
                worst = (k, db)
        if 100 * blk["aa"] * len(blocks) >= aa and blk["ab"] and blk["bb"]:
            g = 20.0 * math.log10(abs(float(blk["ab"]) / float(blk["bb"])))
            gains = (g, g) if gains is None else (min(gains[0], g), max(gains[1], g))
    if worst:
        w["worst_block"], w["worst_block_db"] = worst
    if gains:
        w["gain_min_db"], w["gain_max_db"] = gains
    identical = sigma > 0 and equal == W * cc
    locked = lock >= need
    flags |= _capi.CMP_LOCKED if locked else _capi.CMP_UNRELATED
    flags |= _capi.CMP_AT_EDGE if R > 0 and abs(d) == R else 0
    flags |= _capi.CMP_DRIFT if len(seg_lags) > 1 and max(seg_lags) - min(seg_lags) > o["drift_frames"] else 0
    flags |= _capi.CMP_IDENTICAL if identical else 0
    flags |= _capi.CMP_SHIFTED if lag else 0
    flags |= _capi.CMP_LENGTHS if m0 or na - m1 or m0 + lag or nb - m1 - lag else 0
    flags |= _capi.CMP_INVERTED if sigma < 0 else 0
    flags |= _capi.CMP_NONFINITE if nonfinite else 0
    flags |= _capi.CMP_RAW if same and sigma > 0 else 0
    if locked and not identical:
        flags |= _capi.CMP_SAME_MASTER if w["residual_lsb2"] <= o["requant_millilsb2"] / 1000.0 else _capi.CMP_DIFFERS
    w["flags"] = flags
    return w


def got(r) -> dict:
    """An rg_compare_result as want_pair's dict (without the rows)."""
    return {f: getattr(r, f) for f in EXACT_FIELDS + FLOAT_FIELDS}


def _close(a, b):
    return a == b or (math.isfinite(a) and math.isfinite(b) and abs(a - b) <= FINISH_RTOL * max(abs(a), abs(b)))


def differences(g, w) -> list:
    """The fields in which two such dicts differ: exactly everywhere in front of the finish, FINISH_RTOL behind it."""
    return [(f, g[f], w[f]) for f in EXACT_FIELDS if g[f] != w[f]] + [(f, g[f], w[f]) for f in FLOAT_FIELDS if not _close(g[f], w[f])]


def row_differences(rows, blocks, w, radius) -> list:
    """... and the lag rows ([segment][8][2R + 3]) and block rows of one pair against want_pair's."""
    bad = []
    for s, seg in enumerate(w["rows"]):
        for c, row in enumerate(seg):
            if [int(v) for v in rows[s][c]] != row:
                bad.append(("row", s, c))
    n_meas = len(w["rows"]) * (len(w["rows"][0]) if w["rows"] else 0)
    if int(np.count_nonzero(np.any(rows != 0, axis=-1))) > n_meas:
        bad.append(("rows that were not measured are not zero",))
    if len(blocks) != len(w["block_rows"]):
        bad.append(("blocks", len(blocks), len(w["block_rows"])))
    for k, (g, blk) in enumerate(zip(blocks, w["block_rows"])):
        if any(getattr(g, f) != blk[f] for f in BLOCK_FIELDS):
            bad.append(("block", k, {f: (getattr(g, f), blk[f]) for f in BLOCK_FIELDS if getattr(g, f) != blk[f]}))
    return bad


# ---- the cases ----------------------------------------------------------------------------------------------------------------
def noise(rng, dtype, n):
    dtype = np.dtype(dtype)
    if dtype == np.float32:
        return (rng.standard_normal(n) * 0.4).astype(np.float32)  # a sample in a hundred beyond full scale
    info = np.iinfo(dtype)
    return rng.integers(info.min, info.max, size=n, endpoint=True, dtype=np.int64).astype(dtype)


def scaled(v, dtype):
    """Small integers as samples of a format whose q they are."""
    dtype = np.dtype(dtype)
    v = np.asarray(v, dtype=np.int64)
    if dtype == np.float32:
        return (v / 32768.0).astype(np.float32)
    return (v << 16).astype(np.int32) if dtype == np.int32 else v.astype(np.int16)


def shifted(rng, x, d, n=None):
    """y of n frames with y[k + d] = x[k], fresh noise where nothing of x arrives."""
    n = len(x) if n is None else n
    y = noise(rng, x.dtype, n)
    lo, hi = max(0, -d), min(len(x), n - d)
    if hi > lo:
        y[lo + d:hi + d] = x[lo:hi]
    return y


def convert(x, dtype):
    """The samples of x in another format, by way of q."""
    q, _ = quantise(x)
    return scaled(q, dtype)


class _Builder:
    def __init__(self):
        self.calls = {}

    def add(self, name, opts, a, b, hint, rate_a=44100, rate_b=None):
        """One pair: two new tracks of the call called `name` (a and b: lists of planes)."""
        opts, tracks, pairs = self.calls.setdefault(name, (opts, [], []))
        k = len(tracks)
        tag = f"{name}/{len(pairs)}"
        tracks += [Tr(tag + "a", list(a), rate_a), Tr(tag + "b", list(b), rate_a if rate_b is None else rate_b)]
        pairs.append((k, k + 1, hint))


@lru_cache(maxsize=None)
def calls():
    """Every case, grouped by the options of its call."""
    rng = np.random.default_rng(0xC0DE)
    B = _Builder()
    P16, T = shape(_capi.FMT_S16_PLANAR)
    one = dict(segments=1, segment_frames=0)
    # the overlap on the kernels' seams at every radius, the true offset cycling through -R, -1, 0, +1, +R from the hint
    lengths = (1, 15, 16, 17, T - 1, T, T + 1, 2 * T + 3)
    for R in RADII:
        for dtype in (np.int16, np.int32, np.float32) if R == 17 else (np.int16,):
            tag = TAGS[np.dtype(dtype)]
            for k, V in enumerate(lengths):
                off = (-R, -1, 0, 1, R)[k % 5]
                x = noise(rng, dtype, V)
                B.add(f"r{R}_{tag}", dict(one, radius=R), [x, noise(rng, dtype, V)], [shifted(rng, x, off), noise(rng, dtype, V)], 0)
            x = noise(rng, dtype, 40)
            B.add(f"r{R}_{tag}", dict(one, radius=R), [x], [x.copy()], 40)     # an overlap of 0 frames: the hint puts the window behind b
            B.add(f"r{R}_{tag}", dict(one, radius=R), [x], [x.copy()], -40)    # ... and in front of it
            B.add(f"r{R}_{tag}", dict(one, radius=R), [x], [x.copy()], 39)     # a single frame is left, at b's end
            B.add(f"r{R}_{tag}", dict(one, radius=R), [x], [x.copy()], -39)    # ... and at its start
    # b shorter than a, and b ending inside the lag window
    x = noise(rng, np.int16, T + 900)
    B.add("r255_s16", dict(one, radius=255), [x], [x[:T + 100].copy()], 0)
    B.add("r255_s16", dict(one, radius=255), [x], [x[300:T + 400].copy()], -300)
    B.add("r255_s16", dict(one, radius=255), [x[:T].copy()], [x[:T + 7].copy()], 0)
    # segments: 1, 4 and 16 of 4096, 4097 and 0 frames, of a copy 3 frames late (and one whose second half is 5 frames late: drift)
    n = 17 * (T + 1) + 100
    x = noise(rng, np.float32, n)
    y = shifted(rng, x, 3)
    z = y.copy()
    z[n // 2 + 5:] = x[n // 2:n - 5]
    for S in (1, 4, 16):
        for G in (T, T + 1, 0):
            o = dict(radius=16, segments=S, segment_frames=G)
            B.add(f"seg{S}x{G}", o, [x], [y], 0)
            B.add(f"seg{S}x{G}", o, [x], [z], 2)
            B.add(f"seg{S}x{G}", o, [x[:2 * T + 3].copy()], [y[:2 * T + 3].copy()], 0)  # V <= S * G for S = 4 and 16: one segment
    # block lengths, all three formats, same and mixed, in both orders; a copy one frame late that differs here and there
    for blk in (1, 7, T + 1, None):
        for da in DTYPES.values():
            for db in DTYPES.values():
                if blk in (1, 7) and da != db and np.dtype(da) != np.int16:
                    continue
                V = 2 * T + 3 if blk != 1 else 300
                x = noise(rng, da, V)
                if np.dtype(da) == np.float32:
                    x = np.clip(x, -1.0, 1.0)
                y = shifted(rng, convert(x, db), 1)
                y[::97] = noise(rng, db, len(y[::97]))
                B.add(f"b{blk}", dict(one, radius=16, block_frames=blk), [x, noise(rng, da, V)], [y, noise(rng, db, V)], 0)
    # 1, 2 and 8 channels, the counts differing
    for ca, cb in ((1, 1), (1, 2), (2, 1), (2, 8), (8, 8)):
        xs = [noise(rng, np.int16, T + 5) for _ in range(8)]
        B.add("channels", dict(one, radius=16), xs[:ca], [shifted(rng, x, -2) for x in xs[:cb]], 0)
    # an inverted copy, of each format (a 16-bit -32768 has no negative: such samples differ by one step)
    for dtype in DTYPES.values():
        x = noise(rng, dtype, T + 5)
        neg = np.where(x == np.iinfo(dtype).min, np.iinfo(dtype).max, -x).astype(dtype) if np.dtype(dtype) != np.float32 else -x
        B.add("values", dict(one, radius=16), [x], [shifted(rng, neg, 2)], 0)
    # the largest sums: everything -32768
    mn = np.full(2 * T + 3, -32768, np.int16)
    B.add("values", dict(one, radius=16), [mn, mn.copy()], [mn.copy(), mn.copy()], 0)
    B.add("values", dict(one, radius=16), [mn], [np.full(2 * T + 3, 32767, np.int16)], 0)
    B.add("values", dict(one, radius=16), [np.full(2 * T + 3, -2 ** 31, np.int32)], [np.full(2 * T + 3, -2 ** 31, np.int32)], 0)
    # float edges, and non-finite samples at the first and the last frame of either side
    f = np.float32
    h = 1.0 / 65536.0  # half a step of q
    edge = np.array([1.0, -1.0, 1.5, -1.5, 1e30, -1e30, 0.99998474, 0.9999924, -0.9999924, h, 3 * h, -h, -3 * h, 5 * h, 0.5 * h, 1.5 * h, -0.0, 0.0, 1e-45, -1e-45,
                     1e-39, -1.1754942e-38, 32766.5 / 32768.0, 32767.5 / 32768.0], f)
    B.add("values", dict(one, radius=16), [edge], [edge.copy()], 0)
    B.add("values", dict(one, radius=16), [edge], [convert(edge, np.int16)], 0)
    B.add("values", dict(one, radius=16), [np.array([-0.0, 0.0, -0.0, 0.5], f)], [np.array([0.0, -0.0, -0.0, 0.5], f)], 0)
    for side in (0, 1):
        for where in (0, -1):
            pair = [np.clip(noise(rng, f, 700), -1, 1), None]
            pair[1] = pair[0].copy()
            pair[side][where] = np.nan if where else np.inf
            B.add("values", dict(one, radius=16), [pair[0]], [pair[1]], 0)
    B.add("values", dict(one, radius=16), [np.full(9, np.nan, f)], [np.full(9, np.nan, f)], 0)
    # a single differing sample: the first frame of a block, the last frame of a piece, the last frame of the overlap
    x = noise(rng, np.int16, P16 + 10)
    for blk, at in ((T + 1, T + 1), (None, P16 - 1), (None, P16 + 9), (T + 1, 0)):
        y = x.copy()
        y[at] ^= 1
        B.add(f"single_b{blk}", dict(one, radius=16, block_frames=blk), [x, x.copy()], [x.copy(), y], 0)
    # the two planes' 16-byte alignments against each other: every residue, in every format
    for dtype in DTYPES.values():
        x = noise(rng, dtype, T + 40)
        for d in range(-8, 9):
            B.add("residues", dict(one, radius=16), [x], [shifted(rng, x, d)], 0)
    # another sample rate: not compared
    x = noise(rng, np.int16, 100)
    B.add("values", dict(one, radius=16), [x], [x.copy()], 0, 44100, 48000)
    return tuple(Call(name, opts, tuple(tracks), tuple(pairs)) for name, (opts, tracks, pairs) in B.calls.items())


@lru_cache(maxsize=None)
def wants(name):
    """[want_pair] of one call, computed once and shared."""
    c = next(c for c in calls() if c.name == name)
    return tuple(want_pair(c.tracks, a, b, h, **c.opts) for a, b, h in c.pairs)
