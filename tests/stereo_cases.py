"""The stereo image scan (include/mp3rgain_amd_stereo.h) restated with numpy and Python integers, and the cases the CPU and GPU
tests share.

The restatement is independent of the library's records and of its cutting: q is numpy arithmetic on the stored values, a
block's sums are int64 reductions (|q| <= 2^15 and the cases are short, so nothing can overflow), a lag's sum is one int64 dot
product of two slices, the choice of the two lags is Python's max over tuples, EMM and ESS are Python integers and float(int) is
their one rounding.  The case list takes the kernels' own boundaries (the frames of a piece P and of a tile T) from
rg_stereo_kernel_shape.  A case is a group: the tracks that one call measures with one radius and one block length, because
both are options of the call.  Not part of the product."""
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

EXACT_FIELDS = ("status", "flags", "frames", "sample_rate", "channels", "format", "dropped_frames", "block_frames", "radius", "blocks",
                "active_blocks", "neg_blocks", "mono_blocks", "lag", "anti_lag", "equal_frames", "opposite_frames", "zero_frames", "nonfinite",
                "ell", "err", "elr", "lag_sum", "anti_sum")                                    # the same on every route
FINISH_FIELDS = ("correlation", "lag_correlation", "anti_correlation", "balance_db", "side_db")  # behind a sqrt or a log10
FINISH_RTOL = 1e-12  # the host's sqrt, division and log10 and Python's may differ in the last bits

Tr = namedtuple("Tr", "name channels sample_rate")  # .channels: planes of one dtype and length (tests/arena_layouts.pack takes these)
Group = namedtuple("Group", "name radius block_frames tracks short")  # the options as Analyzer.stereo_arena takes them (None = default)

DTYPES = {_capi.FMT_F32_PLANAR: np.float32, _capi.FMT_S16_PLANAR: np.int16, _capi.FMT_S32_PLANAR: np.int32}
FMT = {np.dtype(v): k for k, v in DTYPES.items()}
TAGS = {np.dtype(np.int16): "s16", np.dtype(np.int32): "s32", np.dtype(np.float32): "f32"}
MAX_BLOCK, MAX_RADIUS = 384000, 255
DEFAULTS = {"radius": 64, "phase_permille": 587, "delay_permille": 420, "mono_db": 40, "balance_db_limit": 12}
DELAYS = (-255, -64, -3, -1, 1, 2, 17, 64, 255)


def shape(fmt):
    """(P, T) of a format: frames of a piece of the moments kernel and of a tile of the lag kernel."""
    from mp3rgain_amd import stereo_kernel_shape

    p, t, _, _, _ = stereo_kernel_shape(fmt)
    return p, t


# ---- the definitions ----------------------------------------------------------------------------------------------------------
def quantise(x):
    """-> (q as int64, number of non-finite samples)."""
    if x.dtype == np.int16:
        return x.astype(np.int64), 0
    if x.dtype == np.int32:
        return (x >> 16).astype(np.int64), 0  # numpy shifts a signed integer arithmetically: floor
    finite = np.isfinite(x)
    q = np.zeros(len(x), np.int64)
    q[finite] = np.minimum(np.rint(np.clip(x[finite].astype(np.float64), -1.0, 1.0) * 32768.0), 32767.0).astype(np.int64)  # rint: half to even
    return q, int(np.count_nonzero(~finite))


def lag_sums(ql, qr, radius):
    """[C_d for d = -radius .. radius], Python ints."""
    n = len(ql)
    out = []
    for d in range(-radius, radius + 1):
        if abs(d) >= n:
            out.append(0)
        elif d >= 0:
            out.append(int(np.dot(ql[:n - d], qr[d:])))
        else:
            out.append(int(np.dot(ql[-d:], qr[:n + d])))
    return out


def _ratio_db(a, b):
    if a > 0 and b > 0:
        return 10.0 * math.log10(float(a) / float(b))
    return math.inf if a > 0 else (-math.inf if b > 0 else 0.0)


def want_track(tr, radius=None, block_frames=None, **thresholds) -> dict:
    th = dict(DEFAULTS, **thresholds)
    R = th["radius"] if radius is None else radius
    B = int(block_frames) if block_frames else int(tr.sample_rate)
    dt = np.dtype(tr.channels[0].dtype)
    n = len(tr.channels[0])
    w = {f: 0 for f in EXACT_FIELDS}
    w.update({f: 0.0 for f in FINISH_FIELDS})
    w.update(frames=n, sample_rate=tr.sample_rate, channels=len(tr.channels), format=FMT[dt], block_frames=B, radius=R)
    if len(tr.channels) < 2:
        w["flags"] = _capi.ST_COMPLETE | _capi.ST_MONO
        w["sums"] = [0] * (2 * R + 1)
        return w
    xl, xr = tr.channels[0], tr.channels[1]
    ql, nf_l = quantise(xl)
    qr, nf_r = quantise(xr)
    if dt == np.float32:
        equal, opposite = xl == xr, (xl == -xr) & (xl != 0)
    else:
        equal, opposite = xl == xr, (xl.astype(np.int64) + xr.astype(np.int64) == 0) & (xl != 0)
    zero = (xl == 0) & (xr == 0)
    ell = err = elr = blocks = active = neg = mono = 0
    if n:
        starts = np.arange(0, n, B, dtype=np.int64)
        for s, a, b, c, e in zip(starts, np.add.reduceat(ql * ql, starts), np.add.reduceat(qr * qr, starts), np.add.reduceat(ql * qr, starts),
                                 np.add.reduceat(equal.astype(np.int64), starts)):
            a, b, c = int(a), int(b), int(c)
            ell, err, elr, blocks = ell + a, err + b, elr + c, blocks + 1
            active += a + b > 0
            neg += c < 0
            mono += a + b > 0 and int(e) == min(B, n - int(s))
    sums = lag_sums(ql, qr, R)
    assert sums[R] == elr
    lag = max(range(-R, R + 1), key=lambda d: (sums[d + R], -abs(d), d < 0))
    anti = max(range(-R, R + 1), key=lambda d: (-sums[d + R], -abs(d), d < 0))
    w.update(blocks=blocks, active_blocks=active, neg_blocks=neg, mono_blocks=mono, lag=lag, anti_lag=anti, equal_frames=int(equal.sum()),
             opposite_frames=int(opposite.sum()), zero_frames=int(zero.sum()), nonfinite=nf_l + nf_r, ell=ell, err=err, elr=elr, lag_sum=sums[lag + R],
             anti_sum=sums[anti + R], sums=sums)
    if ell > 0 and err > 0:
        norm = math.sqrt(float(ell)) * math.sqrt(float(err))
        w.update(correlation=float(elr) / norm, lag_correlation=float(w["lag_sum"]) / norm, anti_correlation=float(w["anti_sum"]) / norm)
    w["balance_db"] = _ratio_db(ell, err)
    w["side_db"] = _ratio_db(ell + err - 2 * elr, ell + err + 2 * elr)
    dual = n > 0 and w["equal_frames"] == n
    flags = _capi.ST_COMPLETE
    flags |= _capi.ST_MORE_CHANNELS if len(tr.channels) > 2 else 0
    flags |= _capi.ST_SILENT if ell + err == 0 else 0
    flags |= _capi.ST_NONFINITE if nf_l + nf_r else 0
    flags |= _capi.ST_DUAL_MONO if dual else 0
    flags |= _capi.ST_INVERTED_COPY if w["opposite_frames"] > 0 and w["opposite_frames"] + w["zero_frames"] == n else 0
    flags |= _capi.ST_OUT_OF_PHASE if w["correlation"] <= -th["phase_permille"] / 1000.0 else 0
    flags |= _capi.ST_NEAR_MONO if not dual and w["side_db"] <= -float(th["mono_db"]) else 0
    flags |= _capi.ST_ONE_SIDED if abs(w["balance_db"]) >= float(th["balance_db_limit"]) or (ell == 0) != (err == 0) else 0
    flags |= _capi.ST_DELAYED if lag != 0 and w["lag_sum"] > elr and w["lag_correlation"] >= th["delay_permille"] / 1000.0 else 0
    w["flags"] = flags
    return w


def got(r) -> dict:
    """An rg_stereo_result as want_track's dict (without the sums)."""
    return {f: getattr(r, f) for f in EXACT_FIELDS + FINISH_FIELDS}


def _close(a, b):
    return a == b or (math.isfinite(a) and math.isfinite(b) and abs(a - b) <= FINISH_RTOL * max(abs(a), abs(b)))


def differences(g, w) -> list:
    """The fields in which two such dicts differ: exactly everywhere in front of the finish, FINISH_RTOL behind it."""
    return [(f, g[f], w[f]) for f in EXACT_FIELDS if g[f] != w[f]] + [(f, g[f], w[f]) for f in FINISH_FIELDS if not _close(g[f], w[f])]


# ---- the cases ----------------------------------------------------------------------------------------------------------------
def _noise(rng, dtype, n):
    dtype = np.dtype(dtype)
    if dtype == np.float32:
        return (rng.standard_normal(n) * 0.4).astype(np.float32)  # a sample in a hundred beyond full scale
    info = np.iinfo(dtype)
    return rng.integers(info.min, info.max, size=n, endpoint=True, dtype=np.int64).astype(dtype)


def _scaled(v, dtype):
    """Small integers as samples of a format whose q they are."""
    dtype = np.dtype(dtype)
    v = np.asarray(v, dtype=np.int64)
    if dtype == np.float32:
        return (v / 32768.0).astype(np.float32)
    return (v << 16).astype(np.int32) if dtype == np.int32 else v.astype(np.int16)


def delayed(x, d):
    """y with y[n + d] = x[n]: x as the right channel hears it `d` frames late (early when d < 0), zeros where nothing arrives."""
    y = np.zeros_like(x)
    n = len(x)
    if abs(d) < n:
        if d >= 0:
            y[d:] = x[:n - d]
        else:
            y[:n + d] = x[-d:]
    return y


@lru_cache(maxsize=None)
def groups():
    """Every case, grouped by the options of its call."""
    rng = np.random.default_rng(0x57E0)
    by_opts = {}

    def add(R, B, tr, short=True):
        by_opts.setdefault((R, B), [[], True])
        by_opts[(R, B)][0].append(tr)
        by_opts[(R, B)][1] = by_opts[(R, B)][1] and short

    for fmt, dtype in DTYPES.items():
        P, T = shape(fmt)
        tag = TAGS[np.dtype(dtype)]
        # N on the kernels' seams at every radius (N < R included), and at one radius every block length
        for R in (0, 1, 7, 64, 255):
            lengths = sorted({0, 1, 2, R, R + 1, 2 * R + 1, P - 1, P, P + 1, T - 1, T, T + 1, T + R, 2 * T + 3})
            for B in (None,) if R != 7 else (None, 1, 7, P, T + 1):
                for N in lengths:
                    rate = 44100 if N % 2 else 3001  # the default block: one block, or a few with a remainder
                    add(R, B, Tr(f"{tag}_n{N}", [_noise(rng, dtype, N), _noise(rng, dtype, N)], rate), short=N <= 2 * R + 1 or B in (1, 7))
        # structure: identical channels, one the negated other with zeros in between, one channel silent, one track of 1 and one of 8 channels
        x = _noise(rng, dtype, T + 5)
        neg = _scaled(rng.integers(-32767, 32767, size=T + 5, endpoint=True), dtype)
        neg[::3] = 0
        for R, B in ((64, None), (7, 7)):
            add(R, B, Tr(f"{tag}_dual_mono", [x, x.copy()], 44100))
            add(R, B, Tr(f"{tag}_inverted", [neg, -neg], 44100))
            add(R, B, Tr(f"{tag}_left_only", [x, np.zeros_like(x)], 44100))
            add(R, B, Tr(f"{tag}_right_only", [np.zeros_like(x), x], 44100))
            add(R, B, Tr(f"{tag}_silent", [np.zeros(100, dtype), np.zeros(100, dtype)], 44100))
            add(R, B, Tr(f"{tag}_one_channel", [x[:300].copy()], 44100))
            add(R, B, Tr(f"{tag}_eight_channels", [_noise(rng, dtype, 300) for _ in range(8)], 44100))
            # nearly mono: the channels differ in one frame, by ten steps of q
            x2, y = x.copy(), x.copy()
            x2[7], y[7] = _scaled([-5], dtype)[0], _scaled([5], dtype)[0]
            add(R, B, Tr(f"{tag}_near_mono", [x2, y], 44100))
            # ties: +1 and -1 share the largest sum (the negative lag wins); -2 and +1 do (the smaller |d| wins); the same for the smallest
            for name, l, r in (("tie_sign", [0, 0, 0, 0, 9, 0, 0, 0, 0], [0, 0, 0, 9, 0, 9, 0, 0, 0]), ("tie_abs", [0, 0, 0, 0, 9, 0, 0, 0, 0], [0, 0, 9, 0, 0, 9, 0, 0, 0]),
                                ("tie_anti_sign", [0, 0, 0, 0, 9, 0, 0, 0, 0], [0, 0, 0, -9, 0, -9, 0, 0, 0]), ("tie_anti_abs", [0, 0, 0, 0, 9, 0, 0, 0, 0], [0, 0, -9, 0, 0, -9, 0, 0, 0])):
                add(R, B, Tr(f"{tag}_{name}", [_scaled(l, dtype), _scaled(r, dtype)], 44100))
        # the right channel a copy of the left, delayed by d
        base = _noise(rng, dtype, T + 255)
        if dtype == np.float32:
            base = np.clip(base, -1.0, 1.0)
        for d in DELAYS:
            add(255, None, Tr(f"{tag}_delay{d}", [base, delayed(base, d)], 44100), short=False)
            if abs(d) <= 64:
                add(64, None, Tr(f"{tag}_delay{d}", [base[:1000].copy(), delayed(base[:1000], d)], 44100))
    # values
    P16, T = shape(_capi.FMT_S16_PLANAR)
    mn = np.full(2 * T + 3, -32768, np.int16)
    for R, B in ((64, None), (7, 7)):
        add(R, B, Tr("s16_all_minus_full_scale", [mn, mn.copy()], 44100), short=False)  # 8195 * 2^30 > 2^32: a 32-bit sum wraps
        add(R, B, Tr("s16_minus_against_plus_full_scale", [mn, np.full(2 * T + 3, 32767, np.int16)], 44100), short=False)
        add(R, B, Tr("s32_all_int_min", [np.full(2 * T + 3, -2 ** 31, np.int32), np.full(2 * T + 3, -2 ** 31, np.int32)], 44100), short=False)
        # the floor shift: negative values with low bits set; opposite pairs whose q are not opposite; INT_MIN against itself is not opposite
        v = np.array([-1, -65535, -65536, -65537, 65535, 65536, 0x7FFFFFFF, -0x7FFFFFFF, -2 ** 31, 0x0000FFFF, -0x12345679, 1], np.int64)
        add(R, B, Tr("s32_floor_shift", [v.astype(np.int32), np.roll(v, 1).astype(np.int32)], 44100))
        add(R, B, Tr("s32_opposite_raw", [v.astype(np.int32), np.where(v == -2 ** 31, v, -v).astype(np.int32)], 44100))
        f = np.float32
        h = 1.0 / 65536.0  # half a step of q
        edge = np.array([1.0, -1.0, 1.5, -1.5, 1e30, -1e30, 0.99998474, 0.9999924, -0.9999924, h, 3 * h, -h, -3 * h, 5 * h, 0.5 * h, 1.5 * h, -0.0, 0.0, 1e-45,
                         -1e-45, 1e-39, -1.1754942e-38, 32766.5 / 32768.0, 32767.5 / 32768.0], f)
        add(R, B, Tr("f32_edges", [edge, edge[::-1].copy()], 44100))
        add(R, B, Tr("f32_signed_zeros", [np.array([-0.0, 0.0, -0.0, 0.0, 0.5], f), np.array([0.0, -0.0, -0.0, 0.0, -0.5], f)], 44100))
        for where in ("first", "middle", "last"):
            k = {"first": 0, "middle": 17, "last": 34}[where]
            for both in (False, True):
                a, b = _noise(rng, f, 35), _noise(rng, f, 35)
                a[k] = np.nan if both else np.inf
                if both:
                    b[k] = -np.inf
                add(R, B, Tr(f"f32_nonfinite_{where}_{'both' if both else 'one'}", [a, b], 44100))
        add(R, B, Tr("f32_nan_against_itself", [np.full(9, np.nan, f), np.full(9, np.nan, f)], 44100))
    return tuple(Group(f"r{R}_b{B}", R, B, tuple(trs), short) for (R, B), (trs, short) in by_opts.items())


@lru_cache(maxsize=None)
def wants(name):
    """{track name: want_track} of one group, computed once and shared."""
    g = next(g for g in groups() if g.name == name)
    return {tr.name: want_track(tr, g.radius, g.block_frames) for tr in g.tracks}
