"""The dynamic range figure (include/mp3rgain_amd_dr.h) restated with numpy and Python integers, and the cases the CPU and GPU
tests share.

The restatement is independent of the library's records and of its two-limb sums: a block's energy is a Python integer (put
together from three int64 sums of the 16-bit halves of |q|, none of which can overflow), float(int) is the one rounding,
`sorted` is the selection, and the sums of doubles are Python loops in ascending block index.  The case list takes the kernels'
own boundaries (the samples of a lane step C and of a workgroup piece T) from rg_dr_kernel_shape.  A case is a group: the
tracks that one call measures with one pair of options, because the block length is an option of the call.  Not part of the
product."""
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

RAW_FIELDS = ("top_ms", "mean_square", "peak", "peak2", "blocks", "top_blocks", "nonfinite")  # exact on every route
DB_FIELDS = ("dr", "peak_db", "rms_db")                                                       # behind a log10
TRACK_FIELDS = ("status", "flags", "frames", "sample_rate", "channels", "format", "dropped_frames", "block_frames", "dr")
TRACK_DB_FIELDS = ("dr_mean", "peak_db", "rms_db")
DB_RTOL = 1e-12  # the host's log10 and Python's may differ in the last bit

Tr = namedtuple("Tr", "name channels sample_rate")       # .channels: planes of one dtype and length (tests/arena_layouts.pack takes these)
Group = namedtuple("Group", "name block_frames top_permille tracks short")  # the options as Analyzer.dr_arena takes them (None = default)

DTYPES = {_capi.FMT_F32_PLANAR: np.float32, _capi.FMT_S16_PLANAR: np.int16, _capi.FMT_S32_PLANAR: np.int32}
FMT = {np.dtype(v): k for k, v in DTYPES.items()}
SCALE = {np.dtype(np.int16): 2.0 ** 15, np.dtype(np.int32): 2.0 ** 31, np.dtype(np.float32): 2.0 ** 23}
MAX_BLOCK = 1152000


def shape(fmt):
    """(C, T) of a format: samples of a lane step and of a piece."""
    from mp3rgain_amd import dr_kernel_shape

    c, t, _, _ = dr_kernel_shape(fmt)
    return c, t


# ---- the definitions ----------------------------------------------------------------------------------------------------------
def quantise(x):
    """-> (q as int64, number of non-finite samples)."""
    if x.dtype != np.float32:
        return x.astype(np.int64), 0
    finite = np.isfinite(x)
    q = np.zeros(len(x), np.int64)
    q[finite] = np.rint(np.clip(x[finite].astype(np.float64), -256.0, 256.0) * float(1 << 23)).astype(np.int64)  # rint: half to even
    return q, int(np.count_nonzero(~finite))


def block_energies(q, B):
    """-> ([E_i] Python ints, [p_i], [n_i]) of the blocks of B samples."""
    n = len(q)
    if n == 0:
        return [], [], []
    starts = np.arange(0, n, B, dtype=np.int64)
    a = np.abs(q)                       # <= 2^31
    hi, lo = a >> 16, a & 0xFFFF        # a^2 = hi^2 2^32 + 2 hi lo 2^16 + lo^2; every sum below stays under 2^30 * 2^21
    hh = np.add.reduceat(hi * hi, starts)
    hl = np.add.reduceat(hi * lo, starts)
    ll = np.add.reduceat(lo * lo, starts)
    E = [(int(x) << 32) + (int(y) << 17) + int(z) for x, y, z in zip(hh, hl, ll)]
    p = [int(v) for v in np.maximum.reduceat(a, starts)]
    lens = [int(min(B, n - s)) for s in starts]
    return E, p, lens


def block_length(block_frames, sample_rate):
    return int(block_frames) if block_frames else 3 * int(sample_rate)


def want_plane(x, B, permille) -> dict:
    s2 = SCALE[x.dtype] ** 2
    q, nonfinite = quantise(x)
    E, p, lens = block_energies(q, B)
    blocks = len(E)
    w = {"top_ms": 0.0, "mean_square": 0.0, "peak": 0, "peak2": 0, "blocks": blocks, "top_blocks": 0, "nonfinite": nonfinite}
    if not blocks:
        return w
    e = [float(v) for v in E]                                   # int -> float rounds once, to nearest even
    ms = [2.0 * ei / (float(ni) * s2) for ei, ni in zip(e, lens)]
    k = max(1, blocks * permille // 1000)
    t = sorted(ms, reverse=True)[k - 1]
    S, g = 0.0, 0
    for v in ms:
        if v > t:
            S += v
            g += 1
    for _ in range(k - g):
        S += t
    esum = 0.0
    for v in e:
        esum += v
    ps = sorted(p, reverse=True)
    w.update(top_ms=S / k, mean_square=2.0 * esum / (float(len(x)) * s2), peak=ps[0], peak2=ps[1] if blocks > 1 else ps[0], top_blocks=k)
    return w


def _db(factor, x):
    return factor * math.log10(x) if x > 0.0 else -math.inf


def want_track(tr, block_frames=None, top_permille=None) -> dict:
    permille = 200 if top_permille is None else top_permille
    B = block_length(block_frames, tr.sample_rate)
    dt = np.dtype(tr.channels[0].dtype)
    s = SCALE[dt]
    n = len(tr.channels[0])
    chans, flags, sounding = [], _capi.DR_COMPLETE, False
    for x in tr.channels:
        w = want_plane(x, B, permille)
        has = w["peak2"] > 0 and w["top_ms"] > 0.0
        w["dr"] = 20.0 * math.log10((w["peak2"] / s) / math.sqrt(w["top_ms"])) if has else 0.0
        w["peak_db"] = _db(20.0, w["peak"] / s)
        w["rms_db"] = _db(10.0, w["mean_square"])
        sounding = sounding or has
        if w["nonfinite"]:
            flags |= _capi.DR_NONFINITE
        chans.append(w)
    if not sounding or n == 0:
        flags |= _capi.DR_SILENT
    if n < B:
        flags |= _capi.DR_SHORT
    dr_mean = sum(c["dr"] for c in chans) / len(chans)
    return {"status": 0, "flags": flags, "frames": n, "sample_rate": tr.sample_rate, "channels": len(chans), "format": FMT[dt],
            "dropped_frames": 0, "block_frames": B, "dr": int(round(dr_mean)), "dr_mean": dr_mean,
            "peak_db": max(c["peak_db"] for c in chans), "rms_db": _db(10.0, sum(c["mean_square"] for c in chans) / len(chans)), "ch": chans}


def got(r) -> dict:
    """An rg_dr_result as want_track's dict."""
    d = {f: getattr(r, f) for f in TRACK_FIELDS + TRACK_DB_FIELDS}
    d["ch"] = [{f: getattr(r.ch[c], f) for f in RAW_FIELDS + DB_FIELDS} for c in range(int(r.channels))]
    return d


def _close(a, b):
    return a == b or (math.isfinite(a) and math.isfinite(b) and abs(a - b) <= DB_RTOL * max(abs(a), abs(b)))


def differences(g, w) -> list:
    """The fields in which two such dicts differ: exactly everywhere in front of the logarithms, DB_RTOL behind them."""
    bad = [(f, g[f], w[f]) for f in TRACK_FIELDS if g[f] != w[f]]
    bad += [(f, g[f], w[f]) for f in TRACK_DB_FIELDS if not _close(g[f], w[f])]
    if len(g["ch"]) != len(w["ch"]):
        return bad + [("ch", len(g["ch"]), len(w["ch"]))]
    for c, (x, y) in enumerate(zip(g["ch"], w["ch"])):
        bad += [(f"ch{c}.{f}", x[f], y[f]) for f in RAW_FIELDS if x[f] != y[f]]
        bad += [(f"ch{c}.{f}", x[f], y[f]) for f in DB_FIELDS if not _close(x[f], y[f])]
    return bad


# ---- the cases ----------------------------------------------------------------------------------------------------------------
def _noise(rng, dtype, n):
    dtype = np.dtype(dtype)
    if dtype == np.float32:
        return (rng.standard_normal(n) * 0.3).astype(np.float32)
    info = np.iinfo(dtype)
    return rng.integers(info.min, info.max, size=n, endpoint=True, dtype=np.int64).astype(dtype)


def _loudest(dtype):
    dtype = np.dtype(dtype)
    return np.float32(-1.5) if dtype == np.float32 else np.iinfo(dtype).min


@lru_cache(maxsize=None)
def groups():
    """Every case, grouped by the options of its call."""
    rng = np.random.default_rng(0xD12)
    by_opts = {}

    def add(B, permille, tr, short=True):
        key = (B, permille)
        by_opts.setdefault(key, [[], True])
        by_opts[key][0].append(tr)
        by_opts[key][1] = by_opts[key][1] and short

    tags = {np.dtype(np.int16): "s16", np.dtype(np.int32): "s32", np.dtype(np.float32): "f32"}
    for fmt, dtype in DTYPES.items():
        C, T = shape(fmt)
        tag = tags[np.dtype(dtype)]
        # N x B on the kernels' boundaries, mono; a last block of one sample holds the plane's peak
        for N in (0, 1, C - 1, C, C + 1, T - 1, T, T + 1, 2 * T + 3):
            for B in sorted({1, 7, C, T, T + 1, N, N + 1} - {0}):
                x = _noise(rng, dtype, N)
                if N > 1 and N % B == 1:
                    x[:-1] = x[:-1] // 2 if dtype != np.float32 else x[:-1] * np.float32(0.5)
                    x[-1] = _loudest(dtype)
                add(B, None, Tr(f"{tag}_n{N}_b{B}", [x], 44100))
        # 2, 6 and 8 channels
        for ch in (2, 6, 8):
            for N, B in ((T + 1, 7), (2 * T + 3, T), (C + 1, C)):
                add(B, None, Tr(f"{tag}_{ch}ch_n{N}_b{B}", [_noise(rng, dtype, N) for _ in range(ch)], 48000))
        # blocks in {1, 4, 5, 9, 10}: k = 1, 1, 1, 1, 2 at 200 per mille; 1 and 1000 per mille
        for blocks in (1, 4, 5, 9, 10):
            for permille in (None, 1, 1000):
                add(7, permille, Tr(f"{tag}_blocks{blocks}", [_noise(rng, dtype, 7 * blocks - 3)], 44100))
        # ties: all blocks equal; energies [5, 3, 3, 3, 1] with k = 2 (400 per mille of 5 blocks): one of three equal blocks is taken
        one = np.float32(2.0 ** -23) if dtype == np.float32 else 1
        flat = np.tile(np.array([3, -3, 3, -3, 3], dtype=np.int64), 6)
        ladder = np.concatenate([np.array([1] * c + [0] * (5 - c), dtype=np.int64) for c in (5, 3, 3, 3, 1)])
        for permille in (None, 400, 1000):
            add(5, permille, Tr(f"{tag}_all_equal", [(flat * one).astype(dtype)], 44100))
            add(5, permille, Tr(f"{tag}_ladder", [(ladder * one).astype(dtype), (ladder[::-1] * one).astype(dtype)], 44100))
        # more blocks than one pass of the selection holds counters for, whatever the seam reports
        add(3, None, Tr(f"{tag}_many_blocks", [_noise(rng, dtype, 50000), _noise(rng, dtype, 50000) // 3 if dtype != np.float32 else _noise(rng, dtype, 50000)], 44100))
        # peaks: the maximum in two blocks, then in one; one block only
        v = (np.array([9, 1, 0, 0, 0, 0, 0, 1, -9, 0, 0, 0, 0, 0, 3, 0, 0, 0, 0, 0, 0], dtype=np.int64) * one).astype(dtype)
        u = (np.array([9, 1, 0, 0, 0, 0, 0, 1, -3, 0, 0, 0, 0, 0, 5, 0, 0, 0, 0, 0, 0], dtype=np.int64) * one).astype(dtype)
        add(7, None, Tr(f"{tag}_peak_twice", [v], 44100))
        add(7, None, Tr(f"{tag}_peak_once", [u], 44100))
        add(7, None, Tr(f"{tag}_one_block", [u[:5].copy()], 44100))
        add(7, None, Tr(f"{tag}_zeros", [np.zeros(20, dtype), np.zeros(20, dtype)], 44100))
    C32, T32 = shape(_capi.FMT_S32_PLANAR)
    C16, T16 = shape(_capi.FMT_S16_PLANAR)
    # limbs: 8 * 2^62 is the first sum past 2^64; low limbs that carry; the longest block there is
    mn = np.iinfo(np.int32).min
    add(8, None, Tr("s32_int_min_blocks_of_8", [np.full(24, mn, np.int32)], 44100))
    carry = np.empty(T32 + 1, np.int32)
    carry[0::2] = 0x0001FFFF
    carry[1::2] = 0x7FFFFFFF
    add(T32, None, Tr("s32_low_limbs_carry", [carry], 44100))
    add(T32, None, Tr("f32_low_limbs_carry", [(carry[:T32 + 1] >> 8).astype(np.float32) / np.float32(2.0 ** 23) * np.float32(255.0)], 44100))
    add(MAX_BLOCK, None, Tr("s32_int_min_longest_block", [np.full(MAX_BLOCK + 5, mn, np.int32)], 44100), short=False)
    add(MAX_BLOCK, None, Tr("s16_short_clip", [_noise(rng, np.int16, 1000)], 44100), short=False)
    add(MAX_BLOCK, None, Tr("f32_short_clip", [_noise(rng, np.float32, 1000)], 44100), short=False)
    add(7, None, Tr("s16_minus_full_scale_alone", [np.array([-32768], np.int16)], 44100))
    # floats: +-256 and beyond (q = +-2^31), non-finite samples in the first, a middle and the last block, a plane of NaN, -0.0
    # and subnormals, x * 2^23 at exact halves, values beyond +-1
    f = np.float32
    add(7, None, Tr("f32_at_256_and_beyond", [np.array([256.0, -256.0, 300.0, -1e30, 255.99998, -255.99998, 1e-3, 3.4e38, -3.4e38], f)], 44100))
    nf = _noise(rng, np.float32, 35)
    nf[[0, 17, 34]] = [np.nan, np.inf, -np.inf]
    add(7, None, Tr("f32_nonfinite_first_middle_last", [nf, _noise(rng, np.float32, 35)], 44100))
    add(7, None, Tr("f32_all_nan", [np.full(30, np.nan, f)], 44100))
    add(7, None, Tr("f32_all_nan_and_sound", [np.full(30, np.nan, f), _noise(rng, np.float32, 30)], 44100))
    add(7, None, Tr("f32_zeros_and_subnormals", [np.array([-0.0, 0.0, 1e-45, -1e-45, 1e-39, -1.1754942e-38, 1.1754944e-38] * 3, f)], 44100))
    h = 2.0 ** -24
    add(7, None, Tr("f32_exact_halves", [np.array([h, 3 * h, -h, -3 * h, 5 * h, 7 * h, 0.5 * h, 1.5 * h, 2.5 * h, 1.0 + 2 * h, -1.25, 2.5, -7.75, 100.0], f)], 44100))
    # known values at 44.1 kHz, 16-bit, default options (see KNOWN)
    t = np.arange(10 * 44100)
    sine = np.rint(32767.0 * np.sin(2.0 * np.pi * 997.0 * t / 44100.0)).astype(np.int16)
    square = np.where((t // 22) % 2 == 0, 32767, -32767).astype(np.int16)
    t30 = np.arange(30 * 44100)
    quiet = np.rint(3276.7 * np.sin(2.0 * np.pi * 997.0 * t30 / 44100.0)).astype(np.int16)
    two, once = quiet.copy(), quiet.copy()
    two[[1000, 5 * 132300 + 77]] = 32767
    once[1000] = 32767
    for name, x in (("known_sine", sine), ("known_square", square), ("known_two_spikes", two), ("known_one_spike", once)):
        add(None, None, Tr(name, [x, x.copy()], 44100), short=False)
    return tuple(Group(f"b{B}_p{permille}", B, permille, tuple(trs), short) for (B, permille), (trs, short) in by_opts.items())


KNOWN = {"known_sine": 0.0, "known_square": -3.01, "known_two_spikes": 19.99, "known_one_spike": 0.0}  # dr_mean, each within KNOWN_TOL dB
KNOWN_TOL = 0.01


@lru_cache(maxsize=None)
def wants(name):
    """{track name: want_track} of one group, computed once and shared."""
    g = next(g for g in groups() if g.name == name)
    return {tr.name: want_track(tr, g.block_frames, g.top_permille) for tr in g.tracks}
