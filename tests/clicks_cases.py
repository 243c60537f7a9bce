"""The click scan (include/mp3rgain_amd_clicks.h) restated with Python integers and Python floats, and the cases the CPU and GPU
tests share.

The restatement is independent of the library's records and of its cutting: q is numpy arithmetic on the stored values, the
window and the autocorrelation are integers (int64 is wide enough: |xw| <= 2^15 and a block has at most 4096 samples), the
Levinson-Durbin recursion and the quantisation are Python floats (IEEE doubles) in the header's operation order, the residual is
an int64 expression over whole blocks, the median is a sort, and flagged samples become events in one plain loop.  The case list
takes the kernels' own boundary (the samples of a tile) from rg_clicks_kernel_shape.  A case is a group: the tracks that one call
scans with one set of options.  Not part of the product.

How the constructed cases work: in a plane that is zero but for isolated samples of value A, more than `order` apart, every
autocorrelation beyond lag 0 is zero, so every coefficient is zero, the quantisation fails and the block falls back to (2, -1):
the residual of such a sample is A, -2A, A at p, p + 1, p + 2, the medians are 0 and the scale is the floor.  With A large enough
exactly those three samples are flagged, and where the flagged samples lie is known to the sample."""
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

RECORD_FIELDS = ("status", "flags", "frames", "sample_rate", "channels", "format", "dropped_frames", "block_samples", "order", "ratio_permille",
                 "floor", "gap", "max_width", "max_events", "listed", "nonfinite", "events")
CHANNEL_FIELDS = ("flagged", "clicks", "bursts", "widest", "first_click", "strongest_at", "strongest_permille", "fallback_blocks", "median_max")
EVENT_FIELDS = ("start", "width", "peak_at", "strength_permille", "channel", "kind")

Tr = namedtuple("Tr", "name channels sample_rate")  # .channels: planes of one dtype and length (tests/arena_layouts.pack takes these)
Opts = namedtuple("Opts", "block_samples order ratio_permille floor gap max_width max_events",
                  defaults=(_capi.CK_DEFAULT_BLOCK, _capi.CK_DEFAULT_ORDER, _capi.CK_DEFAULT_RATIO_PERMILLE, _capi.CK_DEFAULT_FLOOR, _capi.CK_DEFAULT_GAP,
                            _capi.CK_DEFAULT_MAX_WIDTH, _capi.CK_DEFAULT_MAX_EVENTS))
Group = namedtuple("Group", "name opts tracks")

DTYPES = {_capi.FMT_F32_PLANAR: np.float32, _capi.FMT_S16_PLANAR: np.int16, _capi.FMT_S32_PLANAR: np.int32}
FMT = {np.dtype(v): k for k, v in DTYPES.items()}
TAGS = {np.dtype(np.int16): "s16", np.dtype(np.int32): "s32", np.dtype(np.float32): "f32"}


def tile_samples(block):
    from mp3rgain_amd import clicks_kernel_shape

    return clicks_kernel_shape(block)[0]


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


FALLBACK = ([2, -1], 0)


def model(qb, P):
    """(coefficients, shift) of a block's q (int64 array), and whether it fell back."""
    n = len(qb)
    if n < 4 * P:
        return FALLBACK, True
    N = n - 1
    d = 2 * np.arange(n, dtype=np.int64) - N
    w = (32767 * (N * N - d * d)) // (N * N)
    xw = (qb * w) >> 15
    acf = [int(np.dot(xw[l:], xw[:n - l])) for l in range(P + 1)]
    if acf[0] <= 0:
        return FALLBACK, True
    lp, err = [0.0] * P, float(acf[0])
    for i in range(P):
        acc = float(acf[i + 1])
        for j in range(i):
            acc = acc - lp[j] * float(acf[i - j])
        k = acc / err
        tmp = [lp[j] - k * lp[i - 1 - j] for j in range(i)]
        lp[:i] = tmp
        lp[i] = k
        err = err * (1.0 - k * k)
        if not err > 0.0 and i + 1 < P:
            return FALLBACK, True
    if not all(math.isfinite(c) for c in lp):
        return FALLBACK, True
    top = max(abs(c) for c in lp)
    if top < 2.0 ** -1022:  # zero or subnormal
        return FALLBACK, True
    shift = min(12 - 1 - math.frexp(top)[1], 15)
    if shift < 0:
        return FALLBACK, True
    scale, hi, e, qc = float(1 << shift), (1 << 11) - 1, 0.0, []
    for c in lp:
        e = e + c * scale
        v = int(e + 0.5) if e >= 0.0 else -int(0.5 - e)
        v = max(-hi - 1, min(hi, v))
        e = e - float(v)
        qc.append(v)
    return (qc, shift), False


def plane(x, o):
    """One plane -> a dict of its channel fields, its non-finite count, whether any q is not 0, and all its events."""
    q, nonfinite = quantise(x)
    N, B, P = len(q), o.block_samples, o.order
    e = np.zeros(N, np.int64)
    med, fallback = [], 0
    for at in range(0, N, B):
        n = min(B, N - at)
        (c, shift), fell = model(q[at:at + n], P)
        fallback += fell
        lo = max(at, len(c))  # r[n] = 0 below the order in use
        if lo < at + n:
            s = np.zeros(at + n - lo, np.int64)
            for j, cj in enumerate(c):
                s += cj * q[lo - 1 - j:at + n - 1 - j]
            e[lo:at + n] = np.abs(q[lo:at + n] - (s >> shift))
        med.append(int(np.sort(e[at:at + n])[(n - 1) // 2]))
    events, flagged = [], 0
    if N:
        S = np.array([max([o.floor] + med[max(0, b - 1):b + 2]) for b in range(len(med))], np.int64)
        Sn = np.repeat(S, B)[:N]
        for n in np.nonzero(1000 * e > o.ratio_permille * Sn)[0]:
            n, s = int(n), min(1000 * int(e[n]) // int(Sn[n]), 2 ** 32 - 1)
            flagged += 1
            if events and n - events[-1]["last"] <= o.gap:
                ev = events[-1]
                ev["last"] = n
                if s > ev["strength"]:
                    ev["strength"], ev["peak_at"] = s, n
            else:
                events.append({"start": n, "last": n, "strength": s, "peak_at": n})
    for ev in events:
        ev["width"] = ev["last"] - ev["start"] + 1
        ev["kind"] = _capi.CK_KIND_CLICK if ev["width"] <= o.max_width else _capi.CK_KIND_BURST
    clicks = [ev for ev in events if ev["kind"] == _capi.CK_KIND_CLICK]
    strongest = max(clicks, key=lambda ev: (ev["strength"], -ev["peak_at"])) if clicks else None
    ch = dict(flagged=flagged, clicks=len(clicks), bursts=len(events) - len(clicks), widest=max([ev["width"] for ev in events] + [0]),
              first_click=clicks[0]["start"] if clicks else N, strongest_at=strongest["peak_at"] if clicks else N,
              strongest_permille=strongest["strength"] if clicks else 0, fallback_blocks=fallback, median_max=max(med + [0]))
    return ch, nonfinite, bool(np.any(q != 0)), events


def want_track(tr, o) -> dict:
    dt = np.dtype(tr.channels[0].dtype)
    n = len(tr.channels[0])
    w = dict(status=0, frames=n, sample_rate=tr.sample_rate, channels=len(tr.channels), format=FMT[dt], dropped_frames=0, **o._asdict())
    chans, listed, nonfinite, nonzero, total = [], [], 0, False, 0
    for c, x in enumerate(tr.channels):
        ch, nf, nz, events = plane(x, o)
        chans.append(ch)
        nonfinite, nonzero, total = nonfinite + nf, nonzero or nz, total + len(events)
        listed += [dict(start=ev["start"], width=ev["width"], peak_at=ev["peak_at"], strength_permille=ev["strength"], channel=c, kind=ev["kind"]) for ev in events]
    listed.sort(key=lambda ev: (ev["start"], ev["channel"]))
    flags = _capi.CK_COMPLETE
    flags |= 0 if nonzero else _capi.CK_SILENT
    flags |= _capi.CK_NONFINITE if nonfinite else 0
    flags |= _capi.CK_CLICKS if any(ch["clicks"] for ch in chans) else 0
    flags |= _capi.CK_BURSTS if any(ch["bursts"] for ch in chans) else 0
    flags |= _capi.CK_TRUNCATED if total > o.max_events else 0
    w.update(flags=flags, nonfinite=nonfinite, events=total, listed=min(total, o.max_events), ch=chans, list=listed[:o.max_events])
    return w


def got(r, row) -> dict:
    """An rg_clicks_result and its row of the event list as want_track's dict."""
    g = {f: getattr(r, f) for f in RECORD_FIELDS}
    g["ch"] = [{f: getattr(r.ch[c], f) for f in CHANNEL_FIELDS} for c in range(r.channels)]
    g["list"] = [{f: getattr(ev, f) for f in EVENT_FIELDS} for ev in row[:r.listed]]
    g["unused"] = [k for k, ev in enumerate(row) if k >= r.listed and bytes(ev) != bytes(len(bytes(ev)))]
    g["beyond"] = [c for c in range(r.channels, _capi.CK_MAX_CHANNELS) if bytes(r.ch[c]) != bytes(len(bytes(r.ch[c])))]
    return g


def differences(g, w) -> list:
    """The fields in which a record read by got() differs from want_track's."""
    d = [(f, g[f], w[f]) for f in RECORD_FIELDS if g[f] != w[f]]
    d += [("ch", c, f, a[f], b[f]) for c, (a, b) in enumerate(zip(g["ch"], w["ch"])) for f in CHANNEL_FIELDS if a[f] != b[f]]
    d += [("list", k, a, b) for k, (a, b) in enumerate(zip(g["list"], w["list"])) if a != b]
    if len(g["list"]) != len(w["list"]):
        d.append(("listed", len(g["list"]), len(w["list"])))
    if g["unused"] or g["beyond"]:
        d.append(("not zero", g["unused"], g["beyond"]))
    return d


# ---- the cases ----------------------------------------------------------------------------------------------------------------
def _noise(rng, dtype, n):
    dtype = np.dtype(dtype)
    if dtype == np.float32:
        return (rng.standard_normal(n) * 0.4).astype(np.float32)  # a sample in a hundred beyond full scale
    info = np.iinfo(dtype)
    return rng.integers(info.min, info.max, size=n, endpoint=True, dtype=np.int64).astype(dtype)


def scaled(v, dtype):
    """Integers as samples of a format whose q they are."""
    dtype = np.dtype(dtype)
    v = np.asarray(v, dtype=np.int64)
    if dtype == np.float32:
        return (v / 32768.0).astype(np.float32)
    return (v << 16).astype(np.int32) if dtype == np.int32 else v.astype(np.int16)


def tonal(rng, n, level=6000, floor=4.0):
    """q of a three-tone mix over a small noise floor: blocks with a model of their own."""
    t = np.arange(n)
    x = level * (np.sin(t * 0.031) + 0.5 * np.sin(t * 0.173 + 1.0) + 0.25 * np.sin(t * 0.411 + 2.0)) + rng.normal(0.0, floor, n)
    return np.rint(x).astype(np.int64)


def spikes(n, at, a=20000):
    """q that is zero but for the value `a` at the places `at` (see the module docstring)."""
    v = np.zeros(n, np.int64)
    v[list(at)] = a
    return v


@lru_cache(maxsize=None)
def groups():
    """Every case, grouped by the options of its call."""
    rng = np.random.default_rng(0xC11C)
    by_opts = {}

    def add(o, tr):
        by_opts.setdefault(o, []).append(tr)

    dflt = Opts()
    small, big = Opts(block_samples=256, order=2), Opts(block_samples=4096, order=12)
    wide = Opts(block_samples=4096, order=12, gap=255, max_width=4095)   # an event may span a tile
    none = Opts(max_events=0)
    few = Opts(max_events=3)
    for fmt, dtype in DTYPES.items():
        tag = TAGS[np.dtype(dtype)]
        for o in (dflt, small, big):
            B, P, T, g = o.block_samples, o.order, tile_samples(o.block_samples), o.gap
            lengths = {0, 1, P - 1, P, P + 1, 4 * P - 1, 4 * P, B - 1, B, B + 1, 2 * B + 1, 3 * B, B + 4 * P - 1}
            if o is big:  # the tile's seams, at the block length whose tile is the shortest
                lengths |= {T - 1, T, T + 1, 2 * T + 1}
            for N in sorted(lengths):
                add(o, Tr(f"{tag}_noise_n{N}", [_noise(rng, dtype, N)], 44100))
                if N <= B + 1:
                    add(o, Tr(f"{tag}_tonal_n{N}", [scaled(tonal(rng, N), dtype), scaled(tonal(rng, N), dtype)], 48000))
            # music, silence, music: blocks of zeros fall back and their scale is the floor; a constant; the largest residuals
            m = tonal(rng, 5 * B + 77)
            m[B + 100:3 * B + 50] = 0
            m[4 * B + 10] += 9000  # and a click in the music behind the silence
            add(o, Tr(f"{tag}_zeros_between_music", [scaled(m, dtype)], 44100))
            add(o, Tr(f"{tag}_constant", [scaled(np.full(2 * B + 9, 1000), dtype)], 44100))
            alt = np.where(np.arange(2 * B + 3) % 2 == 0, -32768, 32767)
            add(o, Tr(f"{tag}_alternating_full_scale", [scaled(alt, dtype), scaled(-1 - alt, dtype)], 44100))
            # flagged samples exactly `gap` and `gap` + 1 apart: inside a block and across a block cut (at 4096 also a tile cut)
            for where, p in (("block", 300), ("cut", B - 3)):
                for extra in (0, 1):
                    add(o, Tr(f"{tag}_gap{'+1' if extra else ''}_{where}", [scaled(spikes(p + 3 * B, [p, p + 2 + g + extra]), dtype)], 44100))
            # a click in tonal material on eight channels, the same sample in some of them (the list's order), and one channel clean
            chans = []
            for c in range(8):
                v = tonal(rng, B + 500)
                if c != 3:
                    v[700 + (c // 3)] += 12000
                chans.append(scaled(np.clip(v, -32768, 32767), dtype))
            add(o, Tr(f"{tag}_eight_channels", chans, 96000))
        # widths: max_width and max_width + 1 (chains of spikes 15 apart at most: inside the gap, outside the order)
        add(dflt, Tr(f"{tag}_width32", [scaled(spikes(3000, [1000, 1015, 1029]), dtype)], 44100))
        add(dflt, Tr(f"{tag}_width33", [scaled(spikes(3000, [1000, 1015, 1030]), dtype)], 44100))
        # exactly K events, K + 1, and both with K = 0 and K = 3
        for o in (dflt, none, few):
            for k in (16, 17):
                add(o, Tr(f"{tag}_events{k}", [scaled(spikes(2500, [100 + 130 * j for j in range(k)]), dtype), scaled(spikes(2500, [165]), dtype)], 44100))
        # an event that spans a whole tile, from the tile before into the tile behind
        T = tile_samples(4096)
        add(wide, Tr(f"{tag}_spans_a_tile", [scaled(spikes(3 * T + 5, range(T - 400, 2 * T + 300, 200)), dtype), scaled(spikes(3 * T + 5, [T - 1, T + 250]), dtype)], 44100))
        add(wide, Tr(f"{tag}_tile_cut_gap", [scaled(spikes(2 * T + 9, [T - 3, T + 254]), dtype), scaled(spikes(2 * T + 9, [T - 3, T + 255]), dtype)], 44100))
    # a FILE whose events are exactly K (15 and 1), and one more: not truncated with every slot filled, then truncated
    for k in (15, 16):
        add(dflt, Tr(f"s16_file_events{k + 1}", [scaled(spikes(2500, [100 + 130 * j for j in range(k)]), np.int16), scaled(spikes(2500, [2300]), np.int16)], 44100))
    # cuts between tiles of more than one block, at the shortest lengths that have one (16-bit only: they are long)
    for o in (dflt, small):
        T = tile_samples(o.block_samples)
        v = tonal(rng, T + o.block_samples + 1)
        v[T - 1] += 15000
        v[T + 3] -= 15000
        add(o, Tr("s16_two_tiles", [scaled(np.clip(v, -32768, 32767), np.int16), scaled(spikes(len(v), [T - 3, T + 2 + o.gap, T + 40]), np.int16)], 44100))
    # non-finite floats
    f = np.float32
    for where, k in (("first", 0), ("middle", 600), ("last", 1299)):
        a, b = scaled(tonal(rng, 1300), f), scaled(tonal(rng, 1300), f)
        a[k] = np.nan
        b[k] = np.inf if k else -np.inf
        add(dflt, Tr(f"f32_nonfinite_{where}", [a, b], 44100))
    add(dflt, Tr("f32_all_nan", [np.full(300, np.nan, f)], 44100))
    add(dflt, Tr("f32_beyond_full_scale", [np.array([1.5, -1.5, 1e30, -1e30, 1.0, -1.0, 32767.5 / 32768.0] * 40, f)], 44100))
    add(dflt, Tr("s32_low_bits", [(scaled(tonal(rng, 1100), np.int32) | 0xFFFF).astype(np.int32)], 44100))
    return tuple(Group("b{}_p{}_r{}_f{}_g{}_w{}_k{}".format(*o), o, tuple(trs)) for o, trs in by_opts.items())


@lru_cache(maxsize=None)
def wants(name):
    """{track name: want_track} of one group, computed once and shared."""
    g = next(g for g in groups() if g.name == name)
    return {tr.name: want_track(tr, g.opts) for tr in g.tracks}
