"""The PCM defect scan (include/mp3rgain_amd_stats.h) restated in numpy, and the cases the CPU and GPU tests share.

The restatement is independent of the library and of its part records: a class array per plane, np.diff to find where the class
changes, and the stretches read off the change points.  The case list takes the kernels' own boundaries (chunk, tile, fold
lanes) from rg_pcm_stats_kernel_shape.  Not part of the product."""
import sys
from collections import namedtuple
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

from mp3rgain_amd import _capi  # noqa: E402

OPTIONS = ((1, 1), (3, 64), (1000, 5000))  # (min_clip_run, min_zero_run); the middle one is the header's default
CHANNEL_FIELDS = ("min", "max", "sum", "or_mask", "effective_bits", "clipped", "clip_runs", "longest_clip_run", "first_clip_run", "zeros",
                  "lead_zeros", "trail_zeros", "zero_runs", "longest_zero_run", "nonfinite")
TRACK_FIELDS = ("status", "flags", "frames", "sample_rate", "channels", "format", "bits", "dropped_frames", "lead_silence_frames",
                "trail_silence_frames")

Tr = namedtuple("Tr", "name channels sample_rate bits")  # .channels: planes of one dtype and length (tests/arena_layouts.pack takes these)


# ---- the definitions ----------------------------------------------------------------------------------------------------------
def width(dtype):
    return 16 if np.dtype(dtype) == np.int16 else 32


def full_scale(dtype, bits):
    """(P, M) of an integer container, or (1.0, -1.0)."""
    if np.dtype(dtype) == np.float32:
        return np.float32(1.0), np.float32(-1.0)
    w = width(dtype)
    return ((1 << (bits - 1)) - 1) << (w - bits), -(1 << (w - 1))


def classes(x, bits):
    """-> (class int8 array, zero bool array, finite bool array)."""
    cls = np.zeros(len(x), np.int8)
    if x.dtype == np.float32:
        finite = np.isfinite(x)
        with np.errstate(invalid="ignore"):
            cls[finite & (x >= 1.0)] = 1
            cls[finite & (x <= -1.0)] = -1
            zero = x == 0.0
        return cls, zero, finite
    p, m = full_scale(x.dtype, bits)
    v = x.astype(np.int64)
    cls[v >= p] = 1
    cls[v <= m] = -1
    return cls, v == 0, np.ones(len(x), bool)


def stretches(cls):
    """Maximal runs of one non-zero class -> (starts, ends), ends exclusive."""
    n = len(cls)
    if n == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    change = np.flatnonzero(np.diff(cls.astype(np.int16)) != 0) + 1
    starts = np.concatenate(([0], change))
    ends = np.concatenate((change, [n]))
    keep = cls[starts] != 0
    return starts[keep], ends[keep]


def want_plane(x, bits, min_clip, min_zero) -> dict:
    n = len(x)
    cls, zero, finite = classes(x, bits)
    w = {}
    took = x[finite]
    w["min"] = float(took.min()) if len(took) else 0.0
    w["max"] = float(took.max()) if len(took) else 0.0
    if x.dtype == np.float32:
        q = np.rint(np.clip(took.astype(np.float64), -256.0, 256.0) * float(1 << 23))  # exact products; rint is half to even
        w["sum"] = int(q.astype(np.int64).sum())
        w["or_mask"] = 0
    else:
        w["sum"] = int(x.astype(np.int64).sum())
        w["or_mask"] = int(np.bitwise_or.reduce(x.view(np.uint16 if x.dtype == np.int16 else np.uint32).astype(np.uint64))) if n else 0
    m = w["or_mask"]
    w["effective_bits"] = width(x.dtype) - ((m & -m).bit_length() - 1) if m else 0
    w["clipped"] = int(np.count_nonzero(cls))
    s, e = stretches(cls)
    length = e - s
    counted = length >= min_clip
    w["clip_runs"] = int(np.count_nonzero(counted))
    w["longest_clip_run"] = int(length.max()) if len(length) else 0
    w["first_clip_run"] = int(s[counted][0]) if counted.any() else n
    w["zeros"] = int(np.count_nonzero(zero))
    s, e = stretches(zero.astype(np.int8))
    length = e - s
    w["lead_zeros"] = int(length[0]) if len(s) and s[0] == 0 else 0
    w["trail_zeros"] = int(length[-1]) if len(s) and e[-1] == n else 0
    inner = length[(s > 0) & (e < n)]
    w["zero_runs"] = int(np.count_nonzero(inner >= min_zero))
    w["longest_zero_run"] = int(inner.max()) if len(inner) else 0
    w["nonfinite"] = int(np.count_nonzero(~finite))
    return w


def want_track(tr: Tr, min_clip, min_zero) -> dict:
    dt = tr.channels[0].dtype
    n = len(tr.channels[0])
    ch = [want_plane(p, tr.bits, min_clip, min_zero) for p in tr.channels]
    is_float = dt == np.float32
    bits = 0 if is_float else tr.bits
    flags = _capi.STATS_COMPLETE
    if any(c["clip_runs"] for c in ch):
        flags |= _capi.STATS_CLIPPED
    if any(c["zero_runs"] for c in ch):
        flags |= _capi.STATS_DROPOUT
    if not is_float and any(c["or_mask"] for c in ch) and max(c["effective_bits"] for c in ch) < bits:
        flags |= _capi.STATS_PADDED
    if any(c["nonfinite"] for c in ch):
        flags |= _capi.STATS_NONFINITE
    if all(c["zeros"] == n for c in ch):
        flags |= _capi.STATS_SILENT
    fmt = {np.dtype(np.float32): _capi.FMT_F32_PLANAR, np.dtype(np.int16): _capi.FMT_S16_PLANAR, np.dtype(np.int32): _capi.FMT_S32_PLANAR}[np.dtype(dt)]
    return {"status": 0, "flags": flags, "frames": n, "sample_rate": tr.sample_rate, "channels": len(ch), "format": fmt, "bits": bits,
            "dropped_frames": 0, "lead_silence_frames": min(c["lead_zeros"] for c in ch), "trail_silence_frames": min(c["trail_zeros"] for c in ch),
            "ch": ch}


def got(rec) -> dict:
    """The same fields of an rg_pcm_stats_result."""
    d = {f: int(getattr(rec, f)) for f in TRACK_FIELDS}
    d["ch"] = [{f: (float if f in ("min", "max") else int)(getattr(rec.ch[k], f)) for f in CHANNEL_FIELDS} for k in range(int(rec.channels))]
    return d


def differences(got_d, want_d):
    """[(field path, got, want)]; every comparison is ==."""
    bad = [(f, got_d[f], want_d[f]) for f in TRACK_FIELDS if got_d[f] != want_d[f]]
    for k, (g, w) in enumerate(zip(got_d["ch"], want_d["ch"])):
        bad += [(f"ch[{k}].{f}", g[f], w[f]) for f in CHANNEL_FIELDS if g[f] != w[f]]
    return bad


# ---- the cases ----------------------------------------------------------------------------------------------------------------
def shape():
    from mp3rgain_amd import replaygain

    return replaygain.pcm_stats_kernel_shape()


def lengths():
    c, t, f = shape()
    return [0, 1, c - 1, c, c + 1, t - 1, t, t + 1, 3 * t + c + 1]


def long_length():
    """One plane of 2F + 3 tiles (the last one short): the fold kernel's lanes take runs of 3 tile records."""
    c, t, f = shape()
    return (2 * f + 2) * t + c + 5


CONTAINERS = ((np.int16, (8, 12, 16)), (np.int32, (17, 20, 24, 32)), (np.float32, (32,)))
CONTENTS = ("random", "zero", "pos_fs", "clip_across", "zero_across", "clip_three", "zero_three", "pos_neg", "clip_lengths", "zero_lengths", "sparse")


def _quiet(n, dtype, bits, rng):
    """Samples that are neither zero nor full scale."""
    if np.dtype(dtype) == np.float32:
        x = rng.uniform(0.01, 0.9, n).astype(np.float32)
        return np.where(rng.random(n) < 0.5, x, -x).astype(np.float32)
    w = width(dtype)
    mag = rng.integers(1, (1 << (bits - 1)) - 1, n, dtype=np.int64)  # 1 .. 2^(b-1) - 2
    return (np.where(rng.random(n) < 0.5, mag, -mag) << (w - bits)).astype(dtype)


def _runs(x, at, lens, values):
    """Runs of lens[k] samples of values[k % len(values)] from `at` on, one quiet sample between them, as many as fit whole."""
    for k, ln in enumerate(lens):
        if at + ln + 1 > len(x):
            break
        x[at:at + ln] = values[k % len(values)]
        at += ln + 1
    return x


def _plane(kind, n, dtype, bits, rng):
    c, t, f = shape()
    pos, neg = full_scale(dtype, bits)
    if kind == "random":
        if np.dtype(dtype) == np.float32:
            return rng.uniform(-1.1, 1.1, n).astype(np.float32)
        return (rng.integers(-(1 << (bits - 1)), 1 << (bits - 1), n, dtype=np.int64) << (width(dtype) - bits)).astype(dtype)
    if kind == "zero":
        return np.zeros(n, dtype)
    if kind == "pos_fs":
        return np.full(n, pos, dtype)
    x = _quiet(n, dtype, bits, rng)
    bounds = [b for b in (c, 2 * c, t, 2 * t, 3 * t) if b < n]
    if kind in ("clip_across", "zero_across"):  # from the last sample of one chunk or tile to the first of the next
        for b in bounds:
            x[b - 1:b + 1] = pos if kind == "clip_across" else 0
    elif kind in ("clip_three", "zero_three"):  # three whole chunks (tiles) and one sample each side
        v = neg if kind == "clip_three" else 0
        if n >= 4 * c + 1:
            x[c - 1:4 * c + 1] = v
        if n >= 5 * t + 1:
            x[t - 1:4 * t + 1] = v
        elif n > 3 * t:  # what fits: from inside tile 0 through tiles 1 and 2 into the last one
            x[t - 1:3 * t + 1] = v
    elif kind == "pos_neg":  # +FS then -FS meeting exactly on a tile (chunk) boundary
        for b in bounds:
            x[max(0, b - 5):b] = pos
            x[b:b + 5] = neg
    elif kind == "clip_lengths":  # exactly min - 1 and min of every option set
        _runs(x, 1 if n > 1 else 0, (2, 3, 999, 1000, 3, 2), (pos, neg))
    elif kind == "zero_lengths":  # the same, between a zero stretch that touches the start and one that touches the end
        x[:min(n, 5)] = 0
        _runs(x, 7, (63, 64, 4999, 5000, 64, 63), (0,))
        if n > 20:
            x[-9:] = 0
    elif kind == "sparse":  # single full-scale samples
        hit = rng.random(n) < 0.02
        x[hit] = np.where(rng.random(int(hit.sum())) < 0.5, pos, neg).astype(dtype)
    else:
        raise ValueError(kind)
    return x


def f32_special(n, rng):
    """Quiet floats with every special value the definitions name, in runs and alone."""
    x = _quiet(n, np.float32, 32, rng)
    one = np.float32(1.0)
    special = [np.nan, np.inf, -np.inf, -0.0, 0.0, np.float32(1e-40), np.float32(-1e-42), 1.0, -1.0, np.nextafter(one, np.float32(0)),
               -np.nextafter(one, np.float32(0)), np.nextafter(one, np.float32(2)), 300.0, -300.0, 256.0, 0.5 / (1 << 23), 1.5 / (1 << 23), 2.5 / (1 << 23),
               -0.5 / (1 << 23), -1.5 / (1 << 23), 0.5 + 2.0 ** -24, 0.25 + 3 * 2.0 ** -24, -(0.5 + 3 * 2.0 ** -24)]
    at = 0
    for rep in (1, 3):  # alone, then in runs of 3 (a NaN between two +1.0 runs splits them; -0.0 next to 0.0 is one zero stretch)
        for v in special:
            if at + rep + 1 > n:
                return x
            x[at:at + rep] = v
            at += rep + 1
    for seq in ((1.0, 1.0, np.nan, 1.0, 1.0), (0.0, -0.0, 0.0), (-1.0, -300.0, -np.inf, -1.0)):
        if at + len(seq) + 1 > n:
            break
        x[at:at + len(seq)] = seq
        at += len(seq) + 1
    return x


_cache = {}


def tracks():
    """Every length with every content in every container, the bits cycling; the float specials; 16-bit audio in 24 bits; tracks
    of 2, 6 and 8 channels; three long planes.  Built once."""
    if "tracks" in _cache:
        return _cache["tracks"]
    rng = np.random.default_rng(0x50434D53)
    c, t, f = shape()
    out = []
    for dtype, bit_list in CONTAINERS:
        tag = np.dtype(dtype).name
        for li, n in enumerate(lengths()):
            for ki, kind in enumerate(CONTENTS):
                bits = bit_list[(li + ki) % len(bit_list)]
                out.append(Tr(f"{tag}_b{bits}_{kind}_{n}", [_plane(kind, n, dtype, bits, rng)], 44100, bits))
        for bits in bit_list:  # every width with the contents that depend on it, at one length
            for kind in ("random", "pos_neg", "sparse", "clip_lengths"):
                out.append(Tr(f"{tag}_b{bits}_{kind}_w", [_plane(kind, t + c + 3, dtype, bits, rng)], 48000, bits))
    for n in lengths():
        out.append(Tr(f"float32_special_{n}", [f32_special(n, rng)], 44100, 32))
    for n in (c + 1, t + 1):  # 16-bit audio in a 24-bit container: RG_STATS_PADDED
        pcm = rng.integers(-32768, 32768, n, dtype=np.int64)
        out.append(Tr(f"int32_b24_padded16_{n}", [(pcm << 16).astype(np.int32)], 44100, 24))
        out.append(Tr(f"int16_b16_padded8_{n}", [((pcm >> 8) << 8).astype(np.int16)], 44100, 16))
    for dtype, bits in ((np.int16, 16), (np.int32, 24), (np.float32, 32)):
        for nch in (2, 6, 8):
            for n in (c + 1, t + 1):
                kinds = [CONTENTS[(k * 3 + nch) % len(CONTENTS)] for k in range(nch)]
                planes = [_plane(k, n, dtype, bits, rng) for k in kinds]
                planes[0][:3] = 0  # edge silence in every channel, of different lengths
                planes[0][-2:] = 0
                for p in planes[1:]:
                    p[:4] = 0
                    p[-5:] = 0
                out.append(Tr(f"{np.dtype(dtype).name}_b{bits}_{nch}ch_{n}", planes, 48000, bits))
    big = long_length()
    out.append(Tr(f"int16_b16_random_{big}", [_plane("random", big, np.int16, 16, rng)], 44100, 16))
    out.append(Tr(f"int32_b24_sparse_{big}", [_plane("sparse", big, np.int32, 24, rng)], 44100, 24))
    out.append(Tr(f"float32_clip_three_{big}", [_plane("clip_three", big, np.float32, 32, rng)], 44100, 32))
    x = _plane("zero_three", big, np.int16, 12, rng)
    x[6 * t:] = 0  # and a zero stretch over the fold lanes' runs to the plane's end
    out.append(Tr(f"int16_b12_zero_three_{big}", [x], 44100, 12))
    _cache["tracks"] = out
    return out


def wants(opts):
    """{track name: want_track} for one option pair, computed once and shared."""
    key = ("wants", tuple(opts))
    if key not in _cache:
        _cache[key] = {tr.name: want_track(tr, *opts) for tr in tracks()}
    return _cache[key]


def bits_of(track_list):
    return [tr.bits for tr in track_list]
