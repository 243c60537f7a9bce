"""The rip checksums (include/mp3rgain_amd_rip.h) restated in Python, and the cases the CPU and GPU tests share.

The restatement is independent of the library: zlib.crc32 over the interleaved bytes and over the non-zero samples' bytes, the
AccurateRip sums in numpy uint64, and a plain Python loop used below 10 000 frames.  The case list takes the kernels' own
boundaries (chunk, tile, fold lanes) from rg_rip_kernel_shape.  Not part of the product."""
import sys
import zlib
from collections import namedtuple
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

from mp3rgain_amd import _capi  # noqa: E402

FIRST, LAST = _capi.RIP_FIRST_TRACK, _capi.RIP_LAST_TRACK
ALL_FLAGS = (0, FIRST, LAST, FIRST | LAST)
SKIP = 2940
LOOP_BELOW = 10000

Want = namedtuple("Want", "crc32 crc32_nonnull null_samples arv1 arv2")
Case = namedtuple("Case", "name left right")  # int16 planes of one length
Track = namedtuple("Track", "channels sample_rate")  # what tests/arena_layouts.pack takes


def ar_range(n, flags):
    """(from, to): position i (1-based) counts when from <= i <= to; `to` is signed and the range may be empty."""
    return (SKIP if flags & FIRST else 0), (n - SKIP if flags & LAST else n)


def ar_numpy(left, right, flags):
    n = len(left)
    lo, hi = ar_range(n, flags)
    v = left.astype(np.uint16).astype(np.uint64) | (right.astype(np.uint16).astype(np.uint64) << np.uint64(16))
    i = np.arange(1, n + 1, dtype=np.uint64)
    take = (i >= np.uint64(lo)) & (i.astype(np.int64) <= hi)
    p = (v * i)[take]  # < 2^64: v < 2^32, i < 2^32
    s_lo = int((p & np.uint64(0xFFFFFFFF)).sum(dtype=np.uint64)) & 0xFFFFFFFF  # a uint64 sum of 32-bit terms wraps at 2^64: harmless mod 2^32
    s_hi = int((p >> np.uint64(32)).sum(dtype=np.uint64)) & 0xFFFFFFFF
    return s_lo, (s_lo + s_hi) & 0xFFFFFFFF


def ar_loop(left, right, flags):
    n = len(left)
    lo, hi = ar_range(n, flags)
    v1 = v2 = 0
    for k in range(n):
        i = k + 1
        if lo <= i <= hi:
            p = ((int(left[k]) & 0xFFFF) | ((int(right[k]) & 0xFFFF) << 16)) * i
            v1 = (v1 + (p & 0xFFFFFFFF)) & 0xFFFFFFFF
            v2 = (v2 + (p & 0xFFFFFFFF) + (p >> 32)) & 0xFFFFFFFF
    return v1, v2


def want(left, right, flags) -> Want:
    left = np.ascontiguousarray(left, dtype="<i2")
    right = np.ascontiguousarray(right, dtype="<i2")
    inter = np.empty(2 * len(left), dtype="<i2")
    inter[0::2] = left
    inter[1::2] = right
    nonnull = inter[inter != 0]
    v1, v2 = ar_numpy(left, right, flags)
    if len(left) < LOOP_BELOW:
        assert (v1, v2) == ar_loop(left, right, flags)
    return Want(zlib.crc32(inter.tobytes()) if len(inter) else 0, zlib.crc32(nonnull.tobytes()) if len(nonnull) else 0,
                int(len(inter) - len(nonnull)), v1, v2)


def got(rec) -> Want:
    """The same five numbers of an rg_rip_result."""
    return Want(int(rec.crc32), int(rec.crc32_nonnull), int(rec.null_samples), int(rec.arv1), int(rec.arv2))


def shape():
    from mp3rgain_amd import replaygain

    return replaygain.rip_kernel_shape()


def lengths():
    c, t, f = shape()
    return [0, 1, 2, c - 1, c, c + 1, t - 1, t, t + 1, 2 * t + 1, 3 * t + c + 1, 2939, 2940, 2941, 5879, 5880, 5881, f * t + t + 1]


def _planes(kind, n, rng):
    if kind == "random":
        return rng.integers(-32768, 32768, n, dtype=np.int16), rng.integers(-32768, 32768, n, dtype=np.int16)
    if kind == "zero":
        return np.zeros(n, np.int16), np.zeros(n, np.int16)
    if kind == "ffff":  # every sample 0xFFFF: the largest v, the largest hi32 carries
        return np.full(n, -1, np.int16), np.full(n, -1, np.int16)
    if kind == "min":
        return np.full(n, -32768, np.int16), np.full(n, -32768, np.int16)
    if kind == "sparse":  # about 30 % zeros, drawn per sample and not per frame
        l, r = _planes("random", n, rng)
        l[rng.random(n) < 0.3] = 0
        r[rng.random(n) < 0.3] = 0
        return l, r
    if kind == "zero_left":
        return np.zeros(n, np.int16), _planes("random", n, rng)[1]
    if kind == "one_at_start":
        l, r = _planes("zero", n, rng)
        if n:
            l[0] = 0x1234
        return l, r
    if kind == "one_at_end":
        l, r = _planes("zero", n, rng)
        if n:
            r[-1] = -2
        return l, r
    raise ValueError(kind)


KINDS = ("random", "zero", "ffff", "min", "sparse", "zero_left", "one_at_start", "one_at_end")
_cache = {}


def cases():
    """Every length with every content (the longest one, which is there for the fold kernel's runs, with two).  Built once."""
    if "cases" not in _cache:
        rng = np.random.default_rng(0x52495043)
        longest = max(lengths())
        out = []
        for kind in KINDS:
            for n in lengths():
                if n == longest and kind not in ("random", "sparse"):
                    continue
                out.append(Case(f"{kind}_{n}", *_planes(kind, n, rng)))
        _cache["cases"] = out
    return _cache["cases"]


def wants():
    """{(case name, flags): Want}, computed once and shared."""
    if "wants" not in _cache:
        _cache["wants"] = {(cs.name, fl): want(cs.left, cs.right, fl) for cs in cases() for fl in ALL_FLAGS}
    return _cache["wants"]


def tracks(case_list):
    return [Track([cs.left, cs.right], 44100) for cs in case_list]
