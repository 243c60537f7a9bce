"""A test-side packer of PCM arenas: the layouts the C ABI allows and `replaygain.pack_tracks` never produces.

`pack_tracks` starts every track on a 16-byte boundary and pads with zeros, so a kernel that reads a sample from outside a
track reads a zero there, which changes no energy and no maximum.  Here a track may start at any sample-aligned residue
modulo 128 bytes, the tracks may abut, be stored back to front or share one copy, and what lies around them may be guard
samples that no result survives: +-1e30 / INT_MIN, INT_MAX, or NaN.  Not part of the product.

    arena, descs, guards = pack(tracks, Layout("guard", "loud", "input"))

`tracks` are `PcmTrack`-like objects (`.channels`: planar arrays of one dtype, `.sample_rate`); `descs[i]` describes
`tracks[i]` in every storage order.  `guards` lists the byte ranges [a, b) that hold guard samples."""
import sys
from collections import namedtuple
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

from mp3rgain_amd import _capi  # noqa: E402  (ctypes declarations only: nothing is loaded)

# gap: "abut" | "guard"; guard: "loud" | "nan" (ignored for abut); order: "input" | "reversed" | "aliased";
# shift: where in the residue cycle the first track of each format starts
Layout = namedtuple("Layout", "gap guard order shift", defaults=(0,))

GUARD_FRAMES = 64  # more than any loader's widest over-read: 16 bytes, a 16- or 32-frame tile, 24 frames of true-peak history
FMT = {np.dtype(np.float32): _capi.FMT_F32_PLANAR, np.dtype(np.int16): _capi.FMT_S16_PLANAR, np.dtype(np.int32): _capi.FMT_S32_PLANAR}


def residues(bps):
    """The residues of offset_bytes modulo 128 that the tracks of one format cycle through."""
    return [0, bps, 16 - bps, 16, 64 - bps, 64, 128 - bps]


def guard_samples(dtype, n, kind):
    """n guard samples of a track's format.  loud: alternating +-1e30 (finite through every f32 and f64 product the kernels
    form; +-FLT_MAX would overflow in the interpolator and be dropped as non-finite) or INT_MIN / INT_MAX.  nan: NaN for
    float tracks; integer formats have none and keep the loud guard."""
    dtype = np.dtype(dtype)
    if dtype == np.float32:
        if kind == "nan":
            return np.full(n, np.nan, dtype=np.float32)
        lo, hi = np.float32(-1e30), np.float32(1e30)
    else:
        lo, hi = np.iinfo(dtype).min, np.iinfo(dtype).max
    g = np.empty(n, dtype=dtype)
    g[0::2] = lo
    g[1::2] = hi
    return g


def _dtype(track):
    return np.dtype(track.channels[0].dtype)


def _nbytes(track):
    return sum(int(c.nbytes) for c in track.channels)


def pack(tracks, layout):
    """-> (uint8 arena, TrackDesc array, [(start, end)] guard byte ranges)."""
    n = len(tracks)
    # what is stored, in storage order: indices into `tracks`; `home[i]` = the stored track descriptor i points at
    home = list(range(n))
    if layout.order == "aliased":
        first = {}
        for i, t in enumerate(tracks):
            home[i] = first.setdefault(id(t), i)
    stored = [i for i in range(n) if home[i] == i]
    if layout.order == "reversed":
        stored.reverse()
    elif layout.order not in ("input", "aliased"):
        raise ValueError(layout.order)
    if layout.gap not in ("abut", "guard") or layout.guard not in ("loud", "nan"):
        raise ValueError(layout)

    # pass 1: offsets
    offset, guards, seen, cur = {}, [], {}, 0
    plan = []  # (track index, offset, first byte of the guard in front of it)
    for i in stored:
        t = tracks[i]
        bps = _dtype(t).itemsize
        if layout.gap == "abut":
            off = (cur + bps - 1) // bps * bps  # sample alignment is all the ABI asks for
            plan.append((i, off, off))
        else:
            k = seen.get(bps, 0)
            seen[bps] = k + 1
            r = residues(bps)[(k + layout.shift) % 7]
            off = cur + GUARD_FRAMES * bps
            off += (r - off) % 128
            plan.append((i, off, off - (off - cur) // bps * bps))
        offset[i] = off
        cur = off + _nbytes(t)
        if layout.gap == "guard":
            cur += GUARD_FRAMES * bps  # the guard behind the track, in its own format
    arena = np.zeros(max(cur, 16), dtype=np.uint8)

    # pass 2: bytes
    for i, off, g0 in plan:
        t = tracks[i]
        dt = _dtype(t)
        if off > g0:
            arena[g0:off] = guard_samples(dt, (off - g0) // dt.itemsize, layout.guard).view(np.uint8)
            guards.append((g0, off))
        p = off
        for c in t.channels:
            arena[p:p + c.nbytes] = np.ascontiguousarray(c).view(np.uint8)
            p += c.nbytes
        if layout.gap == "guard":
            arena[p:p + GUARD_FRAMES * dt.itemsize] = guard_samples(dt, GUARD_FRAMES, layout.guard).view(np.uint8)
            guards.append((p, p + GUARD_FRAMES * dt.itemsize))

    descs = (_capi.TrackDesc * max(1, n))()
    for i, t in enumerate(tracks):
        descs[i].offset_bytes = offset[home[i]]
        descs[i].frames = int(t.channels[0].shape[0])
        descs[i].sample_rate = int(t.sample_rate)
        descs[i].channels = len(t.channels)
        descs[i].format = FMT[_dtype(t)]
    return arena, descs, guards


def channel_bytes(arena, desc, dtype, c):
    """Channel c of the track `desc` describes, sliced out of the arena."""
    nb = int(desc.frames) * np.dtype(dtype).itemsize
    a = int(desc.offset_bytes) + c * nb
    return arena[a:a + nb].view(dtype)
