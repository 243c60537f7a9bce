"""The AccurateRip signatures at every drive offset (include/mp3rgain_amd_rip.h, DRIVE OFFSETS) restated in numpy, and the
discs the CPU and GPU tests share.

The restatement is independent of the library: the disc's words padded with `radius` zeros on both sides and, per track and
offset, a slice times arange(from, to + 1) in uint64, summed as `& 0xFFFFFFFF` and `>> 32`.  Offset 0 is asserted against
tests/rip_cases.py's `want`.  The discs take the kernel's own tile from rg_rip_offsets_kernel_shape.  Not part of the product."""
import sys
from collections import namedtuple
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(Path(__file__).resolve().parent))

import rip_cases as rc  # noqa: E402

FIRST, LAST = rc.FIRST, rc.LAST
RADIUS_MAX = 2939
Disc = namedtuple("Disc", "name tracks flags")  # tracks: [(left, right)] int16 planes; flags: one per track
M32 = np.uint64(0xFFFFFFFF)


def shape():
    from mp3rgain_amd import replaygain

    return replaygain.rip_offsets_kernel_shape()


def words(disc):
    """W of the whole disc, uint64."""
    parts = [l.astype(np.uint16).astype(np.uint64) | (r.astype(np.uint16).astype(np.uint64) << np.uint64(16)) for l, r in disc.tracks]
    return np.concatenate(parts) if parts else np.zeros(0, np.uint64)


def restate(disc, radius):
    """-> (arv1, arv2), uint32 [n, 2 radius + 1], [t][o + radius]."""
    n = len(disc.tracks)
    pad = np.zeros(radius, np.uint64)
    w = np.concatenate([pad, words(disc), pad])  # w[radius + j] = W[j]
    v1, v2 = np.zeros((n, 2 * radius + 1), np.uint32), np.zeros((n, 2 * radius + 1), np.uint32)
    base = 0
    for t, (left, _) in enumerate(disc.tracks):
        frames = len(left)
        lo, hi = rc.ar_range(frames, disc.flags[t])
        lo = max(lo, 1)
        if hi >= lo:
            i = np.arange(lo, hi + 1, dtype=np.uint64)
            for o in range(-radius, radius + 1):
                a = radius + base + lo - 1 + o  # of W[B + lo - 1 + o]
                p = w[a:a + len(i)] * i
                s_lo = int((p & M32).sum(dtype=np.uint64)) & 0xFFFFFFFF
                s_hi = int((p >> np.uint64(32)).sum(dtype=np.uint64)) & 0xFFFFFFFF
                v1[t, o + radius] = s_lo
                v2[t, o + radius] = (s_lo + s_hi) & 0xFFFFFFFF
        base += frames
    for t, (left, right) in enumerate(disc.tracks):
        wt = rc.want(left, right, disc.flags[t])
        assert (int(v1[t, radius]), int(v2[t, radius])) == (wt.arv1, wt.arv2), (disc.name, t)
    return v1, v2


def lengths():
    t, _ = shape()
    return [0, 1, 2, 3, 1500, t - 1, t, t + 1, 2 * t + 1, 2939, 2940, 2941, 5879, 5880, 5881]


def _disc_flags(n):
    fl = [0] * n
    if n:
        fl[0] |= FIRST
        fl[-1] |= LAST
    return fl


_cache = {}


def discs():
    """Every length of lengths() and every content, in discs of at most 8 tracks and 40 000 frames; each mixes tracks
    shorter than the radius between longer ones, so that one halo spans several of them.  Built once."""
    if "discs" in _cache:
        return _cache["discs"]
    t, _ = shape()
    rng = np.random.default_rng(0x4F464653)

    def mk(name, spec, flags=None):
        tracks = [rc._planes(kind, n, rng) for kind, n in spec]
        return Disc(name, tracks, flags if flags is not None else _disc_flags(len(tracks)))

    out = [
        mk("mixed_a", [("random", 5879), ("one_at_start", 1), ("ffff", 3), ("random", 2 * t + 1), ("zero", 0), ("sparse", 2), ("ffff", t),
                       ("random", 2941)]),
        mk("mixed_b", [("sparse", t + 1), ("random", 2), ("one_at_end", 1), ("random", 0), ("ffff", 5880), ("random", 1500), ("ffff", 3),
                       ("random", t - 1)]),
        mk("mixed_c", [("ffff", 5881), ("random", 2939), ("zero", 0), ("random", 1), ("sparse", 2940), ("zero", 1500), ("one_at_start", 2),
                       ("random", 5879)]),
        # every flag combination on middle tracks, long and short
        mk("flags", [("random", 2941), ("random", 5881), ("ffff", 3), ("random", t + 1), ("sparse", 5880), ("one_at_end", 2940), ("random", 1500)],
           [LAST, FIRST | LAST, FIRST, FIRST | LAST, LAST, FIRST, 0]),
        mk("impulses", [("one_at_start", 1500), ("one_at_end", 3), ("one_at_end", t), ("one_at_start", 2), ("one_at_start", 2941)], [0] * 5),
        mk("single", [("random", 2 * t + 1)]),                 # one track, flagged first and last
        mk("single_one_position", [("ffff", 5880)]),            # from = to = 2940
        mk("single_empty", [("random", 5879)]),                 # to < from
        mk("short", [("random", 1), ("ffff", 2), ("sparse", 3), ("zero", 0), ("random", 1500), ("one_at_end", 3)], [0] * 6),  # shorter than the radius
        mk("zeros", [("zero", 2941), ("zero", 1)]),
    ]
    assert sorted({len(l) for d in out for l, _ in d.tracks}) == sorted(set(lengths()))
    assert all(len(d.tracks) <= 8 and sum(len(l) for l, _ in d.tracks) <= 40000 for d in out)
    assert sum(len(l) for l, _ in out[8].tracks) < RADIUS_MAX
    _cache["discs"] = out
    return out


def restated(radius):
    """{disc name: (arv1, arv2)} at `radius`, computed once and shared."""
    key = ("restated", radius)
    if key not in _cache:
        _cache[key] = {d.name: restate(d, radius) for d in discs()}
    return _cache[key]


def tracks(disc):
    return [rc.Track([l, r], 44100) for l, r in disc.tracks]
