"""The tracks of the position sweeps (tests/test_peak_sweep_cpu.py, tests/test_gpu_peak_sweep.py,
tests/test_gpu_r128_peak_sweep.py).  Not part of the product.

A maximum or an "any" flag observes one frame only, so a sweep is one batch of many short tracks that are identical but for one
marker: track i carries it at position p_i.  The background is the quiet noise of tests/layout_cases.py (|x| <= 2^-7), drawn on
the 16-bit grid, so that the same normalised signal exists exactly as s16 `v`, f32 `v / 32768` and s32 `v << 16` and one float64
reference serves all three.  A marker is at least 0.9 of full scale (more than 100 x the background), exact in every format, and
distinct for every track of a call: track i of n carries 32768 - j, j = (i + rot) mod n, negative where j is even.  So j = 0 is
exactly negative full scale (-1.0 / INT16_MIN / INT32_MIN), the signs alternate, and a peak credited to a neighbouring track
shows.  `rot` moves the full-scale track to another position from call to call.  In a stereo track the marker goes to channel
p % 2.

Nothing here comes from the code under test: the expected sample peak of track i is |marker_i| / 32768."""
import functools
import math
from dataclasses import dataclass

import numpy as np

import layout_cases
import r128ref

FORMATS = layout_cases.FORMATS
NP_TYPE = {"f32": np.float32, "s16": np.int16, "s32": np.int32}
BACKGROUND_MAX = 256  # 2^-7 of full scale on the 16-bit grid
TP_TILE = 1024  # frames per tile of the true-peak kernel; 16 tiles make one workgroup's chunk

RG1_OFFSETS = (-17, -16, -13, -12, -5, -4, -1, 0, 1, 3, 4, 11, 12, 15, 16)  # 16: the TM tile, 12: the halo turn, 4: a piece
R128_OFFSETS = (-33, -32, -5, -4, -1, 0, 1, 3, 4, 31, 32)  # 32: the R 128 tile
EDGE = 40  # the first and last frames every structure list adds
MAX_ARENA = 256 << 20


def grid16(seed, frames, nch):
    """The quiet background on the 16-bit grid: `nch` int32 arrays, |v| <= 256."""
    return [c.astype(np.int32) for c in layout_cases.quiet(seed, frames, nch, "s16")]


def as_format(v, fmt):
    """Values of the 16-bit grid in a sample format; exact in each."""
    v = np.asarray(v, dtype=np.int32)
    if fmt == "f32":
        return (v / 32768.0).astype(np.float32)
    if fmt == "s16":
        return v.astype(np.int16)
    return v << 16


def unit(v):
    """Values of the 16-bit grid as float64, full scale 1.0: what every format normalises to."""
    return np.asarray(v, dtype=np.float64) / 32768.0


def markers(n, rot=0):
    j = (np.arange(n) + rot) % n
    return np.where(j % 2 == 0, -1, 1).astype(np.int32) * (32768 - j).astype(np.int32)


def exhaustive(frames):
    return np.arange(frames)


def _structure(frames, step, offsets):
    p = {k * step + d for k in range(frames // step + 2) for d in offsets}
    p |= set(range(EDGE)) | set(range(frames - EDGE, frames))
    return np.array(sorted(q for q in p if 0 <= q < frames))


def rg1_structure(frames, window):
    return _structure(frames, window, RG1_OFFSETS)


def r128_structure(frames, hop):
    return _structure(frames, hop, R128_OFFSETS)


def tp_structure():
    return np.array([TP_TILE * k + d for k in range(1, 18) for d in range(-16, 17)])


@dataclass(frozen=True, eq=False)
class Sweep:
    """One list of positions over one background.  `boundaries`: every b whose b - 1 and b a structure list must contain.
    `doublets`: a track whose position is odd carries the marker in frames p and p + 1 (p + 1 < frames), so that its true peak
    lies between two samples."""
    name: str
    rate: int
    frames: int
    nch: int
    positions: np.ndarray
    seed: int
    boundaries: tuple = ()
    doublets: bool = False
    formats: tuple = FORMATS  # the formats the GPU modules run this list in; each call's arena stays under MAX_ARENA

    def __len__(self):
        return len(self.positions)

    @functools.cached_property
    def background(self):
        return grid16(self.seed, self.frames, self.nch)

    def channel(self, p):
        return int(p) % self.nch

    def marked(self, i, rot=0):
        """Track i on the 16-bit grid (int32 channels), a copy."""
        ch = [c.copy() for c in self.background]
        p, m = int(self.positions[i]), int(markers(len(self), rot)[i])
        ch[self.channel(p)][p] = m
        if self.doublets and p % 2 and p + 1 < self.frames:
            ch[self.channel(p)][p + 1] = m
        return ch

    def arena_bytes(self, fmt):
        return len(self) * self.nch * self.frames * np.dtype(NP_TYPE[fmt]).itemsize

    def tracks(self, fmt, rot=0, pick=None):
        """-> (per track its channel arrays in `fmt`, views of one block; the tracks' markers on the 16-bit grid).
        pick: indices into the position list (the formats of one call may share a list between them)."""
        idx = np.arange(len(self)) if pick is None else np.asarray(pick)
        pos = self.positions[idx]
        m = markers(len(self), rot)[idx]
        block = np.empty((len(idx), self.nch, self.frames), dtype=NP_TYPE[fmt])
        block[:] = np.stack([as_format(c, fmt) for c in self.background])
        rows, mf = np.arange(len(idx)), as_format(m, fmt)
        block[rows, pos % self.nch, pos] = mf
        if self.doublets:
            two = (pos % 2 == 1) & (pos + 1 < self.frames)
            block[rows[two], pos[two] % self.nch, pos[two] + 1] = mf[two]
        return [[block[i, c] for c in range(self.nch)] for i in range(len(idx))], m

    def true_peak_refs(self, rot=0):
        """r128ref.true_peak of every track: the float64 interpolator over the marked channel, and the other channel's
        background, which no marker changes, once."""
        return _true_peak_refs(self, rot)


@functools.lru_cache(maxsize=None)
def _true_peak_refs(sw, rot):
    others = [r128ref.true_peak([unit(c)], sw.rate) for c in sw.background]
    out = np.empty(len(sw))
    for i in range(len(sw)):
        c = sw.channel(sw.positions[i])
        rest = max([others[k] for k in range(sw.nch) if k != c], default=0.0)
        out[i] = max(r128ref.true_peak([unit(sw.marked(i, rot)[c])], sw.rate), rest)
    return out


def expected_peaks(m):
    return np.abs(unit(m))


def window(rate):
    return rate // 20


def hop(rate):
    return r128ref.hop_frames(rate)


def _multiples(step, frames):
    return tuple(range(step, frames, step))


# ---- ReplayGain 1.0 ---------------------------------------------------------------------------------------------------------
RG1_RATES = (8000, 22050)  # W = 400: the servo form of the moment window; W = 1102: the classic form


@functools.lru_cache(maxsize=None)
def rg1_exhaustive(rate, nch):
    n = 2 * window(rate) + 37
    return Sweep(f"rg1-exhaustive-{rate}-{nch}ch", rate, n, nch, exhaustive(n), 8100 + rate % 97 + nch,
                 formats=FORMATS if nch == 2 else ("s16",))


@functools.lru_cache(maxsize=None)
def rg1_structured(nch):
    """Two full lanes of 37 windows, a ragged third lane and a partial window; s16 stereo and f32 mono between them."""
    rate = 8000
    w = window(rate)
    n = 77 * w + 5
    return Sweep(f"rg1-structure-{nch}ch", rate, n, nch, rg1_structure(n, w), 8200 + nch, _multiples(w, n),
                 formats=("s16",) if nch == 2 else ("f32",))


FIND_PEAK_FRAMES, FIND_PEAK_CHANNELS = 700, 3


@functools.lru_cache(maxsize=None)
def find_peak_background():
    return grid16(8300, FIND_PEAK_FRAMES, FIND_PEAK_CHANNELS)


def find_peak_track(index, fmt):
    """The three-channel track with its marker at sample `index` of the planar block -> (channels in fmt, marker)."""
    m = int(markers(FIND_PEAK_FRAMES * FIND_PEAK_CHANNELS)[index])
    ch = [c.copy() for c in find_peak_background()]
    ch[index // FIND_PEAK_FRAMES][index % FIND_PEAK_FRAMES] = m
    return [as_format(c, fmt) for c in ch], m


NONFINITE_RATE, NONFINITE_FRAMES = 8000, 2 * 400 + 37
NONFINITE_KINDS = {"nan": np.nan, "+inf": np.inf, "-inf": -np.inf}


def nonfinite_tracks(oracle, what):
    """f32 stereo synth noise (what the hand-picked non-finite test uses) with one non-finite sample, at every position, in
    channel p % 2 -> per track its two channels, and the clean track."""
    n = NONFINITE_FRAMES
    clean = [oracle.synth_f32(93, c, NONFINITE_RATE, n) for c in range(2)]
    block = np.empty((n, 2, n), dtype=np.float32)
    block[:] = np.stack(clean)
    p = np.arange(n)
    block[p, p % 2, p] = np.float32(NONFINITE_KINDS[what])
    return [[block[i, 0], block[i, 1]] for i in range(n)], clean


# ---- EBU R 128 --------------------------------------------------------------------------------------------------------------
R128_RATE = 8000


@functools.lru_cache(maxsize=None)
def r128_exhaustive():
    n = 4 * hop(R128_RATE) + 45
    return Sweep("r128-exhaustive", R128_RATE, n, 2, exhaustive(n), 8400, doublets=True)


@functools.lru_cache(maxsize=None)
def r128_structured():
    h = hop(R128_RATE)
    n = 40 * h + 333
    return Sweep("r128-structure", R128_RATE, n, 2, r128_structure(n, h), 8401, _multiples(h, n), doublets=True)


TP_RATES = (8000, 96000)  # F = 4 (12 frames of history), F = 2 (24)
TP_FRAMES = 17 * TP_TILE + 100


@functools.lru_cache(maxsize=None)
def tp_structured(rate):
    return Sweep(f"tp-structure-{rate}", rate, TP_FRAMES, 1, tp_structure(), 8500 + rate % 89,
                 tuple(TP_TILE * k for k in range(1, 18)), doublets=True)


def tp_format_of(p):
    """The formats cycle with the tile index k."""
    return FORMATS[((int(p) + 16) // TP_TILE) % 3]


def r128_nonfinite_tracks():
    """The exhaustive R 128 sweep's background as f32 with a NaN at every position, channel p % 2 -> per track its two channels."""
    sw = r128_exhaustive()
    n = sw.frames
    block = np.empty((n, 2, n), dtype=np.float32)
    block[:] = np.stack([as_format(c, "f32") for c in sw.background])
    p = np.arange(n)
    block[p, p % 2, p] = np.float32(np.nan)
    return [[block[i, 0], block[i, 1]] for i in range(n)]


@functools.lru_cache(maxsize=None)
def r128_nonfinite_refs():
    """(sample peak, true peak) of every track of r128_nonfinite_tracks: r128ref drops the non-finite sample from the one and
    exactly the interpolator outputs it touches from the other."""
    sw = r128_exhaustive()
    bg = [as_format(c, "f32") for c in sw.background]
    others_tp = [r128ref.true_peak([c], sw.rate) for c in bg]
    others_sp = [r128ref.sample_peak([c]) for c in bg]
    sp, tp = np.empty(sw.frames), np.empty(sw.frames)
    for p in range(sw.frames):
        c = p % 2
        x = bg[c].copy()
        x[p] = np.nan
        sp[p] = max(r128ref.sample_peak([x]), others_sp[1 - c])
        tp[p] = max(r128ref.true_peak([x], sw.rate), others_tp[1 - c])
    return sp, tp


def all_sweeps():
    """Every marker sweep of the two GPU modules; tests/test_peak_sweep_cpu.py holds each to the preconditions."""
    out = [rg1_exhaustive(rate, nch) for rate in RG1_RATES for nch in (2, 1)]
    out += [rg1_structured(2), rg1_structured(1), r128_exhaustive(), r128_structured()]
    out += [tp_structured(rate) for rate in TP_RATES]
    return out


def windows_of(rate, frames):
    """Windows the ReplayGain 1.0 histogram counts for a track none of whose windows is silent: the partial last one too."""
    return math.ceil(frames / window(rate))
