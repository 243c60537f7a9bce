"""The tracks of the arena-layout tests (tests/test_arena_layouts_cpu.py, tests/test_gpu_arena_layouts.py) and of
`tools/r128_refcheck.py --layout-cases`.  Not part of the product.

Every track is quiet uniform noise, |x| <= 2^-7, from a fixed seed: a guard sample (tests/arena_layouts.py) is at least 128
times any of them, so one guard sample consumed by a kernel changes a peak, a true peak, a window or a block beyond any
tolerance.  Some tracks also carry legitimate full-scale samples (-1.0, INT16_MIN, INT32_MIN: a sample peak of exactly 1.0)
at their very edges: the end of channel 0 abuts the start of channel 1 in memory, so reading one into the other shows too.

A case is (id, [channel arrays], rate).  Everything is short: about 2 s at 8 kHz at the most, but for one track of 3.1 s,
the shortest that has short-term blocks."""
import functools
import json
from pathlib import Path

import numpy as np

FORMATS = ("f32", "s16", "s32")
QUIET = 2.0 ** -7
W441 = 2205  # the 50 ms window of the ReplayGain 1.0 path at 44.1 kHz
TP_CHUNK = 16 * 1024  # frames one workgroup of the true-peak kernel walks


def tp_factor(rate):
    return 4 if rate < 96000 else 2 if rate < 192000 else 1


def quiet(seed, frames, nch, fmt):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(nch):
        x = rng.uniform(-QUIET, QUIET, frames)
        if fmt == "f32":
            out.append(x.astype(np.float32))
        elif fmt == "s16":
            out.append(np.round(x * 32768.0).astype(np.int16))
        else:
            out.append(np.round(x * 2147483648.0).astype(np.int32))
    return out


def full_scale(chans, c, frames):
    """Negative full scale into the given frames of channel c."""
    dt = chans[c].dtype
    chans[c][list(frames)] = np.float32(-1.0) if dt == np.float32 else np.iinfo(dt).min
    return chans


def format_cases(rate, frames0):
    """The three formats x mono, stereo, three channels, odd frame counts (channel 1 of an s16 track then starts 2 bytes
    off a 4-byte boundary)."""
    cases, k = [], 0
    for fmt in FORMATS:
        for nch in (1, 2, 3):
            frames = frames0 + 2 * k + 1
            cases.append((f"fmt-{fmt}-{nch}ch-{rate}-{frames}", quiet(1000 + k, frames, nch, fmt), rate))
            k += 1
    return cases


EDGES = (("first1", lambda n: range(0, 1)), ("first4", lambda n: range(0, 4)), ("last1", lambda n: range(n - 1, n)),
         ("last4", lambda n: range(n - 4, n)))


def edge_cases(rate, frames0):
    """Full scale in the first / last 1 / 4 frames of channel 0, and of channel 1 only; every format."""
    cases, k = [], 0
    for fmt in FORMATS:
        for c in (0, 1):
            for name, where in EDGES:
                frames = frames0 + (k % 5)
                ch = full_scale(quiet(2000 + k, frames, 2, fmt), c, where(frames))
                cases.append((f"edge-{fmt}-ch{c}-{name}-{frames}", ch, rate))
                k += 1
    return cases


@functools.lru_cache(maxsize=None)
def rg1_cases():
    """ReplayGain 1.0: formats and channels, edge-loud tracks, lengths around the decisions of the TM loader at 44.1 kHz
    (`start + roundup4(L) <= frames` flips inside 3 W + {-1 .. 4}), a track shorter than a window, an empty one, and short
    tracks at other rates, so that several tracks share a wave and cross wave and block boundaries."""
    cases = format_cases(44100, 2 * W441 + 300) + edge_cases(8000, 4 * 800 + 3)
    k = 0
    for d in (-1, 0, 1, 2, 3, 4):
        for fmt in FORMATS:
            frames = 3 * W441 + d
            ch = quiet(3000 + k, frames, 2, fmt)
            if k % 2:
                full_scale(ch, k % 4 // 2, range(frames - 1, frames))
            cases.append((f"len-3W{d:+d}-{fmt}", ch, 44100))
            k += 1
    cases.append(("len-short", quiet(3100, W441 - 7, 2, "f32"), 44100))
    cases.append(("len-empty", quiet(3101, 0, 2, "s16"), 44100))
    for j, (rate, secs) in enumerate(((8000, 1.2), (8000, 0.3), (48000, 0.41), (48000, 0.3), (96000, 0.31), (96000, 0.3))):
        frames = int(rate * secs) + j
        ch = full_scale(quiet(3200 + j, frames, 1 + j % 2, FORMATS[j % 3]), 0, range(frames - 1, frames))
        cases.append((f"rate-{rate}-{frames}-{FORMATS[j % 3]}", ch, rate))
    return cases


def tp_geometry_lengths(rate):
    hist = 48 // tp_factor(rate)
    return [1023, 1024, 1025, TP_CHUNK - hist - 1, TP_CHUNK - hist // 2 + 1, TP_CHUNK - 1, TP_CHUNK, TP_CHUNK + 1]


@functools.lru_cache(maxsize=None)
def tp_geometry_cases():
    """(id, channels, rate, frame of the full-scale sample): the true-peak kernel works in chunks of 16 tiles of 1024 frames
    plus a tail of 48 / F frames; an impulse in a track's last frame peaks 24 / F frames after the track's end, for these
    lengths in a tile or a workgroup that holds no input frame of its own."""
    cases, k = [], 0
    for rate in (8000, 96000):
        for n in tp_geometry_lengths(rate):
            for where in (0, n - 1):
                fmt = FORMATS[k % 3]
                nch = 1 + (k // 3) % 2
                ch = full_scale(quiet(4000 + k, n, nch, fmt), nch - 1, (where,))
                cases.append((f"tp-{rate}-{n}-at{'0' if where == 0 else 'N-1'}-{fmt}-{nch}ch", ch, rate, where))
                k += 1
    return cases


@functools.lru_cache(maxsize=None)
def r128_cases():
    """EBU R 128: formats and channels, edge-loud tracks, lengths around a hop and a block at 8 kHz (hop 800), the true-peak
    geometry, and the rate edges: 384000 (the maximum, F = 1), 95999 and 191999 (the last rates with F = 4 and F = 2) and
    8004 (a hop that is not rate / 10)."""
    hop = 800
    cases = format_cases(8000, 6 * hop + 10) + edge_cases(8000, 4 * hop + 3)
    k = 0
    for name, frames, loud in (("hop-1", hop - 1, ()), ("4hops", 4 * hop, ()), ("4hops+1", 4 * hop + 1, (4 * hop,)),
                               ("7hops", 7 * hop, ()), ("7hops+1", 7 * hop + 1, (7 * hop,)),
                               ("7hops+799", 7 * hop + 799, (7 * hop + 798,)), ("20hops+799", 20 * hop + 799, (20 * hop + 400,))):
        fmt = FORMATS[k % 3]
        # the full-scale sample sits in the partial last hop: it counts for the peak and for no energy
        cases.append((f"len-{name}-{fmt}", full_scale(quiet(5000 + k, frames, 2, fmt), k % 2, loud), 8000))
        k += 1
    # the one track long enough (30 hops) to have short-term blocks at all
    cases.append(("len-31hops+5-s16-mono", quiet(5100, 31 * hop + 5, 1, "s16"), 8000))
    cases += [(cid, ch, rate) for cid, ch, rate, _ in tp_geometry_cases()]
    for j, rate in enumerate((384000, 95999, 191999, 8004)):
        frames = int(0.6 * rate) + 1
        ch = full_scale(quiet(6000 + j, frames, 2, FORMATS[j % 3]), j % 2, (frames - 1,) if j % 2 else (0,))
        cases.append((f"rate-{rate}-{FORMATS[j % 3]}", ch, rate))
    return cases


REPEATS = (0, 5, -1, 5)


def with_repeats(cases):
    """The cases, and a few of them again as the same objects: what an aliased layout stores once."""
    return list(cases) + [cases[i] for i in REPEATS]


def nonfinite_case():
    """One NaN in the middle of channel 0 and one -Inf in channel 1 (f32, 44.1 kHz, F = 4: an interpolator output of frame n
    reads frames n - 12 .. n, and a sample peaks 6 frames after itself).  Full-scale samples 5 frames before and 3 frames
    after each of them peak in outputs the non-finite sample touches, which do not count; two samples of 0.5 at 7 and 8
    frames after the NaN peak (about 0.63) in the first output frame it does not touch.  So the true peak is about 0.63,
    below the sample peak of 1.0, only if exactly the touched outputs are dropped: one frame fewer and it is about 1.0, one
    frame more and the 0.63 is lost."""
    rate, frames = 44100, 3 * 4410 + 77
    ch = quiet(7000, frames, 2, "f32")
    m, q = frames // 2, 1234
    ch[0][m] = np.nan
    ch[1][q] = -np.inf
    full_scale(ch, 0, (m - 5, m + 3))
    full_scale(ch, 1, (q - 5, q + 3))
    ch[0][m + 7] = ch[0][m + 8] = np.float32(0.5)
    return ch, rate


def load_measured():
    return json.loads((Path(__file__).resolve().parent / "golden" / "r128_layout_measured.json").read_text())
