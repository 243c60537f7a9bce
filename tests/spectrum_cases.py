"""The spectral scan (include/mp3rgain_amd_spectrum.h) restated in float64 numpy, and the cases the CPU and GPU tests share.

The restatement is independent of the library: numpy's rfft over a strided view of the frames, and the verdict written from the
header's definitions with the math module.  The case list takes the kernels' tile size from rg_spectrum_kernel_shape.  Not
part of the product."""
import functools
import json
import math
import sys
from collections import namedtuple
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

from mp3rgain_amd import _capi  # noqa: E402

L, H, BANDS, W = 4096, 2048, 256, 8
MEASURED = ROOT / "tests" / "golden" / "spectrum_measured.json"
TOLERANCE_FACTOR = 8.0  # the tests allow this many times the recorded worst error (tools/spectrum_refcheck.py)
F64_TOLERANCE = 1e-11   # route 0 against numpy, of the plane's total energy: two float64 transforms of 4096 points

Tr = namedtuple("Tr", "name channels sample_rate")  # .channels: planes of one dtype and length (tests/arena_layouts.pack takes these)


def shape():
    import mp3rgain_amd as rg
    return rg.spectrum_kernel_shape()


# ---- the definitions ----------------------------------------------------------------------------------------------------------
def frames_of(n):
    return 0 if n < L else (n - L) // H + 1


@functools.lru_cache(maxsize=None)
def window():
    n = np.arange(L, dtype=np.float64)
    return (0.5 - 0.5 * np.cos(2.0 * np.pi * n / L)).astype(np.float32)


def values(x):
    """The sample values as the header defines them: float32."""
    if x.dtype == np.float32:
        return x
    w = 16 if x.dtype == np.int16 else 32
    return x.astype(np.float32) * np.float32(2.0 ** -(w - 1))


def want_plane(x):
    """-> (E[256] float64, analysed, skipped)."""
    k = frames_of(len(x))
    e = np.zeros(BANDS, dtype=np.float64)
    if k == 0:
        return e, 0, 0
    v = values(x).astype(np.float64)
    fr = np.lib.stride_tricks.sliding_window_view(v, L)[::H][:k]
    good = np.isfinite(fr).all(axis=1)
    w = window().astype(np.float64)
    for a in range(0, k, 64):
        blk = fr[a:a + 64][good[a:a + 64]]
        if len(blk):
            p = np.abs(np.fft.rfft(blk * w, axis=1)[:, 1:L // 2 + 1]) ** 2
            e += p.reshape(len(blk), BANDS, 8).sum(axis=(0, 2))
    return e, int(good.sum()), int(k - good.sum())


def verdict(p, analysed, fs, edge_db=30.0, min_cutoff_hz=4000.0):
    """-> (cutoff_hz, edge_db, flags) from the 256 band levels."""
    p = [float(x) for x in p]
    top = max(p)
    if analysed == 0 or not top > 0.0:
        return 0.0, 0.0, 0
    floor = top * 1e-12
    ratio = math.pow(10.0, -edge_db / 10.0)
    best, best_d = None, 0.0
    for j in range(W - 1, BANDS - W):
        f_hi = (8.0 * j + 8.5) * fs / L
        if not f_hi >= min_cutoff_hz:
            continue
        below = 0.0
        for i in range(j - W + 1, j + 1):
            below += p[i]
        above = 0.0
        for i in range(j + 1, j + W + 1):
            above += p[i]
        below /= W
        above = max(above / W, floor)
        d = 10.0 * math.log10(below / above) if below > 0.0 else -math.inf  # (C's log10(0))
        if d >= edge_db and max(max(p[j + 1:]), floor) <= below * ratio and (best is None or d > best_d):
            best, best_d = j, d
    if best is None:
        return fs / 2.0, 0.0, 0
    cutoff = (8.0 * best + 8.5) * fs / L
    flags = _capi.SPEC_BANDLIMITED
    if fs >= 64000 and cutoff <= 24500.0:
        flags |= _capi.SPEC_UPSAMPLED
    return cutoff, best_d, flags


def verdict_of_energy(e, analysed, fs, **kw):
    p = [float(x) / (8.0 * analysed) if analysed else 0.0 for x in e]
    return verdict(p, analysed, fs, **kw)


def want_track_flags(tr, channel_flags, skipped):
    flags = _capi.SPEC_COMPLETE
    if frames_of(len(tr.channels[0])) == 0:
        flags |= _capi.SPEC_SHORT
    if any(skipped):
        flags |= _capi.SPEC_NONFINITE
    for f in channel_flags:
        flags |= f
    return flags


# ---- signals ------------------------------------------------------------------------------------------------------------------
def _rng(name):
    return np.random.default_rng(int.from_bytes(name.encode()[:8].ljust(8, b"\0"), "little"))


def shaped_noise(name, n, fs, slope=0.0, cut=None, transition=300.0, level=0.25):
    """Gaussian noise of amplitude spectrum f^-slope (0 white, 0.5 pink, 1 = 1/f^2 power), optionally brick-walled at `cut` Hz with a
    raised-cosine transition, scaled to an RMS of `level`."""
    r = _rng(name)
    m = n + 2 * L
    spec = np.fft.rfft(r.standard_normal(m))
    f = np.fft.rfftfreq(m, 1.0 / fs)
    shape_ = np.ones_like(f)
    if slope:
        shape_[1:] = (f[1:] / 20.0).clip(min=1.0) ** -slope
    if cut is not None:
        t = ((f - (cut - transition / 2)) / transition).clip(0.0, 1.0)
        shape_ *= 0.5 + 0.5 * np.cos(np.pi * t)
    x = np.fft.irfft(spec * shape_, m)[L:L + n]
    return x * (level / np.sqrt(np.mean(x * x)))


def as_s16(x):
    return np.clip(np.rint(x * 32768.0), -32768, 32767).astype(np.int16)


def as_s24(x):
    """24-bit samples left-justified in int32, as the WAV and FLAC routes stage them."""
    return (np.clip(np.rint(x * 8388608.0), -8388608, 8388607).astype(np.int32)) << 8


def as_f32(x):
    return x.astype(np.float32)


CONVERT = {"s16": as_s16, "s24": as_s24, "f32": as_f32}


def lengths(t):
    out = [L - 1, L, L + H - 1, L + H]
    for k in (3, t - 1, t, t + 1, 2 * t + 1):
        out += [L + (k - 1) * H, L + (k - 1) * H + 1]
    return out


VERDICT_FRAMES = 40
VERDICT_SIGNALS = (
    # name, rate, format, slope, cut, transition, level, bandlimited, upsampled
    ("white", 44100, "s16", 0.0, None, 300.0, 0.25, False, False),
    ("pink", 44100, "s16", 0.5, None, 300.0, 0.25, False, False),
    ("brown", 44100, "s16", 1.25, None, 300.0, 0.25, False, False),
    ("white-16k", 44100, "s16", 0.0, 16000.0, 300.0, 0.25, True, False),
    ("pink-16k", 44100, "s16", 0.5, 16000.0, 300.0, 0.25, True, False),
    ("white-16k-wide", 44100, "s16", 0.0, 16000.0, 2000.0, 0.25, True, False),
    ("brown-19k", 44100, "s16", 1.0, 19000.0, 300.0, 0.25, True, False),
    ("pink-up96k", 96000, "s24", 0.5, 21900.0, 300.0, 0.25, True, True),
    ("pink-96k", 96000, "s24", 0.5, None, 300.0, 0.25, False, False),
    ("pink-60dB", 44100, "s16", 0.5, None, 300.0, 0.00025, False, False),
    ("white-16k-f32", 48000, "f32", 0.0, 16000.0, 300.0, 0.25, True, False),
)


def verdict_signal(name):
    """The float64 signal of a verdict case before its conversion, and its row."""
    row = next(r for r in VERDICT_SIGNALS if r[0] == name)
    n = L + (VERDICT_FRAMES - 1) * H + 37
    return shaped_noise(name, n, row[1], row[3], row[4], row[5], row[6]), row


@functools.lru_cache(maxsize=None)
def tracks():
    """Every case as a Tr; the names are unique."""
    t = shape()[3]
    out = []
    fmts = ("s16", "s24", "f32")
    # lengths around the frame and tile boundaries, white noise, every format
    for n in lengths(t):
        for fmt in fmts:
            x = _rng(f"w{n}{fmt}").uniform(-0.5, 0.5, n)
            out.append(Tr(f"white-{fmt}-{n}", (CONVERT[fmt](x),), 44100))
    # one tone in the middle of band j, 32 bands per track: the even frames hold one tone each, the odd ones two halves
    seg = 2 * H
    for k in range(8):
        x = np.zeros(32 * seg)
        for s in range(32):
            j = 32 * k + s
            ph = 2.0 * np.pi * (8 * j + 4.5) / L * np.arange(seg)
            x[s * seg:(s + 1) * seg] = 0.05 * (1 + j % 7) * np.sin(ph + 0.1 * j)
        out.append(Tr(f"tones-{k}", (CONVERT[fmts[k % 3]](x),), (8000, 44100, 48000, 96000)[k % 4]))
    # loud even hops, quiet odd hops; two and six channels, each channel its own signal
    n = L + 6 * H + 5
    env = np.where((np.arange(n) // H) % 2 == 0, 1.0, 1e-3)
    for fmt in fmts:
        r = _rng("evenodd" + fmt)
        out.append(Tr(f"evenodd-{fmt}", tuple(CONVERT[fmt](r.uniform(-0.5, 0.5, n) * env * (c + 1) / 2) for c in range(2)), 48000))
        out.append(Tr(f"six-{fmt}", tuple(CONVERT[fmt](r.uniform(-0.5, 0.5, L + 2 * H + 1) / (c + 1)) for c in range(6)), 96000))
    # the verdict signals
    for row in VERDICT_SIGNALS:
        x, _ = verdict_signal(row[0])
        out.append(Tr(f"verdict-{row[0]}", (CONVERT[row[2]](x),), row[1]))
    sine = 0.5 * np.sin(2.0 * np.pi * 1000.0 / 44100.0 * np.arange(L + 39 * H))
    out.append(Tr("verdict-sine-1k", (as_s16(sine),), 44100))
    # float planes with non-finite samples, and values beyond +-1
    n = L + 4 * H + 100
    base = _rng("nonfinite").uniform(-0.5, 0.5, n).astype(np.float32)
    for name, at, val in (("nan-first", 0, np.nan), ("nan-overlap", 3 * H + 5, np.nan), ("nan-tail", n - 1, np.nan), ("inf-mid", 2 * H + 1000, np.inf),
                          ("neginf-last-frame", 4 * H + L - 1, -np.inf)):
        x = base.copy()
        x[at] = val
        out.append(Tr(name, (x, base.copy()), 44100))
    x = _rng("nan-tiles").uniform(-0.5, 0.5, L + 2 * t * H).astype(np.float32)
    x[t * H + 7] = np.nan  # in the last frame of tile 0 and the first of tile 1
    out.append(Tr("nan-across-tiles", (x,), 44100))
    x = base.copy()
    x[:] = np.nan
    out.append(Tr("nan-everywhere", (x,), 44100))
    out.append(Tr("beyond-full-scale", ((base * 6.0).astype(np.float32),), 44100))
    out.append(Tr("silence", (np.zeros(L + H, dtype=np.int16),), 44100))
    assert len({tr.name for tr in out}) == len(out)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def wants():
    """name -> [(E, analysed, skipped)] per channel."""
    return {tr.name: [want_plane(c) for c in tr.channels] for tr in tracks()}


def errors(e, ref):
    """(max_j |dE[j]| / sum E_ref, the worst relative error over the bands that hold at least 1e-4 of the total)."""
    total = float(ref.sum())
    if not total > 0.0:
        return (0.0 if not np.any(e) else float("inf")), 0.0
    d = np.abs(e - ref)
    big = ref >= 1e-4 * total
    return float(d.max() / total), float((d[big] / ref[big]).max()) if big.any() else 0.0


def measured():
    """(worst of total, worst relative) recorded by tools/spectrum_refcheck.py --record."""
    rec = json.loads(MEASURED.read_text())
    return float(rec["worst_of_total"]), float(rec["worst_relative"])


def got(r):
    return {"status": r.status, "flags": r.flags, "frames": r.frames, "sample_rate": r.sample_rate, "channels": r.channels, "format": r.format,
            "dropped_frames": r.dropped_frames, "cutoff_hz": r.cutoff_hz,
            "ch": [(c.cutoff_hz, c.edge_db, c.analysed_frames, c.skipped_frames, c.flags) for c in r.ch[:r.channels]]}
