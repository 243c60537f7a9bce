"""The checker of the EBU R 128 path: a plain float64 NumPy / SciPy restatement of the algorithm pinned down in
include/mp3rgain_amd_r128.h (ITU-R BS.1770 K-weighting, 400 ms blocks every 100 ms, both gates, true peak by a 49-tap
windowed-sinc interpolator).  It shares no code with the library: `scipy.signal.lfilter` runs the biquads, `np.convolve` the
interpolator.  Not part of the product.

`dtype=np.longdouble` runs the same recursion in extended precision (a plain loop-free restatement is not available for it, so
the two biquads are run by an explicit transposed direct form II loop): tools/r128_refcheck.py measures the float64 checker's
own error with it."""
import math

import numpy as np
from scipy.signal import lfilter

REFERENCE_LUFS = -18.0
ABS_GATE = 10.0 ** ((-70.0 + 0.691) / 10.0)
MIN_RATE, MAX_RATE = 8000, 384000


def coefficients(rate, dtype=np.float64):
    """((b1, a1), (b2, a2)): the shelf and the RLB high-pass at `rate`, from the analogue prototypes."""
    T = np.longdouble
    # the derivation is done in long double whichever precision the filter then runs in
    pi = np.arctan(T(1)) * 4
    f0, G, Q = T("1681.974450955533"), T("3.999843853973347"), T("0.7071752369554196")
    K = np.tan(pi * f0 / T(rate))
    Vh = T(10) ** (G / 20)
    Vb = Vh ** T("0.4996667741545416")
    a0 = 1 + K / Q + K * K
    b1 = [(Vh + Vb * K / Q + K * K) / a0, 2 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0]
    a1 = [T(1), 2 * (K * K - 1) / a0, (1 - K / Q + K * K) / a0]
    f0, Q = T("38.13547087602444"), T("0.5003270373238773")
    K = np.tan(pi * f0 / T(rate))
    a0 = 1 + K / Q + K * K
    b2 = [T(1), T(-2), T(1)]
    a2 = [T(1), 2 * (K * K - 1) / a0, (1 - K / Q + K * K) / a0]
    # the library's coefficients are doubles: round once, then widen again for the long double run
    rd = lambda v: np.array([np.float64(x) for x in v], dtype=np.float64).astype(dtype)  # noqa: E731
    return (rd(b1), rd(a1)), (rd(b2), rd(a2))


def hop_frames(rate):
    return (rate + 5) // 10


def tp_factor(rate):
    return 4 if rate < 96000 else 2 if rate < 192000 else 1


def block_count(rate, frames):
    H = frames // hop_frames(rate)
    return max(H - 3, 0)


def normalise(x, dtype=np.float64):
    """Full scale 1.0: float32 as is, int16 / 32768, int32 / 2^31."""
    x = np.asarray(x)
    if x.dtype == np.int16:
        return x.astype(dtype) / dtype(32768.0)
    if x.dtype == np.int32:
        return x.astype(dtype) / dtype(2147483648.0)
    return x.astype(dtype)


def _biquad_loop(b, a, x):
    """Transposed direct form II, the structure lfilter uses, in the dtype of x (for np.longdouble)."""
    y = np.empty_like(x)
    s1 = s2 = x.dtype.type(0)
    b0, b1, b2 = b
    _, a1, a2 = a
    for n in range(len(x)):
        xn = x[n]
        yn = b0 * xn + s1
        s1 = b1 * xn - a1 * yn + s2
        s2 = b2 * xn - a2 * yn
        y[n] = yn
    return y


def k_weight(x, rate, dtype=np.float64):
    (b1, a1), (b2, a2) = coefficients(rate, dtype)
    if dtype is np.float64:
        return lfilter(b2, a2, lfilter(b1, a1, x))
    return _biquad_loop(b2, a2, _biquad_loop(b1, a1, x))


def hop_energies(channels, rate, dtype=np.float64):
    """e[h]: sum over channels 0 and 1 of the sum of squares of the K-weighted samples of hop h; a partial hop is dropped."""
    hop = hop_frames(rate)
    chans = list(channels)[:2]
    H = len(chans[0]) // hop
    e = np.zeros(H, dtype=dtype)
    for c in chans:
        y = k_weight(normalise(c, dtype), rate, dtype)[:H * hop]
        e += (y * y).reshape(H, hop).sum(axis=1) if H else 0
    return e


def block_z(channels, rate, dtype=np.float64):
    e = hop_energies(channels, rate, dtype)
    hop = hop_frames(rate)
    if len(e) < 4:
        return np.zeros(0, dtype=dtype)
    return (e[:-3] + e[1:-2] + e[2:-1] + e[3:]) / dtype(4 * hop)


def gate(z):
    """-> (loudness_lufs, blocks kept by both gates, relative threshold)."""
    z = np.asarray(z, dtype=np.float64)
    kept = z[z >= ABS_GATE]
    if len(kept) == 0:
        return -math.inf, 0, ABS_GATE
    thr = 0.1 * kept.mean()
    both = kept[kept >= thr]
    if len(both) == 0:
        return -math.inf, 0, thr
    return -0.691 + 10.0 * math.log10(both.mean()), len(both), thr


def gain_from(lufs):
    return 0.0 if lufs == -math.inf else REFERENCE_LUFS - lufs


def finite(channels):
    return all(bool(np.all(np.isfinite(np.asarray(c, dtype=np.float64)))) for c in list(channels)[:2])


def sample_peak(channels):
    m = 0.0
    for c in list(channels)[:2]:
        x = np.abs(normalise(c))
        x = x[np.isfinite(x)]
        if len(x):
            m = max(m, float(x.max()))
    return m


def tp_taps(F):
    j = np.arange(49, dtype=np.float64)
    return np.sinc((j - 24.0) / F) * 0.5 * (1.0 - np.cos(2.0 * np.pi * j / 48.0))


def true_peak(channels, rate):
    F = tp_factor(rate)
    if F == 1:
        return sample_peak(channels)
    h = tp_taps(F)
    m = 0.0
    for c in list(channels)[:2]:
        x = normalise(c)
        if len(x) == 0:
            continue
        u = np.zeros(len(x) * F, dtype=np.float64)
        u[::F] = x
        y = np.abs(np.convolve(u, h))
        y = y[np.isfinite(y)]
        if len(y):
            m = max(m, float(y.max()))
    return m


def analyze(channels, rate, want_true_peak=False):
    """One track -> dict with the fields of rg_r128_track_result (+ the block values)."""
    if not finite(channels):
        z = np.zeros(0)
        lufs, kept, gain = math.nan, 0, math.nan
    else:
        z = block_z(channels, rate)
        lufs, kept, _ = gate(z)
        gain = gain_from(lufs)
    return {"loudness_lufs": lufs, "gain_db": gain, "sample_peak": sample_peak(channels),
            "true_peak": true_peak(channels, rate) if want_true_peak else math.nan, "blocks": block_count(rate, len(channels[0])),
            "blocks_gated": kept, "z": z}


def analyze_album(tracks, want_true_peak=False):
    """tracks: [(channels, rate)] -> (per-track dicts, album dict): both gates over the union of the tracks' blocks."""
    res = [analyze(ch, rate, want_true_peak) for ch, rate in tracks]
    if any(math.isnan(r["loudness_lufs"]) for r in res):
        lufs, kept, gain = math.nan, 0, math.nan
        z = np.zeros(0)
    else:
        z = np.concatenate([r["z"] for r in res]) if res else np.zeros(0)
        lufs, kept, _ = gate(z)
        gain = gain_from(lufs)
    album = {"loudness_lufs": lufs, "gain_db": gain, "sample_peak": max([r["sample_peak"] for r in res], default=0.0),
             "true_peak": max([r["true_peak"] for r in res], default=0.0) if want_true_peak else math.nan,
             "blocks": sum(r["blocks"] for r in res), "blocks_gated": kept, "z": z}
    return res, album


# ---- EBU Tech 3341 test signals ------------------------------------------------------------------------------------------
def sine_segments(rate, segments, freq=1000.0, channels=2):
    """segments: [(seconds, dBFS peak)] -> `channels` identical float64 channels, phase continuous."""
    parts, n0 = [], 0
    for secs, db in segments:
        n = int(round(secs * rate))
        t = (n0 + np.arange(n)) / rate
        parts.append(10.0 ** (db / 20.0) * np.sin(2.0 * np.pi * freq * t))
        n0 += n
    x = np.concatenate(parts)
    return [x.copy() for _ in range(channels)]


TECH3341_LOUDNESS = [
    ("case1", [(20, -23.0)], -23.0),
    ("case2", [(20, -33.0)], -33.0),
    ("case3", [(10, -36.0), (60, -23.0), (10, -36.0)], -23.0),
    ("case4", [(10, -72.0), (10, -36.0), (60, -23.0), (10, -36.0), (10, -72.0)], -23.0),
    ("case5", [(20, -26.0), (20.1, -20.0), (20, -26.0)], -23.0),
]

# Tech 3341 cases 15-19: (name, rate divisor, phase in degrees, amplitude)
TECH3341_TRUEPEAK = [
    ("case15", 4, 0.0, 0.50),
    ("case16", 4, 45.0, 0.50),
    ("case17", 6, 60.0, 0.50),
    ("case18", 8, 67.5, 0.50),
    ("case19", 4, 45.0, 1.41),
]


def truepeak_signal(rate, divisor, phase_deg, amplitude, seconds=1.0):
    """A sine at rate / divisor with a 10 ms raised-cosine fade at both ends (one channel, float64)."""
    n = int(round(seconds * rate))
    k = np.arange(n)
    x = amplitude * np.sin(2.0 * np.pi * k / divisor + math.radians(phase_deg))
    nf = int(round(0.010 * rate))
    ramp = 0.5 * (1.0 - np.cos(np.pi * (np.arange(nf) + 0.5) / nf))
    x[:nf] *= ramp
    x[-nf:] *= ramp[::-1]
    return x
