"""The key scan (include/mp3rgain_amd_key.h): the cases the CPU and GPU tests and tools/key_refcheck.py share, and references
that do not depend on the new C++.

Stage 1: a float64 reference -- the signal as the header defines it (f32 sample values, the f32 mean of the first two
channels), the filter's f32 table applied in float64, numpy.fft.rfft with the spectral scan's window as a float table, float64
band sums, then q and the rows in integers.  Stage 2: the header's definitions restated in Python integers (`ref_stage2`),
which the serial host twin has to equal byte for byte, constructed rows, and the synthetic chord progressions with their
generating key.  Not part of the product."""
import json
import sys
from collections import namedtuple
from functools import lru_cache
from math import isqrt
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(Path(__file__).resolve().parent))

import fingerprint_cases as fc  # noqa: E402
import tempo_cases as tc  # noqa: E402

from mp3rgain_amd import _capi  # noqa: E402

MEASURED = ROOT / "tests" / "golden" / "key_measured.json"
TOLERANCE_FACTOR = 4  # as the spectrum, fingerprint and tempo tests take it: for rounding the tool's cases did not meet
L, H, BANDS, CHROMA, RANGE = 4096, 512, 60, 12, 160
Case = fc.Case
pack = fc.pack
signal = fc.signal
q_of = tc.q_of
MAJOR = (656, -286, -1, -263, 205, 139, -220, 390, -250, 41, -273, -138)
MINOR = (654, -257, -47, 418, -277, -45, -292, 260, 68, -255, -92, -135)


def shape():
    import mp3rgain_amd as rg

    return rg.key_kernel_shape()


def decim_of(rate):
    return rate // 5000


def taps_of(D):
    return 16 * D + 1


def n_for(m, D):
    """The shortest N that gives M = m decimated samples (m >= 1)."""
    return m if D == 1 else (m - 1) * D + taps_of(D)


def m_of(n, D):
    if D == 1:
        return n
    return 0 if n < taps_of(D) else (n - taps_of(D)) // D + 1


def chord(n, rate, notes=(48, 52, 55), amp=6000.0, seed=0):
    """MIDI notes as sines with three harmonics over a little noise, in 16-bit LSB units (float64)."""
    t = np.arange(n) / float(rate)
    x = 20.0 * np.random.default_rng(seed).standard_normal(n)
    for note in notes:
        f = 440.0 * 2.0 ** ((note - 69) / 12.0)
        for k in (1, 2, 3):
            x += amp / k * np.sin(2 * np.pi * f * k * t + 0.1 * note)
    return x


# ---- stage 1: cases ------------------------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def cases():
    """Every shape the kernels cut differently, in the three formats: N is the shortest for its M unless said otherwise."""
    W, _, T, _, _ = shape()
    out = []
    seed = [500]

    def add(name, fmt, n, nch=1, rate=44100):
        planes = []
        for _ in range(nch):
            seed[0] += 1
            planes.append(fc.as_format(fc.noise(n, seed[0]), fmt))
        out.append(Case(f"{name}_{fmt}_{nch}ch", planes, rate))
        return planes

    D = 8
    for fmt in ("s16", "s32", "f32"):
        add("n16D", fmt, 16 * D)                           # M = 0
        add("m1", fmt, 16 * D + 1, 2)                      # M = 1
        add("m4095", fmt, n_for(4095, D))                  # F = 0
        add("m4096", fmt, n_for(4096, D) + D - 1)          # F = 1, and a tail that makes no output
        add("m4096", fmt, n_for(4096, D), 3)               # the third channel does not count
        add(f"f{T + 1}", fmt, n_for(L + T * H, D))         # F - 1 = T: exactly one tile
        add(f"f{T + 2}", fmt, n_for(L + (T + 1) * H + 100, D), 2)  # one tile + 1
        add(f"f{2 * T}", fmt, n_for(L + (2 * T - 1) * H, D))       # two tiles - 1
        add(f"m{2 * W}", fmt, n_for(2 * W, D), 2)          # a decimation workgroup's run ends with the track
        add(f"m{2 * W + 1}", fmt, n_for(2 * W + 1, D))     # ... and one output more
    p = add("nonfinite", "f32", n_for(L + (T + 2) * H, D), 2)
    p[0][n_for(L + 3 * H, D)] = np.nan                     # an input NaN reaches 17 outputs
    p[1][5] = np.inf                                       # the first outputs: frames 0 ..
    for rate, fmt, nch in ((8000, "s16", 2), (8000, "f32", 1), (48000, "s32", 2), (48000, "s16", 1), (192000, "s16", 1), (192000, "f32", 2)):
        add(f"rate{rate}", fmt, n_for(L + 2 * H + 3, decim_of(rate)), nch, rate)
    add("rate8000_m255", "s16", 255, 1, 8000)
    add("rate4000", "s16", 6000, 1, 4000)                  # D = 0: RG_KEY_RATE
    add("rate410000", "f32", 5000, 2, 410000)              # D = 82: RG_KEY_RATE
    for fmt in ("s16", "f32"):
        add("silence", fmt, n_for(L + 3 * H, D))[0][:] = 0
        s = add("silence_then_chord", fmt, n_for(L + 20 * H, D), 2)
        for ch in s:
            ch[:] = fc.as_format(chord(len(ch), 44100), fmt)
            ch[:n_for(L + 4 * H, D)] = 0                   # rows 0 .. 4 are silent
    two = add("chord_2s", "s16", 88200, 2)
    for ch in two:
        ch[:] = fc.as_format(chord(88200, 44100, (45, 48, 52, 57)), "s16")
    return tuple(out)


# ---- stage 1: the float64 reference ---------------------------------------------------------------------------------------------
def bands_of(rate):
    """-> (D, e[0 .. 60] as the header's formula gives them or None, whether the rate is supported)."""
    D = decim_of(rate) if rate else 0
    if D < 1 or D > 80:
        return D, None, False
    fd = float(rate) / D
    e = [int(np.floor(440.0 * 2.0 ** ((s - 33.5) / 12.0) * L / fd + 0.5)) for s in range(BANDS + 1)]
    e[0] = max(e[0], 1)
    for s in range(1, BANDS + 1):
        e[s] = max(e[s], e[s - 1] + 1)
    return D, e, e[BANDS] <= L // 2


def filter_of(D):
    """The header's filter in float64, normalised, rounded to f32."""
    half = 8 * D
    n = np.arange(-half, half + 1, dtype=np.float64)
    fc_ = 0.45 / D
    h = 2 * fc_ * np.sinc(2 * fc_ * n) * (0.42 + 0.5 * np.cos(np.pi * n / half) + 0.08 * np.cos(2 * np.pi * n / half))
    return (h / h.sum()).astype(np.float32)


def rows_of(E):
    """The chroma rows of band energies E[F][60] -> uint16[F][12]."""
    E = np.asarray(E)
    if not len(E):
        return np.zeros((0, CHROMA), np.uint16)
    q = q_of(E)
    qmax = q.max(axis=1, keepdims=True)
    v = np.maximum(q - (qmax - RANGE), 0)
    v[(qmax == int(q_of(np.zeros(1))[0]))[:, 0]] = 0
    return v.reshape(len(E), BANDS // CHROMA, CHROMA).sum(axis=1).astype(np.uint16)


Ref = namedtuple("Ref", "decim y frames rows bands nonfinite supported")


def reference_signal(x, rate, taps=None):
    """The float64 reference of a down-mixed f32 signal x -> Ref.  `taps`: the library's table (the test of the table against
    filter_of is separate); None: filter_of."""
    D, e, ok = bands_of(rate)
    if not ok:
        return Ref(D if D <= 80 else D, np.zeros(0), 0, np.zeros((0, CHROMA), np.uint16), np.zeros((0, BANDS)), 0, False)
    x64 = np.asarray(x, dtype=np.float64)
    if D == 1:
        y = x64
    else:
        h = (filter_of(D) if taps is None else np.asarray(taps)).astype(np.float64)
        M = m_of(len(x64), D)
        with np.errstate(invalid="ignore", over="ignore"):
            if M and not np.isfinite(x64).all():
                y = np.array([np.dot(h, x64[j * D:j * D + len(h)]) for j in range(M)])
            else:
                y = np.convolve(x64, h[::-1], mode="valid")[::D][:M] if M else np.zeros(0)
    with np.errstate(over="ignore", invalid="ignore"):
        y32 = y.astype(np.float32).astype(np.float64)  # a frame is non-finite when a y of the f32 signal is
    F = 0 if len(y) < L else (len(y) - L) // H + 1
    if F == 0:
        return Ref(D, y, 0, np.zeros((0, CHROMA), np.uint16), np.zeros((0, BANDS)), 0, True)
    win = (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(L) / L)).astype(np.float32).astype(np.float64)
    frames = np.lib.stride_tricks.sliding_window_view(y32, L)[::H][:F]
    bad = ~np.isfinite(frames).all(axis=1)
    with np.errstate(invalid="ignore"):
        P = np.abs(np.fft.rfft(np.where(bad[:, None], 0.0, frames) * win, axis=1)) ** 2
    E = np.stack([P[:, e[s]:e[s + 1]].sum(axis=1) for s in range(BANDS)], axis=1)
    E[bad] = 0.0
    return Ref(D, y, F, rows_of(E), E, int(bad.sum()), True)


def reference(case):
    return reference_signal(signal(case), case.sample_rate)


def band_error(E, ref):
    return fc.band_error(E, ref)


def y_error(y, ref):
    """The largest |y - ref| relative to the largest |ref|, over the finite reference values; 0 for no output."""
    ok = np.isfinite(ref)
    if not ok.any():
        return 0.0
    top = np.abs(ref[ok]).max()
    return float(np.abs(np.asarray(y, dtype=np.float64)[ok] - ref[ok]).max() / (top if top > 0 else 1.0))


@lru_cache(maxsize=None)
def measured():
    with open(MEASURED) as f:
        return json.load(f)


# ---- stage 2: the definitions restated -----------------------------------------------------------------------------------------
FIELDS = ("flags", "rows", "silent_rows", "key", "tonic", "mode", "correlation_permille", "margin_permille", "segments", "stable_permille")


def pick(Hsum):
    """-> (key, correlation, margin) or None, from twelve Python integers."""
    top = max(Hsum)
    sh = 0
    while (top >> sh) >= 65536:
        sh += 1
    h = [int(v) >> sh for v in Hsum]
    score = [sum(h[p] * (MINOR if k // 12 else MAJOR)[(p - k % 12) % 12] for p in range(12)) for k in range(24)]
    best = max(range(24), key=lambda k: (score[k], -k))
    vh = 12 * sum(v * v for v in h) - sum(h) ** 2
    den = isqrt(1000000 * vh // 12)
    if den == 0 or score[best] <= 0:
        return None
    second = max(score[k] for k in range(24) if k != best)
    return best, max(0, min(1000, 1000 * score[best] // den)), max(0, min(1000, 1000 * (score[best] - second) // score[best]))


def ref_stage2(rows, segment=None):
    """-> dict of FIELDS.  `flags` without COMPLETE, NONFINITE and RATE, which stage 2 does not know."""
    S = segment or _capi.KEY_SEGMENT
    c = np.asarray(rows, dtype=np.int64).reshape(-1, CHROMA)
    F = len(c)
    out = dict.fromkeys(FIELDS, 0)
    out["rows"] = F
    if not F:
        out["flags"] = _capi.KEY_SHORT
        return out
    out["silent_rows"] = int((c.sum(axis=1) == 0).sum())
    out["segments"] = F // S
    p = pick([int(v) for v in c.sum(axis=0)])
    if p is None:
        out["flags"] = _capi.KEY_NONE
        return out
    nonzero = agreeing = 0
    for g in range(F // S):
        Hg = [int(v) for v in c[g * S:(g + 1) * S].sum(axis=0)]
        if not any(Hg):
            continue
        nonzero += 1
        pg = pick(Hg)
        agreeing += pg is not None and pg[0] == p[0]
    out.update(key=p[0], tonic=p[0] % 12, mode=p[0] // 12, correlation_permille=p[1], margin_permille=p[2],
               stable_permille=1000 * agreeing // nonzero if nonzero else 0)
    return out


def record_fields(r, mask=~(_capi.KEY_COMPLETE | _capi.KEY_NONFINITE | _capi.KEY_RATE)):
    d = {f: int(getattr(r, f)) for f in FIELDS}
    d["flags"] &= mask
    return d


def profile_rows(key, count, seed, scale=1.0, noise=20):
    """Rows that look like `key`: its profile shifted to be non-negative, with a little noise."""
    rng = np.random.default_rng(seed)
    prof = np.array(MINOR if key // 12 else MAJOR)
    base = np.roll((prof - prof.min()) * 0.5 * scale, key % 12)
    return np.clip(np.rint(base + rng.integers(0, noise + 1, size=(count, CHROMA))), 0, 800).astype(np.uint16)


ChromaCase = namedtuple("ChromaCase", "name rows segment")


@lru_cache(maxsize=None)
def chroma_cases():
    """Constructed rows with their segment length."""
    out = []
    one = np.zeros((40, CHROMA), np.uint16)
    one[:, 7] = 500
    out.append(ChromaCase("one_pitch_class", (one,), 8))
    out.append(ChromaCase("flat", (np.full((40, CHROMA), 321, np.uint16),), 8))            # every score 0: key 0, Vh = 0: NONE
    out.append(ChromaCase("zeros", (np.zeros((40, CHROMA), np.uint16),), 8))
    out.append(ChromaCase("rows_800_shift", (np.vstack([np.full((300, CHROMA), 800, np.uint16), profile_rows(14, 300, 1, 1.6)]),), 128))  # H >= 65536: sh > 0
    out.append(ChromaCase("all_800_long", (np.full((700, CHROMA), 800, np.uint16),), 128))  # flat after the shift too
    out.append(ChromaCase("key_change", (np.vstack([profile_rows(0, 64, 2), profile_rows(0, 64, 3), profile_rows(6, 64, 4)]),), 64))
    out.append(ChromaCase("below_one_segment", (profile_rows(21, 127, 5),), 128))           # G = 0: stable 0
    out.append(ChromaCase("one_segment", (profile_rows(21, 128, 6),), 128))
    z = profile_rows(9, 96, 7)
    z[32:64] = 0
    out.append(ChromaCase("a_silent_segment", (z,), 32))                                     # two non-zero segments of three
    out.append(ChromaCase("every_key", tuple(profile_rows(k, 50 + k, 10 + k) for k in range(24)), 16))
    out.append(ChromaCase("more_rows_than_lanes", (profile_rows(17, 1000, 40), np.zeros((0, CHROMA), np.uint16), profile_rows(3, 257, 41)), 8))
    out.append(ChromaCase("segments_beyond_the_lanes", (profile_rows(5, 8 * 300 + 5, 42),), 8))  # 300 segments: a lane owns two
    out.append(ChromaCase("n0", (), 8))
    return tuple(out)


# ---- the tonal material --------------------------------------------------------------------------------------------------------
TRUTH_RATES = (44100, 48000, 96000)
TRUTH_SECONDS = 40
MAJOR_SCALE = (0, 2, 4, 5, 7, 9, 11)
MINOR_SCALE = (0, 2, 3, 5, 7, 8, 10)
PROGRESSION = (0, 3, 4, 0, 5, 3, 4, 0)  # scale degrees: I-IV-V-I-vi-IV-V-I (minor: i-iv-v-i-VI-iv-v-i)


def _tone(f, t, tau):
    """Six harmonics at 1 / k with a decaying envelope."""
    z = np.exp(2j * np.pi * f * t)
    w = z.copy()
    x = w.imag.copy()
    for k in range(2, 7):
        w *= z
        x += w.imag / k
    return x * np.exp(-t / tau)


def progression(key, rate, seconds=TRUTH_SECONDS, seed=3):
    """A bass root plus triads over PROGRESSION, a scale-tone melody, decaying envelopes and a little noise -> float64 in
    [-1, 1]."""
    rng = np.random.default_rng(seed + key)
    scale = MINOR_SCALE if key // 12 else MAJOR_SCALE
    tonic = key % 12
    n = int(seconds * rate)
    x = 1e-3 * rng.standard_normal(n)
    per = n // len(PROGRESSION)

    def midi(degree, octave):
        return 12 * (octave + 1) + tonic + scale[degree % 7] + 12 * (degree // 7)

    def put(at, note, dur, amp, tau):
        m = min(int(dur * rate), n - at)
        if m > 0:
            x[at:at + m] += amp * _tone(440.0 * 2.0 ** ((note - 69) / 12.0), np.arange(m) / float(rate), tau)

    for c, deg in enumerate(PROGRESSION):
        a = c * per
        for beat in range(4):  # the chord struck four times
            at = a + beat * per // 4
            put(at, midi(deg, 2), per / 4 / rate, 0.25, 0.6)
            for third in (0, 2, 4):
                put(at, midi(deg + third, 3 if tonic < 7 else 2) + 12, per / 4 / rate, 0.12, 0.5)
        for step in range(8):  # the melody: scale tones
            put(a + step * per // 8, midi(int(rng.integers(0, 7)), 5 if tonic < 7 else 4), per / 8 / rate, 0.08, 0.25)
    return np.clip(x, -1.0, 1.0)


def truth_cases():
    """(rate, key) of the 72 cases."""
    return [(rate, key) for rate in TRUTH_RATES for key in range(24)]


@lru_cache(maxsize=None)
def truth_planes(rate, key):
    return fc.as_format(progression(key, rate) * 32768.0 * 0.9, "s16")


@lru_cache(maxsize=None)
def white_noise(rate, seconds=TRUTH_SECONDS):
    return fc.as_format(np.random.default_rng(99).standard_normal(int(seconds * rate)) * 3000.0, "s16")
