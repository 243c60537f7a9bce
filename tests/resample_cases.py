"""The rational resampler and the cross-rate duplicate finder (include/mp3rgain_amd_resample.h): the cases the CPU and GPU
tests and tools/xrate_refcheck.py share, and references that do not depend on the new C++.

The plan and the window of an output restated in Python integers; a float64 reference of y (the header's signal, the f32 tap
table applied in float64 with numpy.dot); continuous-time pieces (decaying harmonic notes over a little independent noise)
rendered to 16 bits at any rate, so that "the same recording at another rate" needs no resampler to make.  Not part of the
product."""
import json
import sys
from collections import namedtuple
from functools import lru_cache
from math import gcd
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(Path(__file__).resolve().parent))

import fingerprint_cases as fc  # noqa: E402

from mp3rgain_amd import _capi  # noqa: E402

MEASURED = ROOT / "tests" / "golden" / "xrate_measured.json"
TOLERANCE_FACTOR = 4  # as fingerprint_cases takes it: for rounding the tool's cases did not meet
FC = 11025
Case = fc.Case
pack = fc.pack
signal = fc.signal
PLAN_RATES = (8000, 11025, 22050, 32000, 37800, 44100, 48000, 96000, 192000, 352800, 44056, 384000)
LENGTH_RATES = (22050, 44100, 48000, 32000, 8000)
PIECE_RATES = (44100, 48000, 96000, 32000, 22050, 8000)
DELAY_SECONDS = 0.1337
CODE_SECONDS = 512.0 / FC


# ---- the plan and the window in Python integers ----------------------------------------------------------------------------------
def plan(rate):
    """-> (L, M, P, supported), P = 0 when the rate is not supported."""
    g = gcd(rate, FC)
    L, M = FC // g, rate // g
    ok = rate >= 8000 and L <= 441 and M <= 32 * L
    if not ok:
        return L, M, 0, False
    if L == 1 and M == 1:
        return 1, 1, 1, True
    return L, M, 2 * 8 * max(L, M) // L + 1, True


def window(rate, j):
    """-> (b_j, p_j)"""
    L, M, _, _ = plan(rate)
    b = -((-j * M) // L)
    return b, b * L - j * M


def m_of(n, rate):
    """M_out of N frames: the number of j >= 0 with b_j + P <= N."""
    L, M, P, ok = plan(rate)
    return (n - P) * L // M + 1 if ok and n >= P else 0


def n_for(m, rate):
    """The shortest N that gives M_out = m (m >= 1)."""
    return window(rate, m - 1)[0] + plan(rate)[2]


# ---- cases -----------------------------------------------------------------------------------------------------------------------
@lru_cache(maxsize=None)
def cases():
    """Every length at which the kernel cuts differently, per rate, in the three formats and with 1, 2 and 3 channels: N is the
    shortest for its M_out unless said otherwise."""
    out = []
    seed = [700]

    def add(name, fmt, n, nch=1, rate=44100):
        planes = []
        for _ in range(nch):
            seed[0] += 1
            planes.append(fc.as_format(fc.noise(n, seed[0]), fmt))
        out.append(Case(f"{name}_r{rate}_{fmt}_{nch}ch", planes, rate))
        return planes

    for k, rate in enumerate(LENGTH_RATES):
        fmts = ("s16", "s32", "f32")
        f = lambda i: fmts[(i + k) % 3]  # noqa: E731  (every format meets every length over the rates)
        add("m0", f(0), n_for(1, rate) - 1, 1, rate)       # one sample short of the first window
        add("m1", f(1), n_for(1, rate), 2, rate)
        add("m255", f(2), n_for(255, rate), 1, rate)
        add("m256", f(0), n_for(256, rate), 2, rate)       # exactly one workgroup
        add("m257", f(1), n_for(257, rate), 3, rate)       # the third channel does not count
        add("m511", f(2), n_for(511, rate), 2, rate)
        add("m300_tail", f(0), n_for(301, rate) - 1, 1, rate)  # a tail that fills no output
    add("identity", "f32", 777, 2, 11025)
    add("identity", "s16", 300, 1, 11025)
    add("short", "s16", 5, 1, 48000)
    add("l7", "s32", n_for(600, 37800) + 2, 2, 37800)      # L = 7, M = 24
    add("r192k", "s16", n_for(258, 192000), 1, 192000)     # the longest staged span but one
    add("r352k", "f32", n_for(300, 352800), 2, 352800)     # L = 1, D = 32
    add("r96k", "s16", n_for(700, 96000), 2, 96000)
    add("unsupported", "s16", 5000, 1, 44056)
    add("unsupported", "f32", 5000, 2, 384000)
    # a float plane with a NaN inside: exactly the outputs whose windows hold it are NaN
    for rate in (48000, 44100, 8000):
        p = add("nan", "f32", n_for(600, rate), 2, rate)
        p[1][nan_at(rate)] = np.nan
    return tuple(out)


def nan_at(rate):
    return window(rate, 300)[0] + 3


def nan_outputs(rate, at, m):
    """The outputs j < m whose windows [b_j, b_j + P) hold sample `at`."""
    P = plan(rate)[2]
    return [j for j in range(m) if window(rate, j)[0] <= at < window(rate, j)[0] + P]


# ---- the float64 reference ----------------------------------------------------------------------------------------------------
def reference(case, table=None):
    """y in float64: the header's signal (f32), the f32 tap table of the library applied in float64."""
    import mp3rgain_amd as rg

    L, M, P, ok = plan(case.sample_rate)
    x = signal(case).astype(np.float64)
    m = m_of(len(x), case.sample_rate)
    if not ok or m == 0:
        return np.zeros(0)
    if L == 1 and M == 1:
        return x.copy()
    h = (rg.resample_filter(L, M) if table is None else table).astype(np.float64)
    y = np.zeros(m)
    with np.errstate(invalid="ignore"):
        for j in range(m):
            b, p = window(case.sample_rate, j)
            y[j] = np.dot(h[p], x[b:b + P])
    return y


def y_error(y, ref):
    """The largest |y - ref| relative to the track's largest |ref|, over the finite outputs; 0 for no output."""
    ok = np.isfinite(ref)
    if not ok.any():
        return 0.0
    top = np.abs(ref[ok]).max()
    return float(np.abs(y[ok].astype(np.float64) - ref[ok]).max() / (top if top > 0 else 1.0))


@lru_cache(maxsize=None)
def measured():
    with open(MEASURED) as f:
        return json.load(f)


# ---- continuous-time pieces ---------------------------------------------------------------------------------------------------
def piece(rate, seconds=8.0, delay=0.0, seed=1, noise_seed=None):
    """A piece defined in continuous time, rendered at `rate` to 16 bits: decaying harmonic notes, a new one every 0.23 s or so,
    plus a little noise that is independent from rendering to rendering.  `delay` seconds of silence come first."""
    rng = np.random.default_rng(9000 + seed)
    n = int(round(seconds * rate))
    x = np.zeros(n)
    start = 0.0
    while start < seconds:
        f0 = 110.0 * 2.0 ** (rng.integers(0, 36) / 12.0)
        dur = 0.15 + 0.5 * rng.random()
        amp = 1500.0 + 4000.0 * rng.random()
        phases = rng.random(6) * 2 * np.pi
        # a note sounds for 8 time constants: samples i with start <= i / rate - delay < start + 8 dur
        i0, i1 = int(np.ceil((start + delay) * rate - 1e-9)), min(n, int(np.ceil((start + delay + 8.0 * dur) * rate - 1e-9)))
        if i0 < i1:
            u = np.arange(i0, i1) / float(rate) - delay - start
            env = np.exp(-u / dur)
            for k in range(1, 7):
                if f0 * k < 3600.0:  # below the Nyquist frequency of every rendering
                    x[i0:i1] += env * amp / k * np.sin(2 * np.pi * f0 * k * u + phases[k - 1])
        start += 0.12 + 0.22 * rng.random()
    x += 20.0 * np.random.default_rng((noise_seed if noise_seed is not None else rate) + 31 * seed).standard_normal(n)
    return np.clip(np.rint(x), -32768, 32767).astype(np.int16)


@lru_cache(maxsize=None)
def behaviour_tracks():
    """-> [(name, rate, plane, delay in seconds, which recording)]: one piece at six rates, one of those again delayed by
    133.7 ms, and an unrelated piece."""
    out = [(f"piece_{r}", r, piece(r, seed=1), 0.0, 1) for r in PIECE_RATES]
    out.append(("piece_48000_delayed", 48000, piece(48000, delay=DELAY_SECONDS, seed=1, noise_seed=77), DELAY_SECONDS, 1))
    out.append(("other_44100", 44100, piece(44100, seed=2), 0.0, 2))
    return tuple(out)


def expected_lag(record_flags, delay_i, delay_j):
    """The lag in codes a pair record should carry: of the longer track (b) against the shorter (a)."""
    probe_j = bool(record_flags & _capi.FP_PAIR_PROBE_J)
    return ((delay_i - delay_j) if probe_j else (delay_j - delay_i)) / CODE_SECONDS


def xrate_codes(tracks, route=2, ctx=None):
    """The code arrays of (name, rate, plane, ..) tracks through rg_xrate_fingerprint_arena."""
    import mp3rgain_amd as rg

    cs = [Case(t[0], [t[2]], t[1]) for t in tracks]
    arena, descs = pack(cs)
    recs, codes, _, _ = rg.xrate_fingerprint_arena(ctx, route, descs, arena, bands=False)
    return [codes[r.codes_at:r.codes_at + r.codes] for r in recs], recs


def match(codes, **opts):
    """The existing stage 2 (host route) with every rate given as 11025 and this call's defaults."""
    import mp3rgain_amd as rg

    o = dict(block=_capi.XR_BLOCK, probes=_capi.XR_PROBES, radius=_capi.XR_RADIUS, max_ber_permille=_capi.XR_MAX_BER_PERMILLE)
    o.update(opts)
    return rg.fingerprint_match_codes(None, 0, codes, [FC] * len(codes), **o)
