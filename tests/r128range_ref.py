"""The checker of loudness range (EBU Tech 3342) and of the momentary / short-term maxima: a plain float64 NumPy restatement
of the definitions in include/mp3rgain_amd_r128.h, on top of the hop energies of tests/r128ref.py.  Every short-term block is
a direct sum of its 30 hop energies; the percentiles are elements of the sorted block list at integer ranks.  It shares no
code with the library.  Not part of the product.

`dtype=np.longdouble` runs the hop energies and the sums in extended precision: tools/r128_range_refcheck.py measures the
float64 checker's own error with it."""
import math
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent))
import r128ref  # noqa: E402

ABS_GATE = r128ref.ABS_GATE
ST_HOPS = 30


def short_term_count(rate, frames):
    H = frames // r128ref.hop_frames(rate)
    return max(H - (ST_HOPS - 1), 0)


def short_term_from(e, rate):
    """st[s] = (e[s] + ... + e[s + 29]) / (30 hop), the 30 terms added one after another in ascending order."""
    n = len(e) - (ST_HOPS - 1)
    if n <= 0:
        return np.zeros(0, dtype=e.dtype)
    s = e[0:n].copy()
    for k in range(1, ST_HOPS):
        s = s + e[k:k + n]
    return s / e.dtype.type(ST_HOPS * r128ref.hop_frames(rate))


def short_term(channels, rate, dtype=np.float64):
    return short_term_from(r128ref.hop_energies(channels, rate, dtype), rate)


def lufs(ms):
    return -0.691 + 10.0 * math.log10(ms) if ms > 0.0 else -math.inf


def ranks(n):
    return (10 * (n - 1) + 50) // 100, (95 * (n - 1) + 50) // 100


def loudness_range(st):
    """-> dict: loudness_range_lu, range_low_lufs, range_high_lufs, st_blocks, st_blocks_gated, thr (the relative threshold
    as a mean square), low, high (the two selected blocks)."""
    st = np.asarray(st, dtype=np.float64)
    out = {"loudness_range_lu": 0.0, "range_low_lufs": -math.inf, "range_high_lufs": -math.inf, "st_blocks": len(st),
           "st_blocks_gated": 0, "thr": ABS_GATE, "low": 0.0, "high": 0.0}
    A = st[st >= ABS_GATE]
    if len(A) == 0:
        return out
    thr = 0.01 * float(A.mean())
    out["thr"] = thr
    K = np.sort(A[A >= thr])
    n = len(K)
    if n == 0:
        return out
    lo, hi = ranks(n)
    low, high = float(K[lo]), float(K[hi])
    out.update(loudness_range_lu=10.0 * math.log10(high / low), range_low_lufs=lufs(low), range_high_lufs=lufs(high),
               st_blocks_gated=n, low=low, high=high)
    return out


_NAN5 = {"loudness_range_lu": math.nan, "range_low_lufs": math.nan, "range_high_lufs": math.nan, "max_momentary_lufs": math.nan,
         "max_short_term_lufs": math.nan, "st_blocks_gated": 0}


def analyze(channels, rate):
    """One track -> dict with the fields of rg_r128_dynamics (+ "st", "z": the block values; "thr", "low", "high")."""
    frames = len(channels[0])
    if not r128ref.finite(channels):
        return dict(_NAN5, st_blocks=short_term_count(rate, frames), st=np.zeros(0), z=np.zeros(0), thr=ABS_GATE, finite=False)
    e = r128ref.hop_energies(channels, rate)
    st = short_term_from(e, rate)
    z = r128ref.block_z(channels, rate)
    out = loudness_range(st)
    out.update(max_momentary_lufs=lufs(float(z.max())) if len(z) else -math.inf,
               max_short_term_lufs=lufs(float(st.max())) if len(st) else -math.inf, st=st, z=z, finite=True)
    return out


def analyze_album(tracks):
    """tracks: [(channels, rate)] -> (per-track dicts, album dict): both gates and the selection over the union of the tracks'
    short-term blocks in track order; the maxima are the maxima over the tracks."""
    res = [analyze(ch, rate) for ch, rate in tracks]
    total = sum(r["st_blocks"] for r in res)
    if not all(r["finite"] for r in res):
        return res, dict(_NAN5, st_blocks=total, st=np.zeros(0), thr=ABS_GATE)
    st = np.concatenate([r["st"] for r in res]) if res else np.zeros(0)
    album = loudness_range(st)
    album.update(max_momentary_lufs=max([r["max_momentary_lufs"] for r in res], default=-math.inf),
                 max_short_term_lufs=max([r["max_short_term_lufs"] for r in res], default=-math.inf), st=st)
    return res, album


# ---- EBU Tech 3342 test signals: a stereo 1 kHz sine in 20 s segments (name, [(seconds, dBFS)], expected LRA in LU, +- 1) ----
TECH3342 = [
    ("case1", [(20, -20.0), (20, -30.0)], 10.0),
    ("case2", [(20, -20.0), (20, -15.0)], 5.0),
    ("case3", [(20, -40.0), (20, -20.0)], 20.0),
    ("case4", [(20, -50.0), (20, -35.0), (20, -20.0), (20, -35.0), (20, -50.0)], 15.0),
]


def tech3342_signal(rate, segments):
    return r128ref.sine_segments(rate, segments)
