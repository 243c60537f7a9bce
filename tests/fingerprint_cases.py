"""The duplicate finder (include/mp3rgain_amd_fingerprint.h): the cases the CPU and GPU tests and tools/fingerprint_refcheck.py
share, and references that do not depend on the new C++.

Stage 1: a float64 reference from numpy.fft.rfft -- the signal as the header defines it (f32 sample values, the f32 mean of
the first two channels), the spectral scan's window as a float table, float64 from there on: band energies, the code bits and
each bit's margin.  Stage 2: the match restated in numpy integers (`ref_match`), which the serial host twin has to equal byte
for byte, and constructed codes with planted copies.  Not part of the product."""
import json
import sys
from collections import namedtuple
from functools import lru_cache
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

from mp3rgain_amd import _capi  # noqa: E402

MEASURED = ROOT / "tests" / "golden" / "fingerprint_measured.json"
TOLERANCE_FACTOR = 4  # as the spectrum tests take it: for rounding the tool's cases did not meet
L, H, BANDS = 4096, 512, 33

Case = namedtuple("Case", "name channels sample_rate")
PAIR = np.dtype([("errors", "<u4"), ("bits", "<u4"), ("lag", "<i4"), ("flags", "<u4")])


# ---- stage 1: signals and cases ------------------------------------------------------------------------------------------------
def noise(n, seed, amp=3000.0):
    """Music-like and cheap: white noise through a short decaying kernel plus two tones, in 16-bit LSB units (float64)."""
    rng = np.random.default_rng(seed)
    w = rng.standard_normal(n + 63)
    y = np.convolve(w, 0.9 ** np.arange(64), mode="valid")
    t = np.arange(n)
    f1, f2 = 300.0 + 37.0 * (seed % 40), 900.0 + 53.0 * (seed % 19)
    return amp * (y / np.std(y) + 0.5 * np.sin(2 * np.pi * f1 * t / 44100.0) + 0.3 * np.sin(2 * np.pi * f2 * t / 44100.0 + 0.3))


def as_format(x, fmt):
    """x in 16-bit LSB units -> a plane of `fmt` ("s16", "s32", "f32"); s32 keeps 24 bits and some below."""
    if fmt == "s16":
        return np.clip(np.rint(x), -32768, 32767).astype(np.int16)
    if fmt == "s32":
        return np.clip(np.rint(x * 65536.0), -2 ** 31, 2 ** 31 - 1).astype(np.int32)
    return (x / 32768.0).astype(np.float32)


def tile_codes():
    import mp3rgain_amd as rg

    return rg.fingerprint_kernel_shape()[0]


@lru_cache(maxsize=None)
def cases():
    """Every shape the kernels cut differently, in the three formats.  N = L + H K + a tail that fills no frame."""
    T = tile_codes()
    out = []
    seed = [100]

    def add(name, fmt, n, nch=1, rate=44100):
        planes = []
        for _ in range(nch):
            seed[0] += 1
            planes.append(as_format(noise(n, seed[0]), fmt))
        out.append(Case(f"{name}_{fmt}_{nch}ch", planes, rate))
        return planes

    for fmt in ("s16", "s32", "f32"):
        add("n4095", fmt, 4095)              # F = 0
        add("n4096", fmt, 4096)              # F = 1, K = 0
        add("n4608", fmt, 4608)              # K = 1
        add("n4608", fmt, 4608, 2)
        add("n4608", fmt, 4608, 3)           # the third channel does not count
        add("k2_tail", fmt, L + 2 * H + 100)  # F = 3: odd, the last pair has one frame
        add("k3", fmt, L + 3 * H, 2)         # F = 4: even
        add(f"k{T}", fmt, L + T * H)         # exactly one tile of codes
        add(f"k{T + 1}", fmt, L + (T + 1) * H + 511, 2)  # one tile + 1
        add(f"k{2 * T - 1}", fmt, L + (2 * T - 1) * H)   # two tiles - 1
    # a float plane with a NaN in one frame and an Inf in the last; 2 channels: the Inf is in the second
    p = add("nonfinite", "f32", L + (2 * T + 2) * H + 7, 2)
    p[0][L + 3 * H + 5] = np.nan            # frames 4 .. 11 hold it
    p[1][-8] = np.inf                        # the last frame only
    q = add("nan_first", "f32", L + 3 * H)
    q[0][3] = np.nan                         # frame 0 only
    for rate in (8000, 44100, 48000, 88200, 96000):
        add(f"rate{rate}", "s16", L + 3 * H, 1, rate)
    add("rate8000", "f32", L + (T + 2) * H, 2, 8000)
    add("music_2s", "s16", 88200, 2)         # enough codes for the flipped-bit share to mean something
    return tuple(out)


def pack(case_list):
    """The cases in one host arena, abutting at sample alignment -> (arena, descs)."""
    import arena_layouts as al

    Tr = namedtuple("Tr", "channels sample_rate")
    arena, descs, _ = al.pack([Tr(list(c.channels), c.sample_rate) for c in case_list], al.Layout("abut", "loud", "input"))
    return arena, list(descs)[:len(case_list)]


# ---- stage 1: the float64 reference ---------------------------------------------------------------------------------------------
def edges(rate):
    """-> (e[0 .. 33] as the header's formula gives them, whether the rate is supported)."""
    e = [int(np.floor(300.0 * (2000.0 / 300.0) ** (m / 33.0) * L / float(rate) + 0.5)) for m in range(BANDS + 1)]
    return e, all(b > a for a, b in zip(e, e[1:])) and e[0] >= 1 and e[BANDS] <= L // 2


def signal(case):
    """The header's signal: f32 sample values, the f32 mean of the first two channels."""
    def value(p):
        if p.dtype == np.int16:
            return p.astype(np.float32) * np.float32(1.0 / 32768.0)
        if p.dtype == np.int32:
            return p.astype(np.float32) * np.float32(1.0 / 2147483648.0)
        return p.astype(np.float32)

    with np.errstate(invalid="ignore", over="ignore"):
        a = value(case.channels[0])
        return (a + value(case.channels[1])) * np.float32(0.5) if len(case.channels) >= 2 else a


Ref = namedtuple("Ref", "frames codes bands margins nonfinite supported")


def reference(case):
    """-> Ref: F, the K codes (uint32), E[F][33] (float64), margins[K][32] = |d| / (the two frames' band energy), the
    number of non-finite frames."""
    e, ok = edges(case.sample_rate)
    x = signal(case)
    F = 0 if len(x) < L or not ok else (len(x) - L) // H + 1
    if F == 0:
        return Ref(0, np.zeros(0, np.uint32), np.zeros((0, BANDS)), np.zeros((0, 32)), 0, ok)
    win = (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(L) / L)).astype(np.float32).astype(np.float64)
    frames = np.lib.stride_tricks.sliding_window_view(x, L)[::H][:F]
    bad = ~np.isfinite(frames).all(axis=1)
    with np.errstate(invalid="ignore"):
        P = np.abs(np.fft.rfft(np.where(bad[:, None], 0.0, frames).astype(np.float64) * win, axis=1)) ** 2
    E = np.stack([P[:, e[m]:e[m + 1]].sum(axis=1) for m in range(BANDS)], axis=1)
    E[bad] = 0.0
    D = E[:, :-1] - E[:, 1:]
    d = D[1:] - D[:-1]
    codes = ((d > 0).astype(np.uint64) << np.arange(32, dtype=np.uint64)).sum(axis=1).astype(np.uint32)
    scale = E[1:].sum(axis=1) + E[:-1].sum(axis=1)
    margins = np.abs(d) / np.where(scale > 0, scale, 1.0)[:, None]
    return Ref(F, codes, E, margins, int(bad.sum()), ok)


def band_error(E, ref):
    """The largest |E - ref| over a frame's bands, relative to the frame's largest reference band energy; 0 for no frame."""
    if not len(ref):
        return 0.0
    top = ref.max(axis=1)
    return float((np.abs(E - ref).max(axis=1) / np.where(top > 0, top, 1.0)).max())


def flipped(codes, ref):
    """-> (differing bits, the largest reference margin among them)."""
    x = (codes ^ ref.codes)[:, None] >> np.arange(32, dtype=np.uint32) & 1
    return int(x.sum()), float(ref.margins[x.astype(bool)].max()) if x.any() else 0.0


@lru_cache(maxsize=None)
def measured():
    with open(MEASURED) as f:
        return json.load(f)


# ---- stage 2: the match restated ------------------------------------------------------------------------------------------------
_POP = np.array([bin(i).count("1") for i in range(65536)], dtype=np.uint32)


def popcount(x):
    x = np.asarray(x, dtype=np.uint32)
    return _POP[x & 0xFFFF] + _POP[x >> 16]


def ref_match(codes, rates, block=256, probes=8, radius=512, permille=None):
    """The header's stage 2 on a list of uint32 code arrays -> PAIR records in (i, j) order.  Python integers throughout."""
    permille = _capi.FP_MAX_BER_PERMILLE if permille is None else permille
    n = len(codes)
    out = []
    for i in range(n):
        for j in range(i + 1, n):
            ok = rates[i] == rates[j] and edges(rates[i])[1] and len(codes[i]) >= block and len(codes[j]) >= block
            if not ok:
                out.append((0, 0, 0, _capi.FP_PAIR_SKIPPED))
                continue
            probe_j = len(codes[j]) < len(codes[i])
            A, B = (codes[j], codes[i]) if probe_j else (codes[i], codes[j])
            ka, kb = len(A), len(B)
            best = None
            for d in range(-radius, radius + 1):
                errors = counting = 0
                for p in range(probes):
                    s = (2 * p + 1) * (ka - block) // (2 * probes)
                    if s + d < 0 or s + d + block > kb:
                        continue
                    errors += int(popcount(A[s:s + block] ^ B[s + d:s + d + block]).sum())
                    counting += 1
                if counting < (probes + 1) // 2:
                    continue
                cand = (errors, counting * block * 32, d)
                if best is None:
                    best = cand
                    continue
                l, r = cand[0] * best[1], best[0] * cand[1]
                if l < r or (l == r and (abs(d), d) < (abs(best[2]), best[2])):
                    best = cand
            if best is None:
                out.append((0, 0, 0, _capi.FP_PAIR_SKIPPED))
                continue
            flags = _capi.FP_PAIR_COMPARED | (_capi.FP_PAIR_PROBE_J if probe_j else 0)
            if best[0] * 1000 <= best[1] * permille:
                flags |= _capi.FP_PAIR_MATCH
            out.append((best[0], best[1], best[2], flags))
    return np.array(out, dtype=PAIR) if out else np.zeros(0, dtype=PAIR)


def random_codes(k, seed):
    return np.random.default_rng(seed).integers(0, 2 ** 32, size=k, dtype=np.uint64).astype(np.uint32)


def flip_bits(codes, positions):
    """`codes` with the bits at `positions` (code index, bit) flipped."""
    out = codes.copy()
    for i, b in positions:
        out[i] ^= np.uint32(1 << b)
    return out


def planted(k_a, k_b, lag, seed, flips=()):
    """A (k_a random codes) and B (k_b codes) with B[s + lag] = A[s] wherever both exist, then `flips` applied to B's copy, at
    positions (index in A, bit).  Everything else in B is random."""
    a = random_codes(k_a, seed)
    b = random_codes(k_b, seed + 1)
    for s in range(k_a):
        if 0 <= s + lag < k_b:
            b[s + lag] = a[s]
    for i, bit in flips:
        if 0 <= i + lag < k_b:
            b[i + lag] ^= np.uint32(1 << bit)
    return a, b


MatchCase = namedtuple("MatchCase", "name codes rates opts")
SMALL = dict(block=32, probes=3, radius=8, max_ber_permille=100)


@lru_cache(maxsize=None)
def match_cases():
    """Constructed code sets with their options.  `small` options unless the defaults are the point."""
    out = []
    R = 44100
    # ka = 100, block 32, 3 probes: blocks [11, 43), [34, 66), [56, 88).  Flips at (12, two bits), 40 (in two blocks) and 70:
    # 5 errors in 3072 bits at the planted lag; radius 8: +-9 is out of reach
    for lag in (0, 1, -1, 8, -8, 9, -9):
        a, b = planted(100, 140, lag, 20 + lag, flips=[(12, 0), (12, 5), (40, 31), (70, 3)])
        out.append(MatchCase(f"lag{lag}", (a, b), (R, R), SMALL))
    a, b = planted(32, 60, 4, 50)
    out.append(MatchCase("ka_is_block", (a, b), (R, R), SMALL))
    a, b = planted(32, 32, 0, 52)
    out.append(MatchCase("kb_is_block", (a, b), (R, R), SMALL))
    out.append(MatchCase("probe_j", (random_codes(90, 54), random_codes(32, 55)), (R, R), SMALL))
    # equal lengths of 100, 4 probes at 8, 25, 42, 59, two needed: at lag 40 probes 0 and 1 count (2048 bits), at lag 44 only
    # probe 0, so a copy planted there is not found
    for lag in (40, 44):
        a, b = planted(100, 100, lag, 60 + lag)
        out.append(MatchCase(f"half_the_probes_lag{lag}", (a, b), (R, R), dict(block=32, probes=4, radius=48, max_ber_permille=100)))
    # ties: a constant code sequence matches at every lag with 0 errors -> lag 0; periodic codes tie at +-period
    c = np.full(80, 0xDEADBEEF, dtype=np.uint32)
    out.append(MatchCase("tie_all_lags", (c, np.full(120, 0xDEADBEEF, dtype=np.uint32)), (R, R), SMALL))
    per = np.tile(random_codes(4, 61), 40)
    out.append(MatchCase("tie_periodic", (per[:96], np.concatenate([random_codes(2, 62), per[:120]])), (R, R), SMALL))
    a, b = planted(100, 100, 3, 63)
    out.append(MatchCase("one_probe", (a, b), (R, R), dict(block=32, probes=1, radius=8, max_ber_permille=100)))
    a, b = planted(100, 100, 0, 64)
    out.append(MatchCase("rates_differ", (a, b), (44100, 48000), SMALL))
    out.append(MatchCase("rate_unsupported", (a, b), (96000, 96000), SMALL))
    out.append(MatchCase("short", (a[:31], b), (R, R), SMALL))
    out.append(MatchCase("n1", (a,), (R,), SMALL))
    out.append(MatchCase("n0", (), (), SMALL))
    # a chain: a ~ b and b ~ c, a !~ c -> one group; d alone; e at another rate; f too short
    base = random_codes(120, 70)
    rng = np.random.default_rng(71)

    def worn(x, share):
        y = x.copy()
        idx = rng.random((len(x), 32)) < share
        return y ^ (idx.astype(np.uint64) << np.arange(32, dtype=np.uint64)).sum(axis=1).astype(np.uint32)

    bb = worn(base, 0.07)
    cc = worn(bb, 0.07)
    out.append(MatchCase("chain", (base, bb, cc, random_codes(120, 72), base.copy(), base[:20].copy()), (R, R, R, R, 48000, R),
                         dict(block=32, probes=3, radius=8, max_ber_permille=100)))
    return tuple(out)


@lru_cache(maxsize=None)
def default_case():
    """40 tracks at the default options: per original one long track of 1400 codes and seven excerpts of about 400 codes from
    anywhere in it (so within and beyond the radius of 512), each more worn than the one before (4 % of the bits per step)."""
    rng = np.random.default_rng(80)
    tracks = []
    for o in range(5):
        long = random_codes(1500, 81 + o)
        tracks.append(long[50:1450].copy())
        for v in range(1, 8):
            start = 50 + int(rng.integers(0, 1000))
            y = long[start:start + 400 + 7 * v].copy()
            idx = rng.random((len(y), 32)) < 0.04 * v
            tracks.append(y ^ (idx.astype(np.uint64) << np.arange(32, dtype=np.uint64)).sum(axis=1).astype(np.uint32))
    return MatchCase("defaults_40", tuple(tracks), (44100,) * len(tracks), dict())
