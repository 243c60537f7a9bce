"""The lossy ancestry scan (include/mp3rgain_amd_ancestry.h): the cases the CPU and GPU tests and tools/ancestry_refcheck.py
share, and a float64 reference that does not depend on the new C++.

The reference is built from oracle/mp3_encoder.py's polyphase_analysis, mdct_granules and alias_encode -- the encoder's own
forward chain -- and numpy: per view the samples in 16-bit LSB units as float64, per segment and alignment the 576 lines of
every granule, the groups of 12, the counts; then the finish restated in Python (fractions for the comparisons of ratios).

Coded inputs are made two ways, and their true grid offset is known by construction: a short cut (analysis -> quantise at a
step chosen by the share of lines it sends to 0 -> requantise -> the float64 decoder's back half -> round to 16 bits), and real
streams from oracle/mp3_encoder.encode, decoded by this library's MP3 decoder.  Both have 1057 samples of delay, so an input
with k leading samples trimmed has its grid at (481 - k) mod 576.  Not part of the product."""
import json
import math
import sys
from collections import namedtuple
from fractions import Fraction
from functools import lru_cache
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
for p in (ROOT, ROOT / "oracle"):
    if str(p) not in sys.path:
        sys.path.insert(0, str(p))

import mp3_encoder as E  # noqa: E402
import mp3_refdec as R  # noqa: E402

from mp3rgain_amd import _capi  # noqa: E402

MEASURED = ROOT / "tests" / "golden" / "ancestry_measured.json"
TOLERANCE_FACTOR = 4  # as the spectrum tests take it: for rounding the tool's cases did not meet
ACTIVE_FLOOR = 1.0 / 216.0
ALIGN = 576
RATE = 44100

# kind: "found" = coded and expected to be flagged at `offset`; "miss" = coded but expected UNFLAGGED (the stated limit);
# "clean" = never coded, unflagged; "shape" = a shape case: only the routes are compared (and the reference's counts)
Case = namedtuple("Case", "name channels sample_rate segments granules kind offset midside")
Case.__new__.__defaults__ = (None, False)


# ---- signals ------------------------------------------------------------------------------------------------------------------
def _coloured(rng, n, pole=0.95):
    w = rng.standard_normal(n + 200)
    y = np.empty_like(w)
    acc = 0.0
    for i, v in enumerate(w):
        acc = pole * acc + v
        y[i] = acc
    return y[200:] / np.std(y[200:])


def music(n, seed, amp=3000.0):
    """Music-like: coloured noise plus two tones, in LSB units (float64)."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / RATE
    return amp * (_coloured(rng, n) + 0.6 * np.sin(2 * np.pi * 440.0 * t) + 0.4 * np.sin(2 * np.pi * 1318.5 * t + 0.3))


def to_s16(x):
    return np.clip(np.rint(x), -32768, 32767).astype(np.int16)


def alias_decode(xr):
    """The decoder's alias reduction: the inverse of E.alias_encode, in place on one long granule."""
    cs, ca = E.alias_coeffs()
    for sb in range(1, 32):
        for i in range(8):
            lo, up = 18 * sb - 1 - i, 18 * sb + i
            a, b = xr[lo], xr[up]
            xr[lo] = a * cs[i] - b * ca[i]
            xr[up] = b * cs[i] + a * ca[i]


def short_cut(x, zero_share):
    """x (LSB units, float64) coded with long blocks at the global step that sends `zero_share` of the lines to 0 ->
    (decoded float64 in LSB units, with 1057 samples of delay; the share that was reached)."""
    n = (len(x) + 575) // 576 * 576 + 2 * 576
    xp = np.zeros(n)
    xp[:len(x)] = x
    ngr = n // 576
    spec = E.mdct_granules(E.polyphase_analysis(xp), [0] * ngr)
    for g in range(ngr):
        E.alias_encode(spec[g])
    body = np.abs(spec[2:-2])
    gg = next(g for g in range(400, -200, -1) if (E.quantise(body, g) == 0).mean() <= zero_share)  # a larger gg is a finer step
    ix = E.quantise(np.abs(spec), gg)
    share = float((E.quantise(body, gg) == 0).mean())
    xr = np.sign(spec) * ix.astype(np.float64) ** (4.0 / 3.0) * 2.0 ** ((gg - 210) / 4.0)
    for g in range(ngr):
        alias_decode(xr[g])
    sub = R.imdct_overlap(xr, np.zeros(ngr, dtype=np.int64), np.zeros(ngr, dtype=bool), np.float64)
    return R.synthesis(sub, np.float64), share


@lru_cache(maxsize=None)
def real_stream(bitrate, nch, allow_ms, allow_short, seed=5):
    """A stream of oracle/mp3_encoder.encode decoded by this library's MP3 decoder -> float32 [channels][frames] in [-1, 1)."""
    from mp3rgain_amd import mp3dec

    _capi.load()  # first: it lets PyTorch bring its HIP runtime in before the library is mapped (one runtime per process)
    dec, info = mp3dec.decode(real_stream_bytes(bitrate, nch, allow_ms, allow_short, seed))
    assert info.skipped_frames == 0
    return dec


@lru_cache(maxsize=None)
def real_stream_bytes(bitrate, nch, allow_ms, allow_short, seed=5):
    """The stream itself."""
    n = 13000
    m = music(n, seed) / 32768.0
    if nch == 2:
        other = music(n, seed + 100, 900.0) / 32768.0  # a side at 0.09 of the mid's energy: mid/side frames when that is allowed (< 0.12)
        pcm = np.stack([m + other, m - other])
    else:
        pcm = m[None, :]
    if allow_short:  # an attack, so that the window switches
        pcm = pcm.copy()
        pcm[:, 6000:6100] += 0.5 * np.sin(2 * np.pi * 3000.0 * np.arange(100) / RATE)[None, :]
    return E.encode(pcm, RATE, bitrate, seed=seed, allow_ms=allow_ms, allow_short=allow_short)


def _trim(planes, k, n):
    return [np.ascontiguousarray(p[k:k + n]) for p in planes]


def grid_after(k):
    return (481 - k) % ALIGN


@lru_cache(maxsize=None)
def cases():
    rng = np.random.default_rng(0xA11CE)
    out = []
    L33 = 576 * 5          # a segment of 3 granules
    N33 = 3 * L33 + 300    # 3 segments of 3 granules fit, with a remainder
    src = music(N33 + 4000, 1)
    # ---- coded, the short cut: coarse, medium, fine
    for tag, share, kind in (("coarse", 0.47, "found"), ("medium", 0.20, "found"), ("fine", 0.03, "miss")):
        dec, _ = short_cut(src, share)
        out.append(Case(f"cut_{tag}_k2000", [to_s16(dec[2000:2000 + N33])], RATE, 3, 3, kind, grid_after(2000)))
    dec, _ = short_cut(src, 0.47)
    for k in (0, 1, 31, 32, 575):
        out.append(Case(f"cut_coarse_k{k}", [to_s16(dec[k:k + N33])], RATE, 3, 3, "found", grid_after(k)))
    # the same coded audio in the other two containers: padded to 24 bits in 32, and as floats
    s = to_s16(dec[2000:2000 + N33])
    out.append(Case("cut_coarse_s32", [s.astype(np.int32) << 16], RATE, 3, 3, "found", grid_after(2000)))
    out.append(Case("cut_coarse_f32", [(s / 32768.0).astype(np.float32)], RATE, 3, 3, "found", grid_after(2000)))
    # ---- coded, real streams (decoded to float, as the MP3 route leaves them, and rounded to 16 bits, as a rip in FLAC has them)
    for br, nch, ms, sh in ((64, 1, False, False), (128, 1, False, True), (64, 2, False, False), (128, 2, False, False), (64, 2, True, False),
                            (128, 2, True, True)):
        dec = real_stream(br, nch, ms, sh)
        name = f"mp3_{br}_{'mono' if nch == 1 else ('ms' if ms else 'lr')}{'_short' if sh else ''}"
        out.append(Case(name + "_k0_f32", _trim(list(dec), 0, N33), RATE, 3, 3, "found", grid_after(0), ms))
        out.append(Case(name + "_k2000_s16", [to_s16(p * 32768.0) for p in _trim(list(dec), 2000, N33)], RATE, 3, 3, "found", grid_after(2000), ms))
    # 320 kb/s: mono is coded so finely that few lines fall to 0 -- the stated limit; in a mid/side stream the side channel is
    # weak, its lines are small against the frame's one quantiser step, and they fall to 0 at any bitrate
    for nch, ms, kind in ((1, False, "miss"), (2, True, "found")):
        dec = real_stream(320, nch, ms, False)
        out.append(Case(f"mp3_320_{'mono' if nch == 1 else 'ms'}_k2000_s16", [to_s16(p * 32768.0) for p in _trim(list(dec), 2000, N33)], RATE, 3, 3, kind,
                        grid_after(2000), ms))
    dec = real_stream(128, 1, False, True)
    for k in (1, 31, 32, 575):
        out.append(Case(f"mp3_128_mono_short_k{k}_s16", [to_s16(dec[0][k:k + N33] * 32768.0)], RATE, 3, 3, "found", grid_after(k)))
    # ---- never coded
    n = N33
    t = np.arange(n) / RATE
    clean = {
        "white": rng.standard_normal(n) * 3000.0,
        "pink": _coloured(rng, n, 0.98) * 3000.0,
        "music": music(n, 2),
        "two_tones": 6000.0 * np.sin(2 * np.pi * 440.0 * t) + 4000.0 * np.sin(2 * np.pi * 1318.5 * t),
        "square_300": np.where(np.floor(2 * 300.0 * t) % 2 == 0, 8000.0, -8000.0),
        "sweep": 8000.0 * np.sin(2 * np.pi * (50.0 * t + 0.5 * (18000.0 / t[-1]) * t * t)),
        "clipped_sine": np.clip(40000.0 * np.sin(2 * np.pi * 997.0 * t), -32768, 32767),
    }
    for name, x in clean.items():
        out.append(Case(f"clean_{name}", [to_s16(x)], RATE, 3, 3, "clean"))
    out.append(Case("clean_music_stereo", [to_s16(music(n, 3)), to_s16(music(n, 4))], RATE, 3, 3, "clean"))
    out.append(Case("clean_padded_24", [to_s16(clean["music"]).astype(np.int32) << 16], RATE, 3, 3, "clean"))
    out.append(Case("clean_silence", [np.zeros(n, np.int16), np.zeros(n, np.int16)], RATE, 3, 3, "clean"))
    nf = (music(n, 6) / 32768.0).astype(np.float32)
    nf[[0, 700, 5000, n - 1]] = [np.nan, np.inf, -np.inf, np.nan]
    out.append(Case("clean_f32_nan_inf", [nf, (music(n, 7) / 32768.0).astype(np.float32)], RATE, 3, 3, "clean"))
    # ---- shapes: the smallest at which the cutting can go wrong
    tile = _capi_tile()
    x = to_s16(music(12 * 576 + 50, 8))
    for G in (1, 2, 3):
        L = 576 * (G + 2)
        for N in sorted({3 * 576 - 1, 3 * 576, L - 1, L, L + 1, 2 * L + 7}):
            for S in (1, 2, 3):
                if (G, S) in ((1, 1), (2, 2), (3, 3)) or N == 2 * L + 7:
                    out.append(Case(f"shape_g{G}_s{S}_n{N}", [x[:N].copy()], RATE, S, G, "shape"))
    out.append(Case("shape_whole_plane", [x[:576 * 6 + 5].copy()], RATE, 0, 1, "shape"))
    out.append(Case(f"shape_tile_plus_1", [x[:576 * (tile + 3) + 9].copy()], RATE, 0, 1, "shape"))  # two tiles, the second of one granule
    for ch in (2, 3, 8):
        planes = [to_s16(music(4 * 576 + 3, 20 + c)) for c in range(ch)]
        out.append(Case(f"shape_{ch}ch", planes, RATE, 2, 1, "shape"))
    out.append(Case("shape_2ch_s32", [(to_s16(music(3 * 576, 30 + c)).astype(np.int32) << 16) + 77 for c in range(2)], RATE, 1, 1, "shape"))
    out.append(Case("shape_2ch_f32", [(music(3 * 576 + 1, 40 + c) / 32768.0).astype(np.float32) for c in range(2)], RATE, 1, 1, "shape"))
    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    return tuple(out)


def _capi_tile():
    from mp3rgain_amd import ancestry_kernel_shape

    return ancestry_kernel_shape()[1]


# ---- the float64 reference ----------------------------------------------------------------------------------------------------
def lsb(plane):
    """A plane in 16-bit LSB units as float64 -> (values, number of non-finite samples)."""
    if plane.dtype == np.int16:
        return plane.astype(np.float64), 0
    if plane.dtype == np.int32:
        return plane.astype(np.float64) / 65536.0, 0
    bad = ~np.isfinite(plane)
    return np.where(bad, 0.0, plane.astype(np.float64)) * 32768.0, int(bad.sum())


def views_of(case):
    """[(kind, float64 samples, nonfinite)] in the order of the record."""
    planes = [lsb(p) for p in case.channels]
    out = [(c, y, nf) for c, (y, nf) in enumerate(planes)]
    if len(planes) == 2:
        (l, _), (r, _) = planes
        out.append((_capi.ANC_VIEW_MID, 0.5 * (l + r), 0))
        out.append((_capi.ANC_VIEW_SIDE, 0.5 * (l - r), 0))
    return out


def cut(N, S, G):
    """-> (S, G, [starts]) as they are used."""
    if N < 3 * 576:
        return 0, 0, []
    whole = N // 576 - 2
    if S == 0 or G > whole:
        return 1, whole, [0]
    L = 576 * (G + 2)
    S = min(S, N // L)
    return S, G, [0] if S == 1 else [576 * (j * (N - L) // (576 * (S - 1))) for j in range(S)]


def _cs_ca():
    cs, ca = E.alias_coeffs()
    return cs, ca


def ref_counts(y, S, G, starts, floor=ACTIVE_FLOOR):
    """small[576], active[576] (int64) of one view in float64."""
    small = np.zeros(ALIGN, np.int64)
    active = np.zeros(ALIGN, np.int64)
    N = len(y)
    cs, ca = _cs_ca()
    sb = np.arange(1, 32)
    lo = (18 * sb[:, None] - 1 - np.arange(8)[None, :]).reshape(-1)
    up = (18 * sb[:, None] + np.arange(8)[None, :]).reshape(-1)
    csv, cav = np.tile(cs, 31), np.tile(ca, 31)
    nslots = 18 * (G + 1)
    for a in starts:
        for p in range(32):
            # 16 slots of run-in (512 >= 480 samples of history), then the slots of q = 0 .. 17
            first = a + p - 512
            need = 32 * (16 + nslots + 17)
            idx = first + np.arange(need)
            x = np.where((idx >= 0) & (idx < N), y[np.clip(idx, 0, N - 1)], 0.0)
            sub = E.polyphase_analysis(x)[16:]
            for q in range(18):
                xr = E.mdct_granules(sub[q:q + nslots], [0] * (G + 1))[1:]   # granule 0 is only history
                a_, b_ = xr[:, lo].copy(), xr[:, up].copy()                   # E.alias_encode, every butterfly at once
                xr[:, lo] = a_ * csv + b_ * cav
                xr[:, up] = b_ * csv - a_ * cav
                g12 = xr.reshape(G, 48, 12)
                ms = (g12 * g12).mean(axis=2)
                act = ms >= floor
                sm = (256.0 * g12 * g12 < ms[:, :, None]) & act[:, :, None]
                small[32 * q + p] += int(sm.sum())
                active[32 * q + p] += 12 * int(act.sum())
    return small, active


def finish_view(small, active, z_min, iso_min):
    """The finish restated: -> dict of the view record's numbers."""
    w = dict(offset=0, ratio=0.0, second=0.0, p0=0.0, z=0.0, iso=0.0, small=0, active=0, active_total=int(active.sum()), flagged=False)
    cand = [r for r in range(ALIGN) if active[r] >= 1]
    if not cand:
        return w
    key = lambda r: (Fraction(int(small[r]), int(active[r])), -r)  # noqa: E731  (ties go to the lowest r)
    best = max(cand, key=key)
    rest = [r for r in cand if r != best]
    w.update(offset=best, small=int(small[best]), active=int(active[best]), ratio=int(small[best]) / int(active[best]))
    if rest:
        s2 = max(rest, key=key)
        w["second"] = int(small[s2]) / int(active[s2])
    ra = int(active.sum()) - int(active[best])
    w["p0"] = (int(small.sum()) - int(small[best])) / ra if ra else 0.0
    var = w["p0"] * (1.0 - w["p0"]) * int(active[best])
    w["z"] = (int(small[best]) - w["p0"] * int(active[best])) / math.sqrt(var) if var > 0.0 else 0.0
    w["iso"] = w["ratio"] / w["second"] if w["second"] > 0.0 else (math.inf if w["ratio"] > 0.0 else 0.0)
    w["flagged"] = w["z"] >= z_min and w["iso"] >= iso_min
    return w


def thresholds():
    """(z_min, iso_min): the geometric means of the two sides recorded in tests/golden/ancestry_measured.json."""
    m = json.loads(MEASURED.read_text())
    return math.sqrt(m["never_coded_max_z"] * m["coded_min_z"]), math.sqrt(m["never_coded_max_iso"] * m["coded_min_iso"])


@lru_cache(maxsize=None)
def reference(name, with_thresholds=True):
    """The float64 reference of one case, computed once and shared: dict(S, G, views=[dict], counts=[(small, active)], flags,
    grid_offset, best_view)."""
    case = next(c for c in cases() if c.name == name)
    z_min, iso_min = thresholds() if with_thresholds else (math.inf, math.inf)
    N = len(case.channels[0])
    S, G, starts = cut(N, case.segments, case.granules)
    views, counts = [], []
    flags = _capi.ANC_COMPLETE
    for kind, y, nf in views_of(case):
        small, active = ref_counts(y, S, G, starts) if S else (np.zeros(ALIGN, np.int64), np.zeros(ALIGN, np.int64))
        w = finish_view(small, active, z_min, iso_min)
        w.update(kind=kind, nonfinite=nf)
        views.append(w)
        counts.append((small, active))
        if nf:
            flags |= _capi.ANC_NONFINITE
    best = None
    for i, w in enumerate(views):
        if w["flagged"] and (best is None or w["z"] > views[best]["z"]):
            best = i
    if best is not None:
        flags |= _capi.ANC_MP3_GRID
        if views[best]["kind"] >= _capi.ANC_VIEW_MID:
            flags |= _capi.ANC_MIDSIDE
    if S == 0:
        flags |= _capi.ANC_SHORT
    if not any(w["active_total"] for w in views):
        flags |= _capi.ANC_SILENT
    return dict(S=S, G=G, views=views, counts=counts, flags=flags, grid_offset=views[best]["offset"] if best is not None else 0, best_view=best)


def pack_one(case, layout=None):
    """One case in an arena of its own, between guards at an odd offset -> (arena, [desc])."""
    import arena_layouts as al

    Tr = namedtuple("Tr", "channels sample_rate")
    arena, descs, _ = al.pack([Tr(list(case.channels), case.sample_rate)], layout or al.Layout("guard", "loud", "input", 1))
    return arena, [descs[0]]
