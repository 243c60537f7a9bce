"""The shared cases of the FLAC encoder's tests (include/mp3rgain_amd_flacenc.h): the smallest shapes at which it can go wrong.

A case is PCM as right-justified integers [channels][n] of `bps` bits at `rate`; a group is the cases of one call of the seam
(the options belong to the call: block size, max_lpc_order).  `packed(group)` lays a group out as the loaders leave PCM in the
arena -- left-justified 16-bit planes for bps <= 16, 32-bit planes above -- at odd sample offsets with guard samples round every
track (tests/arena_layouts.py).  Nothing here is measured from the encoder: the streams are held to their input by the
decoders in the tree and to sizes derived from the format."""
import sys
from collections import namedtuple
from functools import lru_cache
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))
import arena_layouts as al  # noqa: E402

Case = namedtuple("Case", "name pcm bps rate")
Group = namedtuple("Group", "name block lpc cases")
Track = namedtuple("Track", "channels sample_rate")

LENGTHS = lambda block, lpc: [0, 1, 2, lpc + 1, 63, 64, 65, 4095, 4096, 4097, 3 * 4096 + 1]  # noqa: E731


def full_scale(bps):
    return -(1 << (bps - 1)), (1 << (bps - 1)) - 1


def ar2(rng, channels, n, bps, level=0.25):
    """An AR(2) "music-like" signal: a resonance driven by noise, `level` of full scale at its peak."""
    x = np.zeros((channels, n + 2))
    e = rng.normal(0.0, 1.0, (channels, n + 2))
    for i in range(2, n + 2):
        x[:, i] = 1.8 * x[:, i - 1] - 0.9 * x[:, i - 2] + e[:, i]
    x = x[:, 2:]
    peak = np.abs(x).max() if n else 1.0
    lo, hi = full_scale(bps)
    return np.clip(np.round(x / max(peak, 1e-9) * level * hi), lo, hi).astype(np.int64)


def sine(channels, n, bps, period=97.3):
    lo, hi = full_scale(bps)
    t = np.arange(n)
    return np.stack([np.round(0.8 * hi * np.sin(2 * np.pi * t / (period * (1 + 0.1 * c)))).astype(np.int64) for c in range(channels)])


def noise(rng, channels, n, bps):
    lo, hi = full_scale(bps)
    return rng.integers(lo, hi + 1, size=(channels, n), dtype=np.int64)


def rails(n, bps):
    """Both rails alternating, the channels opposed: the side signal needs all bps + 1 bits and the high-order predictors'
    residuals do not fit 32 bits at 24 bits per sample."""
    lo, hi = full_scale(bps)
    l = np.where(np.arange(n) % 2 == 0, hi, lo).astype(np.int64)
    r = np.where(np.arange(n) % 2 == 0, lo, hi).astype(np.int64)
    return np.stack([l, r])


def _content(rng, block):
    n = 2 * block + 100
    m16 = ar2(rng, 2, n, 16)
    mono = ar2(rng, 1, n, 16)
    half = ar2(rng, 2, n, 16)
    half[:, :block // 2] = 0
    half[:, block:block + block // 2] = 0
    return [
        Case("silence", np.zeros((2, n), dtype=np.int64), 16, 44100),
        Case("constant", np.full((2, n), -1234, dtype=np.int64), 16, 44100),
        Case("rails16", rails(n, 16), 16, 44100),
        Case("rails24", rails(n, 24), 24, 44100),
        Case("noise16", noise(rng, 2, n, 16), 16, 44100),
        Case("noise24", noise(rng, 2, n, 24), 24, 44100),
        Case("sine16", sine(2, n, 16), 16, 44100),
        Case("sine24", sine(2, n, 24), 24, 96000),
        Case("ar2_16", m16, 16, 44100),
        Case("mono_16", mono, 16, 44100),
        # 16-bit audio padded to 24: wasted bits.  One channel: in two, the padded mid signal keeps the low bit of L + R that
        # the 16-bit mid signal drops, so a 16-bit twin coded M/S has no padded counterpart of its size
        Case("pad24", mono << 8, 24, 44100),
        Case("pad24_stereo", m16 << 8, 24, 44100),
        Case("l_eq_r", np.concatenate([mono, mono]), 16, 44100),
        Case("r_eq_minus_l", np.concatenate([mono, -mono]), 16, 44100),
        Case("half_silent", half, 16, 44100),
    ]


@lru_cache(maxsize=None)
def groups():
    rng = np.random.default_rng(0xF1AC)
    out = []
    for gname, block, lpc in (("b4096_lpc8", None, None), ("b256_lpc12", 256, 12), ("b1024_lpc0", 1024, 0)):
        eff_block, eff_lpc = block or 4096, 8 if lpc is None else lpc
        cases = []
        if gname != "b1024_lpc0":
            base = ar2(rng, 2, 3 * 4096 + 1, 16)
            cases += [Case(f"len{n}", base[:, :n].copy(), 16, 44100) for n in LENGTHS(eff_block, eff_lpc)]
            cases += _content(rng, eff_block)
        if gname == "b4096_lpc8":
            cases += [Case(f"width{b}", ar2(rng, 2, 4500, b), b, 48000) for b in (8, 12, 16, 20, 24)]
            cases += [Case(f"ch{c}", ar2(rng, c, 4200, 16), 16, 44100) for c in (1, 2, 3, 6, 8)]
            cases += [Case(f"rate{r}", ar2(rng, 1, 300, 16), 16, r) for r in (44100, 48000, 96000, 37800, 352800)]
            # about 40 frames x 8 channels x 24 bits, most of it incompressible: the write kernel's carry from channel to channel
            big = noise(rng, 8, 40 * 4096 - 7, 24)
            big[2] = ar2(rng, 1, 40 * 4096 - 7, 24)[0]
            big[5] >>= 9
            cases.append(Case("big_8ch_24", big, 24, 96000))
        if gname == "b1024_lpc0":
            cases += [Case("ar2_20_3ch", ar2(rng, 3, 2500, 20), 20, 88200), Case("sine12", sine(2, 1500, 12), 12, 32000),
                      Case("len0", np.zeros((2, 0), dtype=np.int64), 16, 44100)]
        out.append(Group(gname, block, lpc, tuple(cases)))
    return tuple(out)


def track_of(case):
    """The case as the arena holds it: left-justified planes."""
    if case.bps <= 16:
        return Track([np.ascontiguousarray((ch << (16 - case.bps)).astype(np.int16)) for ch in case.pcm], case.rate)
    return Track([np.ascontiguousarray((ch << (32 - case.bps)).astype(np.int32)) for ch in case.pcm], case.rate)


@lru_cache(maxsize=None)
def packed(gname, shift=0):
    """-> (arena, descs, bps list) of a group: odd sample offsets, loud guard samples round every track."""
    g = next(g for g in groups() if g.name == gname)
    arena, descs, _ = al.pack([track_of(c) for c in g.cases], al.Layout("guard", "loud", "input", shift))
    return arena, list(descs[:len(g.cases)]), [c.bps for c in g.cases]


def verbatim_frame_bytes(channels, bps, n, header_bytes):
    """A frame of n samples with every channel VERBATIM and independent: header, subframes (8 header bits each), CRC-16."""
    return header_bytes + (channels * (8 + n * bps) + 7) // 8 + 2
