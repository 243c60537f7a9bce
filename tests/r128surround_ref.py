"""The checker of the weighted (multichannel) EBU R 128 path: BS.1770 channel weights on top of tests/r128ref.py and
tests/r128range_ref.py, as include/mp3rgain_amd_r128.h defines them.  The weighted hop energy is the sum over the channels
with a weight that is not zero of weight x `r128ref.hop_energies([channel])`, in ascending channel order; peaks and the
finiteness of a track are over all its channels whatever their weight.  The layout rule is restated here from the header's
text.  It shares no code with the library.  Not part of the product."""
import math
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent))
import r128range_ref  # noqa: E402
import r128ref  # noqa: E402

DEFAULT_MASK = {1: 0x4, 2: 0x3, 3: 0x7, 4: 0x33, 5: 0x37, 6: 0x3F, 7: 0x70F, 8: 0x63F}
LFE, BL, BR, SL, SR = 0x8, 0x10, 0x20, 0x200, 0x400


def layout_weights(channels, mask=0):
    """Channel i is the i-th set bit of the WAVE channel mask in ascending bit order; 0 or a wrong population count: the
    default of the count.  LFE 0, the side surrounds 1.41, the back pair 1.41 when there are no side surrounds, else 1.0."""
    if not 1 <= channels <= 8:
        raise ValueError(channels)
    if mask == 0 or bin(mask).count("1") != channels:
        mask = DEFAULT_MASK[channels]
    sides = bool(mask & (SL | SR))
    out = []
    for bit in range(32):
        pos = 1 << bit
        if not mask & pos:
            continue
        if pos == LFE:
            out.append(0.0)
        elif pos in (SL, SR) or (pos in (BL, BR) and not sides):
            out.append(1.41)
        else:
            out.append(1.0)
    return out[:channels]


def hop_energies(channels, rate, weights, dtype=np.float64):
    H = len(channels[0]) // r128ref.hop_frames(rate)
    e = None
    for c, w in zip(channels, weights):
        if w == 0.0:
            continue
        term = dtype(w) * r128ref.hop_energies([c], rate, dtype)
        e = term if e is None else e + term
    return np.zeros(H, dtype=dtype) if e is None else e


def block_z_from(e, rate):
    if len(e) < 4:
        return np.zeros(0, dtype=e.dtype)
    return (e[:-3] + e[1:-2] + e[2:-1] + e[3:]) / e.dtype.type(4 * r128ref.hop_frames(rate))


def finite(channels):
    return all(r128ref.finite([c]) for c in channels)


def sample_peak(channels):
    return max(r128ref.sample_peak([c]) for c in channels)


def true_peak(channels, rate):
    return max(r128ref.true_peak([c], rate) for c in channels)


def analyze(channels, rate, weights, want_true_peak=False):
    """One weighted track -> the fields of rg_r128_track_result and of rg_r128_dynamics, the block values "z" and "st", the
    hop energies "e"."""
    frames = len(channels[0])
    out = {"sample_peak": sample_peak(channels), "true_peak": true_peak(channels, rate) if want_true_peak else math.nan,
           "blocks": r128ref.block_count(rate, frames), "st_blocks": r128range_ref.short_term_count(rate, frames)}
    if not finite(channels):
        out.update(r128range_ref._NAN5, loudness_lufs=math.nan, gain_db=math.nan, blocks_gated=0, z=np.zeros(0), st=np.zeros(0),
                   e=np.zeros(0), finite=False)
        return out
    e = hop_energies(channels, rate, weights)
    z = block_z_from(e, rate)
    st = r128range_ref.short_term_from(e, rate)
    lufs, kept, _ = r128ref.gate(z)
    out.update(r128range_ref.loudness_range(st))
    out.update(loudness_lufs=lufs, gain_db=r128ref.gain_from(lufs), blocks_gated=kept, z=z, st=st, e=e, finite=True,
               max_momentary_lufs=r128range_ref.lufs(float(z.max())) if len(z) else -math.inf,
               max_short_term_lufs=r128range_ref.lufs(float(st.max())) if len(st) else -math.inf)
    return out


def analyze_album(tracks, want_true_peak=False):
    """tracks: [(channels, rate, weights)] -> (per-track dicts, album dict): the gates of the loudness and of the range over
    the union of the tracks' gating and short-term blocks."""
    res = [analyze(ch, rate, w, want_true_peak) for ch, rate, w in tracks]
    album = {"sample_peak": max([r["sample_peak"] for r in res], default=0.0),
             "true_peak": max([r["true_peak"] for r in res], default=0.0) if want_true_peak else math.nan,
             "blocks": sum(r["blocks"] for r in res), "st_blocks": sum(r["st_blocks"] for r in res)}
    if not all(r["finite"] for r in res):
        album.update(r128range_ref._NAN5, loudness_lufs=math.nan, gain_db=math.nan, blocks_gated=0, z=np.zeros(0), st=np.zeros(0))
        return res, album
    z = np.concatenate([r["z"] for r in res]) if res else np.zeros(0)
    st = np.concatenate([r["st"] for r in res]) if res else np.zeros(0)
    lufs, kept, _ = r128ref.gate(z)
    album.update(r128range_ref.loudness_range(st))
    album.update(loudness_lufs=lufs, gain_db=r128ref.gain_from(lufs), blocks_gated=kept, z=z, st=st,
                 max_momentary_lufs=max([r["max_momentary_lufs"] for r in res], default=-math.inf),
                 max_short_term_lufs=max([r["max_short_term_lufs"] for r in res], default=-math.inf))
    return res, album


def tech3341_case6(rate, seconds=20.0):
    """EBU Tech 3341 case 6: a 1 kHz sine in L, R, C, Ls, Rs at -28, -28, -24, -30, -30 dBFS; -23.0 +- 0.1 LUFS."""
    return [r128ref.sine_segments(rate, [(seconds, db)], channels=1)[0] for db in (-28.0, -28.0, -24.0, -30.0, -30.0)]
