#!/usr/bin/env python3
"""Where the stereo scan's two measured thresholds come from (include/mp3rgain_amd_stereo.h: delay_permille, phase_permille):
synthetic material through the serial host twin (rg_stereo_arena route 0; never the kernels), radius 64.

    python tools/stereo_refcheck.py            print every case's figures and compare with tests/golden/stereo_measured.json
    python tools/stereo_refcheck.py --record   write that file
    python tools/stereo_refcheck.py --subset   the cases without an MP3 encode (what tests/test_stereo_thresholds_cpu.py re-runs)

Never-delayed material: rg_synth.h tracks with independent channels (oracle/pyoracle.synth_f32), panned tones and two-tone
mixes, and partly correlated mixes L = m + g s, R = m - g s of two music-like signals, the side up to 3 dB above the mid (a wide
mix, not an inverted channel).  Of each the figure is `lag_correlation` WHEN THE BEST LAG IS NOT 0 and 0 otherwise -- a file whose
best lag is 0 cannot be flagged whatever the threshold (a panned tone correlates at 0.99 one sample off, and better in place) --
and, for the phase threshold, -correlation.  The inverted material below counts as never delayed as well.
Delayed material: the right channel the left d = +-1, +-2, +-17, +-64 frames late, as 16-bit, as float, re-dithered to 16 bits
(TPDF, one LSB), and after oracle/mp3_encoder.py at 128 and 320 kb/s decoded by the library's MP3 decoder.  Of each the figure is
`lag_correlation`, and the reading must be lag == d.  Inverted material: the right channel the negated left through the same five
treatments; the figure is -correlation.
Recorded: the two sides of each threshold, the defaults (the geometric mean of the two sides, in per mille, rounded), every
case's figures, and under "not_found" the kinds of material whose classes did not separate.  No GPU."""
import json
import math
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
for p in (ROOT, ROOT / "tests", ROOT / "oracle"):
    sys.path.insert(0, str(p))

import numpy as np  # noqa: E402

MEASURED = ROOT / "tests" / "golden" / "stereo_measured.json"
RATE, FRAMES, RADIUS = 44100, 3 * 44100, 64
MP3_FRAMES = 26000  # the encoder is Python: a little over half a second per stream
DELAYS = (1, -1, 2, -2, 17, -17, 64, -64)


def music(n, seed, amp=3000.0):
    """Music-like: coloured noise (a one-pole low-pass at 0.95) plus two tones, in LSB units (float64)."""
    rng = np.random.default_rng(seed)
    w = rng.standard_normal(n + 200)
    y = np.empty_like(w)
    acc = 0.0
    for i, v in enumerate(w):
        acc = 0.95 * acc + v
        y[i] = acc
    y = y[200:] / np.std(y[200:])
    t = np.arange(n) / RATE
    return amp * (y + 0.6 * np.sin(2 * np.pi * 440.0 * t) + 0.4 * np.sin(2 * np.pi * 1318.5 * t + 0.3))


def to_s16(x):
    return np.clip(np.rint(x), -32768, 32767).astype(np.int16)


def delayed(x, d):
    y = np.zeros_like(x)
    n = len(x)
    if d >= 0:
        y[d:] = x[:n - d]
    else:
        y[:n + d] = x[-d:]
    return y


def dither16(x, rng):
    """x in LSB units -> 16-bit with one LSB of TPDF dither."""
    return to_s16(x + rng.random(len(x)) - rng.random(len(x)))


def through_mp3(left, right, bitrate):
    """Two channels in LSB units -> the library's decode of the project's encoder's stream, float32 (the codec delays both channels alike)."""
    import mp3_encoder as E

    from mp3rgain_amd import _capi, mp3dec

    _capi.load()
    pcm = np.stack([left, right]) / 32768.0
    dec, info = mp3dec.decode(E.encode(pcm, RATE, bitrate, seed=3))
    assert info.skipped_frames == 0 and dec.shape[0] == 2
    return [np.ascontiguousarray(dec[0]), np.ascontiguousarray(dec[1])]


def scan(chans):
    """-> (the record, its lag sums) of one track on route 0."""
    import mp3rgain_amd as rg

    arena, descs = rg.replaygain.pack_tracks([rg.PcmTrack(chans, RATE)])
    recs, rows = rg.stereo_arena(None, 0, list(descs)[:1], arena, radius=RADIUS, lag_sums=True)
    return recs[0], rows[0]


def figures(chans):
    r, row = scan(chans)
    norm = math.sqrt(float(r.ell)) * math.sqrt(float(r.err))
    off = max(int(row[k]) for k in range(len(row)) if k != RADIUS) / norm if norm > 0 else 0.0
    return dict(lag=int(r.lag), lag_correlation=round(r.lag_correlation, 6), correlation=round(r.correlation, 6), off_zero_max=round(off, 6),
                beats_zero=bool(r.lag != 0 and r.lag_sum > r.elr))


def never_delayed():
    from oracle import pyoracle as po

    out = {}
    for seed in (0x5EED0001, 0x5EED0002, 0x5EED0003, 0x5EED0004):
        out[f"synth_{seed:x}"] = [po.synth_f32(seed, 0, RATE, FRAMES), po.synth_f32(seed, 1, RATE, FRAMES)]
    t = np.arange(FRAMES) / RATE
    for hz, (a, b) in ((100.0, (1.0, 0.25)), (997.0, (0.7, 0.7)), (5512.5, (0.2, 1.0)), (15000.0, (1.0, 0.9))):
        tone = 20000.0 * np.sin(2 * np.pi * hz * t)
        out[f"panned_tone_{hz:g}"] = [to_s16(a * tone), to_s16(b * tone)]
    two = 9000.0 * np.sin(2 * np.pi * 440.0 * t), 9000.0 * np.sin(2 * np.pi * 1318.5 * t + 0.3)
    out["two_tones_split"] = [to_s16(two[0] + 0.3 * two[1]), to_s16(0.3 * two[0] + two[1])]
    m, s = music(FRAMES, 21), music(FRAMES, 22)
    for g in (0.1, 0.5, 1.0, math.sqrt(2.0)):
        out[f"mix_side_{g:.2f}"] = [to_s16(0.4 * (m + g * s)), to_s16(0.4 * (m - g * s))]
    return out


def treatments(left, right, rng, mp3):
    """The five forms of a pair in LSB units (float64): name -> channels."""
    out = {"s16": [to_s16(left), to_s16(right)], "f32": [(left / 32768.0).astype(np.float32), (right / 32768.0).astype(np.float32)],
           "dithered": [dither16(left, rng), dither16(right, rng)]}
    if mp3:
        for kbps in (128, 320):
            out[f"mp3_{kbps}"] = through_mp3(left[:MP3_FRAMES], right[:MP3_FRAMES], kbps)
    return out


def measure(mp3=True):
    rows = {"never": {}, "delayed": {}, "inverted": {}}
    for name, chans in never_delayed().items():
        rows["never"][name] = figures(chans)
        print("never", name, rows["never"][name], flush=True)
    rng = np.random.default_rng(0x57E1)
    x = music(FRAMES, 7)
    for d in DELAYS:
        for form, chans in treatments(x, delayed(x, d), rng, mp3).items():
            f = figures(chans)
            f["d"] = d
            rows["delayed"][f"d{d}_{form}"] = f
            print("delayed", d, form, f, flush=True)
    for form, chans in treatments(x, -x, rng, mp3).items():
        rows["inverted"][form] = figures(chans)
        print("inverted", form, rows["inverted"][form], flush=True)
    m = dict(radius=RADIUS, frames=FRAMES, mp3_frames=MP3_FRAMES if mp3 else 0)
    # (an inverted copy was never delayed either, and a tone in it correlates half a period off)
    m["never_delayed_max"] = max((f["lag_correlation"] if f["beats_zero"] else 0.0) for kind in ("never", "inverted") for f in rows[kind].values())
    m["never_delayed_off_zero_max"] = max(f["off_zero_max"] for f in rows["never"].values())
    m["delayed_min"] = min(f["lag_correlation"] for f in rows["delayed"].values())
    m["delayed_misread"] = sorted(k for k, f in rows["delayed"].items() if f["lag"] != f["d"] or not f["beats_zero"])
    m["never_inverted_max"] = max(-f["correlation"] for f in rows["never"].values())
    m["inverted_min"] = min(-f["correlation"] for f in rows["inverted"].values())
    m["delay_permille"] = int(round(1000.0 * math.sqrt(max(m["never_delayed_max"], 1e-6) * m["delayed_min"])))
    m["phase_permille"] = int(round(1000.0 * math.sqrt(max(m["never_inverted_max"], 1e-6) * m["inverted_min"])))
    m["not_found"] = ([f"delayed copies that read another lag: {', '.join(m['delayed_misread'])}"] if m["delayed_misread"] else []) + \
                     (["delay: the classes overlap"] if m["never_delayed_max"] >= m["delayed_min"] else []) + \
                     (["phase: the classes overlap"] if m["never_inverted_max"] >= m["inverted_min"] else [])
    m["cases"] = rows
    return m


def main():
    subset = "--subset" in sys.argv
    m = measure(mp3=not subset)
    head = {k: v for k, v in m.items() if k != "cases"}
    print(json.dumps(head, indent=1))
    if "--record" in sys.argv:
        if subset:
            print("--record takes the whole run")
            return 2
        MEASURED.write_text(json.dumps(m, indent=1, sort_keys=True) + "\n")
        return 0
    old = json.loads(MEASURED.read_text())
    same = all(old["cases"][kind][k] == f for kind, cases in m["cases"].items() for k, f in cases.items())
    print("the recorded file", "agrees" if same else "DIFFERS")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
