#!/usr/bin/env python3
"""Where the null test's two measured thresholds come from (include/mp3rgain_amd_compare.h: lock_permille, requant_millilsb2):
synthetic material through the serial host twin (rg_compare_arena route 0; never the kernels), at the defaults (radius 1024, four
segments of 262144 frames, which for this material is the whole overlap).

    python tools/compare_refcheck.py            print every case's figures and compare with tests/golden/compare_measured.json
    python tools/compare_refcheck.py --record   write that file
    python tools/compare_refcheck.py --subset   the cases without an MP3 encode (what tests/test_compare_thresholds_cpu.py re-runs)

lock_permille.  Unrelated pairs: rg_synth.h tracks of different seeds (oracle/pyoracle.synth_f32; ALL SEEDS SHARE THE GENERATOR'S
STEADY TONES, which is what their reading reflects) and music-like signals of different seeds that share two tones as well.
Same-recording pairs: a copy +-1, +-17, +-588 and +-1023 frames from the hint; 16-bit, float and 24-bit copies; -6 dB of gain; an
inverted copy; oracle/mp3_encoder.py at 64, 128 and 320 kb/s decoded by the library's MP3 decoder (the hint is the codec's delay,
read once from the 320 kb/s stream with a wide radius); a "remaster" made here (a +-3 dB shelf and a 2:1 compressor).  The figure
is `lock`, and every same-recording pair must read its lag.
requant_millilsb2.  Same-master treatments: gains of -6, -3 and +1 dB then rounding to 16 bits with and without TPDF dither; 24
bits to 16 by truncation and by dithered rounding; float to 16 bits.  Everything else that locks: the three MP3 streams and the
remaster.  The figure is `residual_lsb2`.
Recorded: the two sides of each threshold, the defaults (the geometric mean of the two sides, in thousandths, rounded), every
case's figures, and under "not_found" the classes that did not separate.  Exit status 1 when a pair of classes does not separate.
No GPU."""
import json
import math
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
for p in (ROOT, ROOT / "tests", ROOT / "oracle"):
    sys.path.insert(0, str(p))

import numpy as np  # noqa: E402

MEASURED = ROOT / "tests" / "golden" / "compare_measured.json"
RATE, FRAMES = 44100, 3 * 44100
MP3_FRAMES = 26000  # the encoder is Python: a little over half a second per stream
OFFSETS = (1, -1, 17, -17, 588, -588, 1023, -1023)
FLOOR = 1e-3  # a side that measures 0 (a copy that nulls completely) enters the geometric mean as this


def music(n, seed, amp=3000.0):
    """Music-like: coloured noise (a one-pole low-pass at 0.95) with a slow swell plus two tones, in LSB units (float64)."""
    rng = np.random.default_rng(seed)
    w = rng.standard_normal(n + 200)
    y = np.empty_like(w)
    acc = 0.0
    for i, v in enumerate(w):
        acc = 0.95 * acc + v
        y[i] = acc
    y = y[200:] / np.std(y[200:])
    t = np.arange(n) / RATE
    y *= 0.6 + 0.4 * np.sin(2 * np.pi * 0.7 * t + seed)
    return amp * (y + 0.6 * np.sin(2 * np.pi * 440.0 * t) + 0.4 * np.sin(2 * np.pi * 1318.5 * t + 0.3))


def to_s16(x):
    return np.clip(np.rint(x), -32768, 32767).astype(np.int16)


def to_s24(x):
    """LSB units of 16 bits -> 24-bit samples in the 32-bit container."""
    return (np.clip(np.rint(x * 256.0), -(1 << 23), (1 << 23) - 1).astype(np.int64) << 8).astype(np.int32)


def to_f32(x):
    return (x / 32768.0).astype(np.float32)


def tpdf(n, rng):
    return rng.random(n) - rng.random(n)


def shifted(x, d, rng):
    """y with y[k + d] = x[k], quiet noise where nothing of x arrives."""
    y = 30.0 * rng.standard_normal(len(x))
    lo, hi = max(0, -d), min(len(x), len(x) - d)
    y[lo + d:hi + d] = x[lo:hi]
    return y


def remaster(x):
    """A +3 dB low shelf and -3 dB above it (one-pole split at about 700 Hz), then a 2:1 compressor above a threshold on a smoothed
    envelope."""
    low = np.empty_like(x)
    acc = 0.0
    for i, v in enumerate(x):
        acc += 0.1 * (v - acc)
        low[i] = acc
    y = 10 ** (3 / 20) * low + 10 ** (-3 / 20) * (x - low)
    env = np.empty_like(y)
    acc = 0.0
    for i, v in enumerate(np.abs(y)):
        acc += (0.01 if v > acc else 0.0005) * (v - acc)
        env[i] = acc
    thr = 2000.0
    gain = np.where(env > thr, np.sqrt(thr / np.maximum(env, 1.0)), 1.0)
    return y * gain


def through_mp3(x, bitrate):
    """One channel in LSB units -> the library's decode of the project's encoder's stream, float32 (with the codec's delay)."""
    import mp3_encoder as E

    from mp3rgain_amd import _capi, mp3dec

    _capi.load()
    pcm = np.stack([x, x]) / 32768.0
    dec, info = mp3dec.decode(E.encode(pcm, RATE, bitrate, seed=3))
    assert info.skipped_frames == 0
    return np.ascontiguousarray(dec[0])


def figures(a, b, hint=0, **opts):
    """-> the figures of the pair (a, b), one channel each, on route 0."""
    import mp3rgain_amd as rg
    from mp3rgain_amd import _capi

    arena, descs = rg.replaygain.pack_tracks([rg.PcmTrack([a], RATE), rg.PcmTrack([b], RATE)])
    r = rg.compare_arena(None, 0, list(descs)[:2], [(0, 1, hint)], arena, **opts)[0]
    return dict(lag=int(r.lag), polarity=int(r.polarity), lock=round(r.lock, 6), residual_lsb2=round(r.residual_lsb2, 6), gain_db=round(r.gain_db, 4),
                null_db=(round(r.null_db, 3) if math.isfinite(r.null_db) else None), at_edge=bool(r.flags & _capi.CMP_AT_EDGE),
                identical=bool(r.flags & _capi.CMP_IDENTICAL))


def unrelated():
    from oracle import pyoracle as po

    seeds = (0x5EED0001, 0x5EED0002, 0x5EED0003, 0x5EED0004)
    out = {}
    for i, s in enumerate(seeds):
        for t in seeds[i + 1:]:
            out[f"synth_{s:x}_{t:x}"] = (po.synth_f32(s, 0, RATE, FRAMES), po.synth_f32(t, 0, RATE, FRAMES))
    for s, t in ((7, 8), (7, 21), (21, 22)):
        out[f"music_{s}_{t}"] = (to_s16(music(FRAMES, s)), to_s16(music(FRAMES, t)))
    return out


def same_recording(x, rng):
    """name -> (a, b, hint, the lag it must read, its polarity)."""
    ref = to_s16(x)
    out = {f"offset{d}": (ref, to_s16(shifted(x, d, rng)), 0, d, 1) for d in OFFSETS}
    out["f32_copy"] = (ref, to_f32(x), 0, 0, 1)
    out["s24_copy"] = (ref, to_s24(x), 0, 0, 1)
    out["gain-6"] = (ref, to_s16(x * 10 ** (-6 / 20)), 0, 0, 1)
    out["inverted"] = (ref, to_s16(-x), 0, 0, -1)
    return out


def same_master(x, rng):
    n = len(x)
    out = {}
    for db in (-6, -3, 1):
        g = 10 ** (db / 20)
        out[f"gain{db:+d}_rounded"] = (to_s24(x), to_s16(g * x))
        out[f"gain{db:+d}_dithered"] = (to_s24(x), to_s16(g * x + tpdf(n, rng)))
    out["s24_truncated"] = (to_s24(x), np.floor(x).clip(-32768, 32767).astype(np.int16))
    out["s24_dithered"] = (to_s24(x), to_s16(x + tpdf(n, rng)))
    out["f32_to_s16"] = (to_f32(x), to_s16(x))
    return out


def measure(mp3=True, frames=FRAMES):
    rows = {"unrelated": {}, "same": {}, "master": {}, "other": {}}
    if frames == FRAMES:
        for name, (a, b) in unrelated().items():
            rows["unrelated"][name] = figures(a, b)
            print("unrelated", name, rows["unrelated"][name], flush=True)
    rng = np.random.default_rng(0xC0A1)
    x = music(frames, 7)
    misread = []
    for name, (a, b, hint, d, sigma) in same_recording(x, rng).items():
        f = figures(a, b, hint)
        rows["same"][name] = f
        if (f["lag"], f["polarity"]) != (hint + d, sigma):
            misread.append(name)
        print("same", name, f, flush=True)
    for name, (a, b) in same_master(x, rng).items():
        rows["master"][name] = figures(a, b)
        print("master", name, rows["master"][name], flush=True)
    rm = to_s16(remaster(x))
    rows["other"]["remaster"] = figures(to_s16(x), rm)
    print("other remaster", rows["other"]["remaster"], flush=True)
    m = dict(frames=frames, mp3_frames=MP3_FRAMES if mp3 else 0)
    if mp3:
        xs = x[:MP3_FRAMES]
        delay = figures(to_s16(xs), through_mp3(xs, 320), 0, radius=2047)["lag"]
        m["mp3_delay"] = delay
        for kbps in (320, 128, 64):
            f = figures(to_s16(xs), through_mp3(xs, kbps), delay)
            rows["other"][f"mp3_{kbps}"] = f
            if f["lag"] != delay or f["polarity"] != 1:
                misread.append(f"mp3_{kbps}")
            print("other mp3", kbps, f, flush=True)
    locked = dict(rows["same"], **rows["other"])
    m["unrelated_max"] = max((f["lock"] for f in rows["unrelated"].values()), default=None)
    m["same_min"] = min(f["lock"] for f in locked.values())
    m["same_misread"] = sorted(misread)
    m["master_max"] = max(f["residual_lsb2"] for f in rows["master"].values())
    m["other_min"] = min(f["residual_lsb2"] for f in rows["other"].values())
    m["not_found"] = [f"same-recording pairs that read another lag or polarity: {', '.join(misread)}"] if misread else []
    if m["unrelated_max"] is not None:
        m["lock_permille"] = int(round(1000.0 * math.sqrt(max(m["unrelated_max"], FLOOR) * m["same_min"])))
        if m["unrelated_max"] >= m["same_min"]:
            m["not_found"].append("lock: the classes overlap")
    m["requant_millilsb2"] = int(round(1000.0 * math.sqrt(max(m["master_max"], FLOOR) * m["other_min"])))
    if m["master_max"] >= m["other_min"]:
        m["not_found"].append("requant: the classes overlap")
    m["cases"] = rows
    return m


def main():
    subset = "--subset" in sys.argv
    m = measure(mp3=not subset)
    print(json.dumps({k: v for k, v in m.items() if k != "cases"}, indent=1))
    if m["not_found"]:
        print("NOT SEPARATED:", "; ".join(m["not_found"]))
        return 1
    if "--record" in sys.argv:
        if subset:
            print("--record takes the whole run")
            return 2
        MEASURED.write_text(json.dumps(m, indent=1, sort_keys=True) + "\n")
        return 0
    old = json.loads(MEASURED.read_text())
    same = all(old["cases"][kind].get(k) == f for kind, cases in m["cases"].items() for k, f in cases.items())
    print("the recorded file", "agrees" if same else "DIFFERS")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
