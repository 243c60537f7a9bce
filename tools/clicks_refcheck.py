#!/usr/bin/env python3
"""Where the click scan's measured default comes from (include/mp3rgain_amd_clicks.h: ratio_permille): synthetic material
through the serial host twin (rg_clicks_arena route 0; never the kernels), every other option at its default.

    python tools/clicks_refcheck.py            print every case's figures and compare with tests/golden/clicks_measured.json
    python tools/clicks_refcheck.py --record   write that file

Undamaged material, by kind: rg_synth.h tracks of 12 s (oracle/pyoracle.synth_f32; one of them hot, all with the one-second
silence gap), tone mixes over a noise floor of 2^-13 of full scale, partly tonal mixes (coloured noise and two tones), the tempo
cases' drum pattern, the tone mix and the partly tonal mix through oracle/mp3_encoder.py at 128 and 320 kb/s decoded by the
library's MP3 decoder (faded in and out over 20 ms: a stream that starts in mid-wave has a click of its own), and both as
24-bit integers and as float.  Each is scanned at every ratio of a ladder from PROBE (4 x the scale) upwards in steps of 4 %
until nothing is flagged any more, and its figure is the strength of the strongest CLICK read at ANY of them: at a low ratio a
strong sample may sit inside a wide event, which is a burst there, and become a click of its own higher up.  `undamaged_max` is
the largest figure of the kinds counted clean.  THE DRUM PATTERN IS NOT COUNTED CLEAN (NOT_CLEAN): its snare and hat are noise
that starts at full level within one sample, which is what this detector looks for; it is measured like the others and
reported as a false positive with its numbers.  At the end every clean kind is scanned at the recorded default and must read no
clicks, and every claimed class must be found at it.
Damaged material: defects planted into the 16-bit tone mix and the 16-bit partly tonal mix at PLACES, one class per copy:
single-sample impulses of 1/64 .. 1/2 of full scale (alternating sign), a run of 4 stuck samples, skips of 1, 10 and 588
samples, a repeated 588-sample sector.  Each copy is scanned at ratio_permille = undamaged_max + 1, where nothing undamaged is
flagged, with a list of 256 events; a planted defect is FOUND when an event starts within `gap` of its place, and its strength
is the strongest such event's.  A class (defect x material) is CLAIMED when every one of its defects is found and the weakest of
them reads at least MARGIN (1.5) times `undamaged_max` -- a class that clears the undamaged side by a hair is not one to promise;
otherwise it goes under `not_found` with its numbers.  `ratio_permille`, the default, is the geometric mean of `undamaged_max`
and `claimed_min`, the smallest strength of the claimed classes.  No GPU."""
import json
import math
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
for p in (ROOT, ROOT / "tests", ROOT / "oracle"):
    sys.path.insert(0, str(p))

import numpy as np  # noqa: E402

MEASURED = ROOT / "tests" / "golden" / "clicks_measured.json"
RATE, FRAMES, SYNTH_FRAMES = 44100, 3 * 44100, 12 * 44100
MP3_FRAMES = 26000  # the encoder is Python: a little over half a second per stream
PROBE = 4000
GAP = 16
MARGIN = 1.5  # a stated convention of this tool
NOT_CLEAN = ("drums",)  # kinds measured and reported, but not counted as the undamaged side (see the docstring)
PLACES = tuple(9000 + 12007 * k for k in range(10))  # ten places, none on a block's seam
IMPULSES = (64, 32, 16, 8, 4, 2)                      # 1 / these of full scale


def tone_mix(n, seed, floor=4.0):
    """Three tones over a Gaussian noise floor of `floor` LSB (2^-13 of full scale), in LSB units (float64)."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / RATE
    return 7000.0 * np.sin(2 * np.pi * 220.0 * t) + 4000.0 * np.sin(2 * np.pi * 1318.5 * t + 0.3) + 2000.0 * np.sin(2 * np.pi * 3520.0 * t + 1.1) + \
        floor * rng.standard_normal(n)


def music(n, seed, amp=3000.0):
    """Partly tonal: coloured noise (a one-pole low-pass at 0.95) plus two tones, in LSB units (float64)."""
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


def to_s24(x):
    """24-bit samples in the arena's 32-bit container."""
    return (np.clip(np.rint(x * 256.0), -(1 << 23), (1 << 23) - 1).astype(np.int64) << 8).astype(np.int32)


def to_f32(x):
    return (x / 32768.0).astype(np.float32)


def through_mp3(x, bitrate):
    """One signal in LSB units, faded in and out over 20 ms, as both channels -> the library's decode of the project's encoder's
    stream, float32."""
    import mp3_encoder as E

    from mp3rgain_amd import _capi, mp3dec

    _capi.load()
    fade = int(0.02 * RATE)  # a stream that starts or stops in mid-wave has a click of its own there
    ramp = 0.5 - 0.5 * np.cos(np.pi * np.arange(fade) / fade)
    x = x.copy()
    x[:fade] *= ramp
    x[-fade:] *= ramp[::-1]
    pcm = np.stack([x, x]) / 32768.0
    dec, info = mp3dec.decode(E.encode(pcm, RATE, bitrate, seed=3))
    assert info.skipped_frames == 0 and dec.shape[0] == 2
    return [np.ascontiguousarray(dec[0]), np.ascontiguousarray(dec[1])]


def scan(chans, ratio, events=0):
    """-> one track's Clicks on route 0."""
    import mp3rgain_amd as rg

    arena, descs = rg.replaygain.pack_tracks([rg.PcmTrack(chans, RATE)])
    recs, rows = rg.clicks_arena(None, 0, list(descs)[:1], arena, ratio_permille=ratio, max_events=events)
    return rg.clicks_from_record(recs[0], rows)


def undamaged(mp3=True):
    from oracle import pyoracle as po
    import tempo_cases as tc

    out = {}
    for name, seed in (("synth_1", 0x5EED0001), ("synth_2", 0x5EED0002), ("synth_hot", 0x5EED0003 | (1 << 40))):
        out[name] = ("synth", [po.synth_f32(seed, 0, RATE, SYNTH_FRAMES), po.synth_f32(seed, 1, RATE, SYNTH_FRAMES)])
    tones, mixes = [tone_mix(FRAMES, 31), tone_mix(FRAMES, 32)], [music(FRAMES, 21), music(FRAMES, 22)]
    out["tonal_s16"] = ("tonal", [to_s16(v) for v in tones])
    out["mixed_s16"] = ("mixed", [to_s16(v) for v in mixes])
    out["tonal_s24"] = ("tonal_24", [to_s24(v) for v in tones])
    out["mixed_s24"] = ("mixed_24", [to_s24(v) for v in mixes])
    out["tonal_f32"] = ("tonal_float", [to_f32(v) for v in tones])
    out["mixed_f32"] = ("mixed_float", [to_f32(v) for v in mixes])
    out["drums"] = ("drums", [to_s16(20000.0 * tc.drum_pattern(120.0, RATE, 3.0)), to_s16(20000.0 * tc.drum_pattern(97.0, RATE, 3.0, seed=5))])
    if mp3:
        for kbps in (128, 320):
            out[f"tonal_mp3_{kbps}"] = (f"mp3_{kbps}", through_mp3(tones[0][:MP3_FRAMES], kbps))
            out[f"mixed_mp3_{kbps}"] = (f"mp3_{kbps}", through_mp3(mixes[0][:MP3_FRAMES], kbps))
    return out


def damaged():
    """name -> (defect class, material, channels, [the windows [a, b] in which each planted defect has to be found])."""
    out = {}
    for material, x in (("tonal", tone_mix(FRAMES, 31)), ("mixed", music(FRAMES, 21))):
        for d in IMPULSES:
            y = x.copy()
            for k, p in enumerate(PLACES):
                y[p] += (32768.0 / d) * (1 if k % 2 == 0 else -1)
            out[f"impulse_1/{d}_{material}"] = (f"impulse_1/{d}", material, [to_s16(y)], [(p - GAP, p + GAP) for p in PLACES])
        y = x.copy()
        for p in PLACES:
            y[p + 1:p + 4] = y[p]
        out[f"stuck_4_{material}"] = ("stuck_4", material, [to_s16(y)], [(p - GAP, p + 3 + GAP) for p in PLACES])
        for k in (1, 10, 588):
            keep = np.ones(len(x), bool)
            for p in PLACES:
                keep[p:p + k] = False
            at = [p - k * j for j, p in enumerate(PLACES)]  # where each cut lies once the earlier ones are gone
            out[f"skip_{k}_{material}"] = (f"skip_{k}", material, [to_s16(x[keep])], [(a - GAP, a + GAP) for a in at])
        parts, at, last = [], [], 0
        for j, p in enumerate(PLACES):  # the sector [p, p + 588) twice
            parts += [x[last:p + 588], x[p:p + 588]]
            at.append(p + 588 + 588 * j)
            last = p + 588
        parts.append(x[last:])
        out[f"repeat_588_{material}"] = ("repeat_588", material, [to_s16(np.concatenate(parts))], [(a - GAP, a + GAP) for a in at])
    return out


def ladder(chans):
    """One undamaged file scanned at every ratio of a ladder from PROBE up in steps of 4 % until nothing is flagged any more: the
    strongest click at ANY of them (a strong sample inside a wide event at a low ratio is a burst there and becomes a click
    higher up), the highest ratio at which a click was read, and the highest at which a sample was flagged."""
    best, click_ratio, flag_ratio, r, first = 0, 0, 0, PROBE, None
    while r <= 1000000:
        c = scan(chans, r)
        first = first or c
        if not sum(ch.flagged for ch in c.ch):
            break
        flag_ratio = r
        if c.clicks:
            best, click_ratio = max(best, max(ch.strongest_permille for ch in c.ch)), r
        r = int(r * 1.04) + 1
    return first, best, click_ratio, flag_ratio


def reading(c):
    return dict(clicks=c.clicks, bursts=c.bursts, strongest_click=max(ch.strongest_permille for ch in c.ch), widest=max(ch.widest for ch in c.ch))


def measure(mp3=True):
    rows = {"undamaged": {}, "damaged": {}}
    kinds, material = {}, undamaged(mp3)
    for name, (kind, chans) in material.items():
        first, best, click_ratio, flag_ratio = ladder(chans)
        f = dict(kind=kind, strongest_click=best, highest_ratio_with_a_click=click_ratio, highest_ratio_with_a_flagged_sample=flag_ratio,
                 at_probe=reading(first), median_max=max(c.median_max for c in first.ch), fallback_blocks=sum(c.fallback_blocks for c in first.ch))
        rows["undamaged"][name] = f
        kinds[kind] = max(kinds.get(kind, 0), f["strongest_click"])
        print("undamaged", name, f, flush=True)
    U = max(v for k, v in kinds.items() if k not in NOT_CLEAN)
    classes = {}
    for name, (cls, mat, chans, windows) in damaged().items():
        r = scan(chans, U + 1, 256)
        found = []
        for a, b in windows:
            near = [e.strength_permille for e in r.events if a <= e.start <= b]
            found.append(max(near) if near else 0)
        f = dict(defect=cls, material=mat, planted=len(windows), found=sum(1 for v in found if v), strengths=found,
                 smallest=min([v for v in found if v], default=0), events=r.events_total, clicks=r.clicks, bursts=r.bursts)
        rows["damaged"][name] = f
        classes[name] = f
        print("damaged", name, f, flush=True)
    claimed = sorted(n for n, f in classes.items() if f["found"] == f["planted"] and f["smallest"] >= MARGIN * U)
    m = dict(frames=FRAMES, synth_frames=SYNTH_FRAMES, mp3_frames=MP3_FRAMES if mp3 else 0, probe_permille=PROBE, margin=MARGIN, places=list(PLACES))
    m["undamaged_max_by_kind"] = kinds
    m["not_clean_kinds"] = list(NOT_CLEAN)
    m["undamaged_max"] = U
    m["claimed"] = claimed
    m["claimed_min"] = min(classes[n]["smallest"] for n in claimed) if claimed else 0
    m["not_found"] = {n: dict(found=f["found"], planted=f["planted"], smallest=f["smallest"]) for n, f in classes.items() if n not in claimed}
    m["ratio_permille"] = int(round(math.sqrt(float(U) * float(m["claimed_min"])))) if claimed else 0
    # the default held to the material it was made from: the clean kinds read no clicks at it, the others are false positives
    m["at_default"] = {}
    for name, (kind, chans) in material.items():
        f = reading(scan(chans, max(m["ratio_permille"], 1000)))
        f["kind"] = kind
        m["at_default"][name] = f
        if kind not in NOT_CLEAN:
            assert f["clicks"] == 0, (name, f)
    m["false_positives_at_default"] = {n: f for n, f in m["at_default"].items() if f["clicks"]}
    # ... and the claimed classes all found at it
    m["claimed_at_default"] = {}
    made = damaged()
    for name in claimed:
        _, _, chans, windows = made[name]
        r = scan(chans, m["ratio_permille"], 256)
        got = sum(1 for a, b in windows if any(a <= e.start <= b for e in r.events))
        m["claimed_at_default"][name] = dict(found=got, planted=len(windows), events=r.events_total)
        assert got == len(windows), (name, got)
    m["cases"] = rows
    return m


def main():
    m = measure()
    print(json.dumps({k: v for k, v in m.items() if k != "cases"}, indent=1))
    if "--record" in sys.argv:
        MEASURED.write_text(json.dumps(m, indent=1, sort_keys=True) + "\n")
        return 0
    old = json.loads(MEASURED.read_text())
    same = all(old["cases"][kind][k] == f for kind, cases in m["cases"].items() for k, f in cases.items())
    print("the recorded file", "agrees" if same else "DIFFERS")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
