#!/usr/bin/env python3
"""The float64 restatement of the tempo scan (tests/tempo_cases.py, numpy.fft.rfft and Python integers) over the shared case
list, against the host routes (rg_tempo_arena routes 0 and 2; never the kernels against themselves), and over the synthetic
rhythmic material, against the tempo it was generated at.

    python tools/tempo_refcheck.py            print the figures and compare with tests/golden/tempo_measured.json
    python tools/tempo_refcheck.py --record   write that file

Recorded:
 1. band energies: the largest error of E from routes 0 and 2 against the reference over the shared cases, relative to the
    frame's largest band energy; onsets: the share of onsets in which a route differs from the reference (route 0 over the
    shared cases, route 2 over those and the rhythmic material below), and the largest difference (a band energy next to a
    step of q moves an onset by a quarter of a step);
 2. the rhythmic material (click tracks and a kick / snare / hat pattern, 40 s, 44100 and 48000 Hz, nine tempi) through the
    restatement at the defaults: the largest relative error of the reading against the generating BPM, the ranges of
    confidence and stability, the readings of 60, 170 and 200 BPM (the octave convention) and the confidence of white noise;
 3. the beat bias: per click track the offset between the first true click and the best phase's grid (bias 0), folded into half
    a period around 0; RG_TEMPO_BEAT_BIAS is their median, and the spread is recorded.
No GPU."""
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT))

import numpy as np  # noqa: E402

import tempo_cases as tc  # noqa: E402


def shared_cases():
    import mp3rgain_amd as rg

    cs = tc.cases()
    arena, descs = tc.pack(cs)
    err, differ, largest, total = {0: 0.0, 2: 0.0}, {0: 0, 2: 0}, {0: 0, 2: 0}, 0
    refs = [tc.reference(c) for c in cs]
    for route in (0, 2):
        recs, onsets, bands = rg.tempo_arena(None, route, descs, arena)
        at = 0
        for c, r, ref in zip(cs, recs, refs):
            assert (r.band_frames, r.onsets, r.nonfinite_frames) == (ref.frames, len(ref.onsets), ref.nonfinite), c.name
            err[route] = max(err[route], tc.band_error(bands[at:at + r.band_frames].astype(np.float64), ref.bands))
            at += r.band_frames
            d = np.abs(onsets[r.onsets_at:r.onsets_at + r.onsets].astype(np.int64) - ref.onsets.astype(np.int64))
            differ[route] += int((d != 0).sum())
            largest[route] = max(largest[route], int(d.max(initial=0)))
        total = sum(int(r.onsets) for r in recs)
    return err, differ, largest, total


def fold(x, period):
    return (x + period / 2.0) % period - period / 2.0


def reading(planes, rate, count=None):
    """The restatement's reading of one plane; count[0], count[1] += the onsets in which route 2 differs from it, and all."""
    case = tc.Case("x", [planes], rate)
    ref = tc.reference_signal(tc.signal(case), rate)
    if count is not None:
        import mp3rgain_amd as rg

        arena, descs = tc.pack([case])
        onsets = rg.tempo_arena(None, 2, descs, arena, bands=False)[1]
        d = np.abs(onsets.astype(np.int64) - ref.onsets.astype(np.int64))
        count[0] += int((d != 0).sum())
        count[1] += len(d)
        count[2] = max(count[2], int(d.max(initial=0)))
    return tc.ref_stage2(ref.onsets, rate, bias=0)[0]


def measure():
    err, differ, largest, total = shared_cases()
    print("shared cases: band error", err, "differing onsets", differ, "of", total, "largest", largest, flush=True)
    rel, conf, stable, offsets, rows = 0.0, [], [], {"click": [], "drums": []}, {}
    count = [differ[2], total, largest[2]]  # route 2 against the reference, the rhythmic material included
    for kind, rate, bpm in tc.truth_cases():
        r = reading(tc.truth_planes(kind, rate, bpm), rate, count)
        got = r["bpm_milli"] / 1000.0
        e = abs(got - bpm) / bpm
        period = r["period16"] * 32.0
        off = fold(tc.FIRST_BEAT * rate - r["first_beat"], period)
        rel = max(rel, e)
        conf.append(r["confidence_permille"])
        stable.append(r["stable_permille"])
        offsets[kind].append(off)
        rows[f"{kind}_{rate}_{bpm}"] = [got, round(e, 5), r["confidence_permille"], r["stable_permille"], round(off, 1)]
        print(kind, rate, bpm, rows[f"{kind}_{rate}_{bpm}"], flush=True)
    octave = {}
    for bpm, want in tc.OCTAVE_BPMS:
        for rate in tc.TRUTH_RATES:
            r = reading(tc.fc.as_format(tc.click_track(bpm, rate) * 32768.0 * 0.9, "s16"), rate)
            octave[f"{bpm}_{rate}"] = r["bpm_milli"] / 1000.0
            assert abs(octave[f"{bpm}_{rate}"] - want) / want < 0.02, (bpm, rate, octave)
    noise = max(reading(tc.white_noise(rate), rate)["confidence_permille"] for rate in tc.TRUTH_RATES)
    clicks = np.array(offsets["click"])
    bias = int(round(float(np.median(clicks))))
    return dict(band_error_route0=err[0], band_error_route2=err[2], onsets_route0=total, differing_onsets_route0=differ[0],
                differing_share_route0=differ[0] / total, onsets_route2=count[1], differing_onsets_route2=count[0],
                differing_share_route2=count[0] / count[1], largest_onset_difference=max(largest[0], count[2]),
                relative_error_max=round(rel, 5), confidence_min=min(conf), confidence_max=max(conf), stable_min=min(stable),
                octave_readings=octave, noise_confidence=noise, beat_bias=bias, click_offset_min=round(float(clicks.min()), 1),
                click_offset_max=round(float(clicks.max()), 1), drums_offset_min=round(float(min(offsets["drums"])), 1),
                drums_offset_max=round(float(max(offsets["drums"])), 1), readings=rows)


def main():
    m = measure()
    head = {k: v for k, v in m.items() if k != "readings"}
    print(json.dumps(head, indent=1))
    from mp3rgain_amd import _capi

    if m["beat_bias"] != _capi.TEMPO_BEAT_BIAS:
        print(f"RG_TEMPO_BEAT_BIAS is {_capi.TEMPO_BEAT_BIAS}, the measured median {m['beat_bias']}")
    if "--record" in sys.argv:
        tc.MEASURED.write_text(json.dumps(m, indent=1, sort_keys=True) + "\n")
        return 0
    old = json.loads(tc.MEASURED.read_text())
    same = all(old[k] == v for k, v in head.items())
    print("the recorded file", "agrees" if same else "DIFFERS")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
