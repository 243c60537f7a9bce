#!/usr/bin/env python3
"""The float64 restatement of the key scan (tests/key_cases.py: the filter's table applied in float64, numpy.fft.rfft and Python
integers) over the shared case list, against the host routes (rg_key_arena routes 0 and 2; never the kernels against
themselves), and over the synthetic chord progressions, against the key they were generated in.

    python tools/key_refcheck.py            print the figures and compare with tests/golden/key_measured.json
    python tools/key_refcheck.py --record   write that file

Recorded:
 1. the decimated signal: the largest error of y from routes 0 and 2 against the reference over the shared cases, relative to
    the track's largest |y|; band energies: the largest error of E, relative to the frame's largest band energy; rows: the share
    of row entries in which a route differs from the reference, and the largest difference (a band energy next to a step of q
    moves an entry by one; a band next to the frame's largest moves up to five entries of a row);
 2. the progressions (I-IV-V-I-vi-IV-V-I with a bass root, six harmonics at 1/k, a scale-tone melody, 40 s; all 24 keys at
    44100, 48000 and 96000 Hz) through route 2 at the defaults: every one must read its generating key, and the ranges of
    correlation, margin and stability are recorded, with the correlation of white noise and the verdict of digital silence.
No GPU."""
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT))

import numpy as np  # noqa: E402

import key_cases as kc  # noqa: E402


def slices(recs, y, bands, chroma):
    ya = 0
    for r in recs:
        yield y[ya:ya + r.decimated], bands[r.chroma_at:r.chroma_at + r.rows].astype(np.float64), chroma[r.chroma_at:r.chroma_at + r.rows]
        ya += r.decimated


def shared_cases():
    import mp3rgain_amd as rg

    cs = kc.cases()
    arena, descs = kc.pack(cs)
    refs = [kc.reference(c) for c in cs]
    out = {}
    for route in (0, 2):
        recs, y, bands, chroma = rg.key_arena(None, route, descs, arena)
        yerr = berr = 0.0
        differ = largest = total = 0
        for c, r, ref, (yy, E, rows) in zip(cs, recs, refs, slices(recs, y, bands, chroma)):
            assert (r.decim if ref.supported else 0, r.decimated, r.rows, r.nonfinite_frames) == (ref.decim if ref.supported else 0, len(ref.y), ref.frames, ref.nonfinite), c.name
            yerr = max(yerr, kc.y_error(yy, ref.y))
            berr = max(berr, kc.band_error(E, ref.bands))
            d = np.abs(rows.astype(np.int64) - ref.rows.astype(np.int64))
            differ += int((d != 0).sum())
            largest = max(largest, int(d.max(initial=0)))
            total += d.size
        out[route] = dict(y_error=yerr, band_error=berr, differing=differ, largest=largest, entries=total)
    return out


def reading(planes, rate, segment=None):
    import mp3rgain_amd as rg

    arena, descs = kc.pack([kc.Case("x", [planes], rate)])
    return rg.key_arena(None, 2, descs, arena, segment=segment, bands=False)[0][0]


def measure():
    import mp3rgain_amd as rg

    shared = shared_cases()
    print("shared cases:", shared, flush=True)
    corr, margin, stable, rows, wrong = {r: [] for r in kc.TRUTH_RATES}, [], [], {}, []
    for rate, key in kc.truth_cases():
        r = reading(kc.truth_planes(rate, key), rate)
        if r.key != key or r.flags & 0x13:
            wrong.append((rate, key, r.key, r.flags))
        corr[rate].append(r.correlation_permille)
        margin.append(r.margin_permille)
        stable.append(r.stable_permille)
        rows[f"{rate}_{key}"] = [rg.key_name(r.key), r.correlation_permille, r.margin_permille, r.stable_permille]
        print(rate, rg.key_name(key), rows[f"{rate}_{key}"], flush=True)
    assert not wrong, wrong
    noise = [reading(kc.white_noise(rate), rate).correlation_permille for rate in kc.TRUTH_RATES]
    silence = reading(np.zeros(44100 * 10, np.int16), 44100)
    m = dict(readings=rows, right=len(rows), cases=len(rows), noise_correlation_min=min(noise), noise_correlation_max=max(noise),
             silence_flags=int(silence.flags), margin_min=min(margin), margin_max=max(margin), stable_min=min(stable))
    for rate in kc.TRUTH_RATES:
        m[f"correlation_min_{rate}"], m[f"correlation_max_{rate}"] = min(corr[rate]), max(corr[rate])
    for route, d in shared.items():
        m[f"y_error_route{route}"] = d["y_error"]
        m[f"band_error_route{route}"] = d["band_error"]
        m[f"differing_entries_route{route}"] = d["differing"]
        m[f"differing_share_route{route}"] = d["differing"] / d["entries"]
        m[f"entries_route{route}"] = d["entries"]
    m["largest_entry_difference"] = max(d["largest"] for d in shared.values())
    return m


def main():
    m = measure()
    head = {k: v for k, v in m.items() if k != "readings"}
    print(json.dumps(head, indent=1))
    if "--record" in sys.argv:
        kc.MEASURED.write_text(json.dumps(m, indent=1, sort_keys=True) + "\n")
        return 0
    old = json.loads(kc.MEASURED.read_text())
    same = all(old[k] == v for k, v in head.items())
    print("the recorded file", "agrees" if same else "DIFFERS")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
