#!/usr/bin/env python3
"""How far the spectrum kernels' f32 arithmetic is from the float64 definitions: route 2 of rg_spectrum_arena (the kernels'
butterflies, tables, tile and fold order on the host; the kernels themselves are held to it byte for byte) against the numpy
restatement of tests/spectrum_cases.py, over the shared cases.  Per channel of every case: max_j |dE[j]| / sum_j E_ref[j], and
for the bands that hold at least 1e-4 of the total the worst relative error.  Needs no GPU.

  python tools/spectrum_refcheck.py            # print the table
  python tools/spectrum_refcheck.py --record   # and write tests/golden/spectrum_measured.json, which bounds the tests"""
import argparse
import json
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))

import arena_layouts as al  # noqa: E402
import spectrum_cases as sc  # noqa: E402

import mp3rgain_amd as rg  # noqa: E402


def measure():
    tracks, wants = sc.tracks(), sc.wants()
    arena, descs, _ = al.pack(tracks, al.Layout("guard", "loud", "input", 3))
    recs, e = rg.spectrum_arena(None, 2, list(descs)[:len(tracks)], arena)
    cases = {}
    for i, tr in enumerate(tracks):
        worst = (0.0, 0.0)
        for c, (ref, analysed, skipped) in enumerate(wants[tr.name]):
            if (recs[i].ch[c].analysed_frames, recs[i].ch[c].skipped_frames) != (analysed, skipped):
                raise SystemExit(f"{tr.name} channel {c}: frames {recs[i].ch[c].analysed_frames} + {recs[i].ch[c].skipped_frames}, expected {analysed} + {skipped}")
            of_total, relative = sc.errors(e[i, c], ref)
            worst = (max(worst[0], of_total), max(worst[1], relative))
        cases[tr.name] = {"of_total": worst[0], "relative": worst[1]}
    return cases


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--record", action="store_true", help="write tests/golden/spectrum_measured.json")
    a = ap.parse_args()
    cases = measure()
    for name, c in cases.items():
        print(f"{name:28s} of total {c['of_total']:.3e}   relative {c['relative']:.3e}")
    rec = {"tool": "tools/spectrum_refcheck.py", "route": 2, "reference": "float64 numpy restatement (tests/spectrum_cases.py)",
           "frames_per_tile": sc.shape()[3],
           "worst_of_total": max(c["of_total"] for c in cases.values()), "worst_relative": max(c["relative"] for c in cases.values()),
           "cases": cases}
    print(f"worst: of total {rec['worst_of_total']:.3e}, relative {rec['worst_relative']:.3e}")
    if a.record:
        sc.MEASURED.write_text(json.dumps(rec, indent=1) + "\n")
        print(f"wrote {sc.MEASURED.relative_to(ROOT)}")


if __name__ == "__main__":
    main()
