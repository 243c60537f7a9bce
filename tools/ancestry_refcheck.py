#!/usr/bin/env python3
"""The float64 reference of the ancestry scan (tests/ancestry_cases.py) over the shared case list, against the serial host twin
(rg_ancestry_arena route 0; never the kernels against themselves).

    python tools/ancestry_refcheck.py            print every case's figures and compare with tests/golden/ancestry_measured.json
    python tools/ancestry_refcheck.py --record   write that file

Recorded: the largest z and the largest iso of any never-coded case; the smallest z and iso of any coded case that is expected
to be found (of its strongest view); the defaults of z_min and iso_min, each the geometric mean of its two sides; the worst
|small_f32 - small_f64| / active and |active_f32 - active_f64| / active_f64 over all cases, views and alignments with
active >= 1; every case's figures.  No GPU."""
import json
import math
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT))

import numpy as np  # noqa: E402

import ancestry_cases as ac  # noqa: E402


def measure():
    import mp3rgain_amd as rg

    rows = {}
    worst_small = worst_active = 0.0
    for case in ac.cases():
        ref = ac.reference(case.name, False)
        arena, descs = ac.pack_one(case)
        recs, cnt = rg.ancestry_arena(None, 0, descs, arena, case.segments, case.granules)
        for v, (small, active) in enumerate(ref["counts"]):
            on = active >= 1
            if on.any():
                worst_small = max(worst_small, float((np.abs(cnt[0, v, 0].astype(np.int64) - small)[on] / active[on]).max()))
                worst_active = max(worst_active, float((np.abs(cnt[0, v, 1].astype(np.int64) - active)[on] / active[on]).max()))
        strongest = max(ref["views"], key=lambda w: w["z"])
        finite_iso = [w["iso"] for w in ref["views"] if math.isfinite(w["iso"])]
        rows[case.name] = dict(kind=case.kind, expected_offset=case.offset, offset=strongest["offset"], view=strongest["kind"],
                               z=round(strongest["z"], 4), iso=round(strongest["iso"], 4) if math.isfinite(strongest["iso"]) else None,
                               ratio=round(strongest["ratio"], 5), second=round(strongest["second"], 5), p0=round(strongest["p0"], 5),
                               max_z=round(max(w["z"] for w in ref["views"]), 4), max_iso=round(max(finite_iso), 4) if finite_iso else None,
                               route0_offset=int(recs[0].view[ref["views"].index(strongest)].offset))
        print(case.name, rows[case.name], flush=True)
    clean = [r for r in rows.values() if r["kind"] == "clean"]
    found = [r for r in rows.values() if r["kind"] == "found"]
    m = dict(never_coded_max_z=max(r["max_z"] for r in clean), never_coded_max_iso=max(r["max_iso"] for r in clean if r["max_iso"] is not None),
             coded_min_z=min(r["z"] for r in found), coded_min_iso=min(r["iso"] for r in found),
             worst_small_error=worst_small, worst_active_error=worst_active, active_floor=ac.ACTIVE_FLOOR)
    m["z_min"] = round(math.sqrt(m["never_coded_max_z"] * m["coded_min_z"]), 2)
    m["iso_min"] = round(math.sqrt(m["never_coded_max_iso"] * m["coded_min_iso"]), 3)
    m["cases"] = rows
    return m


def main():
    m = measure()
    head = {k: v for k, v in m.items() if k != "cases"}
    print(json.dumps(head, indent=1))
    if "--record" in sys.argv:
        ac.MEASURED.write_text(json.dumps(m, indent=1, sort_keys=True) + "\n")
        return 0
    old = json.loads(ac.MEASURED.read_text())
    same = all(old[k] == v for k, v in head.items())
    print("the recorded file", "agrees" if same else "DIFFERS")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
