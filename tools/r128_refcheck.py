#!/usr/bin/env python3
"""How exact is the float64 checker of the EBU R 128 path (tests/r128ref.py)?  Runs it against the same recursion in
np.longdouble over exactly the parity signals of tests/r128cases.py, on the CPU, and reports the worst relative error of a
gating block above the absolute gate.  tests/test_gpu_r128.py takes its tolerance from the recorded value (100 x).

    python tools/r128_refcheck.py            # print per case
    python tools/r128_refcheck.py --record   # and write tests/golden/r128_measured.json

--layout-cases runs the same measurement over the tracks of tests/layout_cases.py only (the arena-layout tests,
tests/test_gpu_arena_layouts.py) and records to tests/golden/r128_layout_measured.json.
"""
import argparse
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))
import r128cases  # noqa: E402
import r128ref  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--record", action="store_true")
    ap.add_argument("--layout-cases", action="store_true")
    args = ap.parse_args()
    if args.layout_cases:
        import layout_cases

        cases = layout_cases.r128_cases()
        name, over = "r128_layout_measured.json", "tests/layout_cases.r128_cases()"
    else:
        cases = [(c[0], r128cases.make(*c[1:]), c[2]) for c in r128cases.parity_cases()]
        name, over = "r128_measured.json", "tests/r128cases.parity_cases()"
    per_case, worst = {}, 0.0
    for cid, chans, rate in cases:
        z64 = r128ref.block_z(chans, rate)
        # a track without a block has nothing to measure: the extended-precision loop is not run for it
        zld = r128ref.block_z(chans, rate, np.longdouble) if len(z64) else z64.astype(np.longdouble)
        above = zld >= r128ref.ABS_GATE
        err = float(np.max(np.abs(z64[above] - zld[above]) / zld[above])) if np.any(above) else 0.0
        per_case[cid] = err
        worst = max(worst, err)
        print(f"{cid:32s} blocks {len(z64):4d} above the gate {int(np.count_nonzero(above)):4d} worst relative error {err:.3e}", flush=True)
    print(f"worst relative block error: {worst:.3e}")
    if args.record:
        out = ROOT / "tests" / "golden" / name
        out.write_text(json.dumps({"what": "worst relative error of a gating block above the absolute gate, float64 checker against "
                                           "np.longdouble, over " + over,
                                   "longdouble_eps": float(np.finfo(np.longdouble).eps),
                                   "worst_relative_block_error": worst, "per_case": per_case}, indent=1) + "\n")
        print(f"wrote {out}")


if __name__ == "__main__":
    main()
