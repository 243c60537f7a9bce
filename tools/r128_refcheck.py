#!/usr/bin/env python3
"""How exact is the float64 checker of the EBU R 128 path (tests/r128ref.py)?  Runs it against the same recursion in
np.longdouble over exactly the parity signals of tests/r128cases.py, on the CPU, and reports the worst relative error of a
gating block above the absolute gate.  tests/test_gpu_r128.py takes its tolerance from the recorded value (100 x).

    python tools/r128_refcheck.py            # print per case
    python tools/r128_refcheck.py --record   # and write tests/golden/r128_measured.json
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
    args = ap.parse_args()
    per_case, worst = {}, 0.0
    for cid, kind, rate, frames, nch, fmt, seed in r128cases.parity_cases():
        chans = r128cases.make(kind, rate, frames, nch, fmt, seed)
        z64 = r128ref.block_z(chans, rate)
        zld = r128ref.block_z(chans, rate, np.longdouble)
        above = zld >= r128ref.ABS_GATE
        err = float(np.max(np.abs(z64[above] - zld[above]) / zld[above])) if np.any(above) else 0.0
        per_case[cid] = err
        worst = max(worst, err)
        print(f"{cid:32s} blocks {len(z64):4d} above the gate {int(np.count_nonzero(above)):4d} worst relative error {err:.3e}", flush=True)
    print(f"worst relative block error: {worst:.3e}")
    if args.record:
        out = ROOT / "tests" / "golden" / "r128_measured.json"
        out.write_text(json.dumps({"what": "worst relative error of a gating block above the absolute gate, float64 checker against "
                                           "np.longdouble, over tests/r128cases.parity_cases()",
                                   "longdouble_eps": float(np.finfo(np.longdouble).eps),
                                   "worst_relative_block_error": worst, "per_case": per_case}, indent=1) + "\n")
        print(f"wrote {out}")


if __name__ == "__main__":
    main()
