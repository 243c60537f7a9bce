#!/usr/bin/env python3
"""How exact is the float64 checker of the loudness range (tests/r128range_ref.py)?  Runs it against the same recursion and the
same 30-term sums in np.longdouble over exactly the signals of tests/r128range_cases.py, on the CPU, and reports the worst
relative error of a short-term block above the absolute gate (and, beside it, of a gating block).
tests/test_gpu_r128_range.py takes its tolerance from the recorded value (100 x).

    python tools/r128_range_refcheck.py [--jobs 8]            # print per case
    python tools/r128_range_refcheck.py --record              # and write tests/golden/r128_range_measured.json
"""
import argparse
import json
import sys
from concurrent.futures import ProcessPoolExecutor
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))
import r128range_cases as cases  # noqa: E402
import r128range_ref as ref  # noqa: E402
import r128ref  # noqa: E402


def _worst(a64, ald):
    above = ald >= r128ref.ABS_GATE
    return float(np.max(np.abs(a64[above] - ald[above]) / ald[above])) if np.any(above) else 0.0, int(np.count_nonzero(above))


def one(case):
    cid, kind, rate, frames, nch, fmt, seed = case
    chans = cases.make(kind, rate, frames, nch, fmt, seed)
    e64 = r128ref.hop_energies(chans, rate)
    eld = r128ref.hop_energies(chans, rate, np.longdouble)
    st_err, st_above = _worst(ref.short_term_from(e64, rate), ref.short_term_from(eld, rate))
    hop = r128ref.hop_frames(rate)
    z = lambda e: (e[:-3] + e[1:-2] + e[2:-1] + e[3:]) / e.dtype.type(4 * hop) if len(e) >= 4 else e[:0]  # noqa: E731
    z_err, _ = _worst(z(e64), z(eld))
    return cid, max(len(e64) - 29, 0), st_above, st_err, z_err


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--record", action="store_true")
    ap.add_argument("--jobs", type=int, default=8)
    args = ap.parse_args()
    sys.path.insert(0, str(ROOT))
    from oracle import pyoracle

    pyoracle.build()  # the music signals' generator: built once, before the workers load it
    st_case, z_case = {}, {}
    with ProcessPoolExecutor(args.jobs) as pool:
        for cid, n, above, st_err, z_err in pool.map(one, cases.range_cases()):
            st_case[cid], z_case[cid] = st_err, z_err
            print(f"{cid:32s} short-term blocks {n:4d} above the gate {above:4d} worst relative error {st_err:.3e} "
                  f"(gating blocks {z_err:.3e})", flush=True)
    worst_st, worst_z = max(st_case.values()), max(z_case.values())
    print(f"worst relative short-term block error: {worst_st:.3e}; gating block error: {worst_z:.3e}")
    if args.record:
        out = ROOT / "tests" / "golden" / "r128_range_measured.json"
        out.write_text(json.dumps({"what": "worst relative error of a short-term block (and of a gating block) above the absolute gate, "
                                           "float64 checker against np.longdouble, over tests/r128range_cases.range_cases()",
                                   "longdouble_eps": float(np.finfo(np.longdouble).eps),
                                   "worst_relative_st_error": worst_st, "worst_relative_block_error": worst_z,
                                   "per_case": st_case, "per_case_block": z_case}, indent=1) + "\n")
        print(f"wrote {out}")


if __name__ == "__main__":
    main()
