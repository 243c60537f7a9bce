#!/usr/bin/env python3
"""The rates of the click scan's kernels (MI355X) and of their serial host twin: 1000 tracks of three minutes of 44.1 kHz 16-bit
stereo filled on the device with pseudo-random samples (rg_clicks_rate), beside DR's read-floor kernel over an arena of the same
shape (rg_dr_rate) run by the same process.

    tools/clicks_rate.py [--tracks 1000] [--seconds 180] [--host-tracks 16] [--threads 16] [--reps 5] [--warm-ms 400] [--emit-ratio 1.99]
                         [--json profiles/clicks_rate.json]

Per call of a hook: after a warm-up (the legs launched in turn for `warm-ms` milliseconds), `reps` rounds alternate over one
arena, HIP events around the launches alone; medians and the spread (min .. max) are reported.
  1. the tile kernel (scan), the fold kernel and the emit kernel at the defaults, where the uniform fill has no event and the emit
     leg is empty, and at a ratio of 1.99, where every plane fills its list and the emit kernel runs over a tile or two of every
     plane; the scan as bytes of PCM per second and as multiply-adds of the definition per second, beside DR's read floor (each
     hook fills its own arena and runs its own rounds: the legs share the process, they do not alternate with the floor);
  2. the same at block lengths 256 and 4096, whose tiles hold 46 blocks and 1;
  3. the serial host twin on `threads` threads over a host copy of the first `host-tracks` tracks, its time scaled to the count.
     Every host record and event list must equal the kernels'."""
import argparse
import ctypes as C
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

HBM_PEAK_GB_S = 8000.0      # MI355X: 8 TB/s
# the fill is uniform, not Gaussian: its residual never exceeds twice its median, so nothing is flagged at the defaults.  Just below
# 2 about one sample in 400 is, every plane fills its list of 16 within its first tile or two, and the emit kernel has work
EMIT_RATIO = 1990


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tracks", type=int, default=1000)
    ap.add_argument("--seconds", type=float, default=180.0)
    ap.add_argument("--host-tracks", type=int, default=16)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warm-ms", type=float, default=400.0)
    ap.add_argument("--emit-ratio", type=float, default=EMIT_RATIO / 1000.0, help="the ratio of the leg that gives the emit kernel work")
    ap.add_argument("--json", default=str(ROOT / "profiles" / "clicks_rate.json"))
    a = ap.parse_args()
    import torch  # noqa: F401  (torch first: one HIP runtime per process)

    import mp3rgain_amd as rg
    from mp3rgain_amd import _capi

    L = _capi.load()
    n, frames = a.tracks, int(44100 * a.seconds)
    host_n = min(n, a.host_tracks)
    med = statistics.median
    stage = lambda x: {"ms": med(x), "ms_min": min(x), "ms_max": max(x), "ms_all": list(x)}  # noqa: E731
    legs, mismatches = [], 0
    D = _capi
    runs = ((D.FMT_S16_PLANAR, "s16", D.CK_DEFAULT_BLOCK, D.CK_DEFAULT_RATIO_PERMILLE, host_n), (D.FMT_S16_PLANAR, "s16", D.CK_DEFAULT_BLOCK, int(round(a.emit_ratio * 1000)), host_n),
            (D.FMT_S16_PLANAR, "s16", 256, D.CK_DEFAULT_RATIO_PERMILLE, 0), (D.FMT_S16_PLANAR, "s16", 4096, D.CK_DEFAULT_RATIO_PERMILLE, 0),
            (D.FMT_F32_PLANAR, "f32", D.CK_DEFAULT_BLOCK, D.CK_DEFAULT_RATIO_PERMILLE, 0))
    with rg.Analyzer(0) as an:
        for fmt, name, block, ratio, hosts in runs:
            scan, fold, emit, host = ((C.c_double * a.reps)() for _ in range(4))
            bad, nbytes, macs = C.c_size_t(), C.c_uint64(), C.c_uint64()
            o = D.ClicksOpts(block, D.CK_DEFAULT_ORDER, ratio, D.CK_DEFAULT_FLOOR, D.CK_DEFAULT_GAP, D.CK_DEFAULT_MAX_WIDTH, D.CK_DEFAULT_MAX_EVENTS)
            an._check(L.rg_clicks_rate(an.handle, n, frames, fmt, C.byref(o), hosts, a.threads, a.reps, a.warm_ms, scan, fold, emit, host, C.byref(bad),
                                       C.byref(nbytes), C.byref(macs)))
            gb = nbytes.value / 1e9
            mismatches += bad.value if hosts else 0
            leg = {"format": name, "block_samples": block, "ratio_permille": ratio, "tracks": n, "frames": frames, "arena_gb": gb, "scan": stage(scan),
                   "fold": stage(fold), "emit": stage(emit), "multiply_adds": macs.value}
            t = macs.value / 1e12 / (med(scan) / 1e3)
            leg["scan"].update(gb_per_s=gb / (med(scan) / 1e3), fraction_of_hbm_peak=gb / (med(scan) / 1e3) / HBM_PEAK_GB_S, tera_multiply_adds_per_s=t)
            line = (f"{name} B={block} ratio={ratio / 1000:g} {n} x {a.seconds:.0f} s ({gb:.1f} GB): scan {med(scan):.1f} ms ({min(scan):.1f} .. {max(scan):.1f}; "
                    f"{leg['scan']['gb_per_s']:.0f} GB/s, {t:.2f} T multiply-adds/s); fold {med(fold):.2f} ms ({min(fold):.2f} .. {max(fold):.2f}); "
                    f"emit {med(emit):.2f} ms ({min(emit):.2f} .. {max(emit):.2f})")
            if hosts:
                hm = med(host) * n / hosts
                leg.update(host_threads=a.threads, host_tracks_scanned=hosts, host_ms=hm, host_ms_all_unscaled=list(host),
                           kernels_over_host=hm / (med(scan) + med(fold) + med(emit)), host_mismatches=bad.value)
                line += f"; host x{a.threads} {hm:.0f} ms ({leg['kernels_over_host']:.0f} x), {bad.value} mismatches"
            print(line, flush=True)
            legs.append(leg)
        # DR's read floor, same process, an arena of the same shape
        dr_legs = []
        for fmt, name in ((D.FMT_S16_PLANAR, "s16"), (D.FMT_F32_PLANAR, "f32")):
            dr, stats, floor, host = ((C.c_double * a.reps)() for _ in range(4))
            bad, nbytes = C.c_size_t(), C.c_uint64()
            an._check(L.rg_dr_rate(an.handle, n, frames, fmt, 0, a.threads, a.reps, a.warm_ms, dr, stats, floor, host, C.byref(bad), C.byref(nbytes)))
            mine = next(x for x in legs if x["format"] == name and x["block_samples"] == D.CK_DEFAULT_BLOCK)["scan"]
            d = {"format": name, "arena_gb": nbytes.value / 1e9, "read_floor": stage(floor), "scan_over_read_floor": mine["ms"] / med(floor)}
            print(f"{name}: read floor {med(floor):.2f} ms ({min(floor):.2f} .. {max(floor):.2f}): the scan takes {d['scan_over_read_floor']:.1f} times the floor", flush=True)
            dr_legs.append(d)
    result = {"tool": "clicks_rate", "rate": 44100, "channels": 2, "seconds_per_track": a.seconds, "reps": a.reps, "warm_ms": a.warm_ms,
              "hbm_peak_gb_per_s": HBM_PEAK_GB_S, "emit_ratio": a.emit_ratio, "legs": legs, "dr": dr_legs, "mismatches": mismatches}
    print(f"mismatches {mismatches}")
    Path(a.json).parent.mkdir(parents=True, exist_ok=True)
    Path(a.json).write_text(json.dumps(result, indent=1) + "\n")
    if mismatches:
        raise SystemExit(f"{mismatches} host records or event lists differ from the kernels'")


if __name__ == "__main__":
    main()
