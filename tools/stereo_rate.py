#!/usr/bin/env python3
"""The rates of the stereo scan's kernels (MI355X) and of their serial host twin: 1000 tracks of three minutes of 44.1 kHz 16-bit
stereo filled on the device, then the same frames as 32-bit float (rg_stereo_rate), beside the DR pair and its read floor
(rg_dr_rate) and the tempo scan's window kernel (rg_tempo_rate) run by the same process.

    tools/stereo_rate.py [--tracks 1000] [--seconds 180] [--host-tracks 16] [--threads 16] [--reps 5] [--warm-ms 400]
                         [--json profiles/stereo_rate.json]

Per call of a hook: after a warm-up (the legs launched in turn for `warm-ms` milliseconds), `reps` rounds alternate over one
arena, HIP events around the launches alone; medians and the spread (min .. max) are reported.
  1. moments + fold, as bytes per second, beside the DR pieces + fold pair and DR's read-floor kernel over an arena of the same
     shape (each hook fills its own: the three legs do not share rounds, only the process);
  2. the lag kernel at radius 64 and radius 8, as multiply-adds of the definition per second and as a share of the FP64 vector
     FMA peak (39.3 T fused multiply-adds per second: 256 CUs x 4 SIMDs x 16 lanes at 2.4 GHz), beside the tempo scan's window
     kernel (integer multiply-adds) in the same process;
  3. the serial host twin on `threads` threads over a host copy of the first `host-tracks` tracks, its time scaled to the count.
     Every host record and lag sum must equal the kernels'."""
import argparse
import ctypes as C
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

HBM_PEAK_GB_S = 8000.0      # MI355X: 8 TB/s
FP64_FMA_PEAK_T = 39.3      # T fused multiply-adds per second on the vector pipe (78.6 TFLOP/s)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tracks", type=int, default=1000)
    ap.add_argument("--seconds", type=float, default=180.0)
    ap.add_argument("--host-tracks", type=int, default=16)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warm-ms", type=float, default=400.0)
    ap.add_argument("--json", default=str(ROOT / "profiles" / "stereo_rate.json"))
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
    with rg.Analyzer(0) as an:
        for fmt, name, radius, hosts in ((_capi.FMT_S16_PLANAR, "s16", 64, host_n), (_capi.FMT_S16_PLANAR, "s16", 8, 0), (_capi.FMT_F32_PLANAR, "f32", 64, host_n)):
            mom, lag, host = ((C.c_double * a.reps)() for _ in range(3))
            bad, nbytes, macs = C.c_size_t(), C.c_uint64(), C.c_uint64()
            an._check(L.rg_stereo_rate(an.handle, n, frames, fmt, radius, hosts, a.threads, a.reps, a.warm_ms, mom, lag, host, C.byref(bad), C.byref(nbytes),
                                       C.byref(macs)))
            gb = nbytes.value / 1e9
            mismatches += bad.value if hosts else 0
            leg = {"format": name, "radius": radius, "tracks": n, "frames": frames, "arena_gb": gb, "moments_and_fold": stage(mom), "lags": stage(lag),
                   "multiply_adds": macs.value}
            leg["moments_and_fold"].update(gb_per_s=gb / (med(mom) / 1e3), fraction_of_hbm_peak=gb / (med(mom) / 1e3) / HBM_PEAK_GB_S)
            t = macs.value / 1e12 / (med(lag) / 1e3)
            leg["lags"].update(tera_multiply_adds_per_s=t, fp64_fma_peak_tera_per_s=FP64_FMA_PEAK_T, share_of_fp64_fma_peak=t / FP64_FMA_PEAK_T)
            line = (f"{name} R={radius} {n} x {a.seconds:.0f} s ({gb:.1f} GB): moments + fold {med(mom):.2f} ms ({min(mom):.2f} .. {max(mom):.2f}; "
                    f"{leg['moments_and_fold']['gb_per_s']:.0f} GB/s); lags {med(lag):.1f} ms ({min(lag):.1f} .. {max(lag):.1f}); {t:.2f} T multiply-adds/s = "
                    f"{100 * t / FP64_FMA_PEAK_T:.1f} % of the FP64 vector FMA peak")
            if hosts:
                hm = med(host) * n / hosts
                leg.update(host_threads=a.threads, host_tracks_scanned=hosts, host_ms=hm, host_ms_all_unscaled=list(host),
                           kernels_over_host=hm / (med(mom) + med(lag)), host_mismatches=bad.value)
                line += f"; host x{a.threads} {hm:.0f} ms ({leg['kernels_over_host']:.0f} x), {bad.value} mismatches"
            print(line, flush=True)
            legs.append(leg)
        # the DR pair and its read floor, same process, an arena of the same shape
        dr_legs = []
        for fmt, name in ((_capi.FMT_S16_PLANAR, "s16"), (_capi.FMT_F32_PLANAR, "f32")):
            dr, stats, floor, host = ((C.c_double * a.reps)() for _ in range(4))
            bad, nbytes = C.c_size_t(), C.c_uint64()
            an._check(L.rg_dr_rate(an.handle, n, frames, fmt, 0, a.threads, a.reps, a.warm_ms, dr, stats, floor, host, C.byref(bad), C.byref(nbytes)))
            gb = nbytes.value / 1e9
            d = {"format": name, "arena_gb": gb, "dr_pair": stage(dr), "read_floor": stage(floor)}
            mine = next(x for x in legs if x["format"] == name and x["radius"] == 64)["moments_and_fold"]
            d.update(dr_share_of_read_floor=med(floor) / med(dr), moments_share_of_read_floor=med(floor) / mine["ms"], moments_over_dr_ms=mine["ms"] / med(dr))
            print(f"{name}: DR pieces + fold {med(dr):.2f} ms ({min(dr):.2f} .. {max(dr):.2f}), read floor {med(floor):.2f} ms ({min(floor):.2f} .. {max(floor):.2f}): "
                  f"the DR pair runs at {100 * d['dr_share_of_read_floor']:.0f} % of the floor, moments + fold at {100 * d['moments_share_of_read_floor']:.0f} %", flush=True)
            dr_legs.append(d)
        # the tempo scan's window kernel, same process
        arrays = [(C.c_double * a.reps)() for _ in range(6)]
        bad = C.c_size_t()
        an._check(L.rg_tempo_rate(an.handle, n, frames, None, 0, a.threads, a.reps, a.warm_ms, *arrays, C.byref(bad)))
    acf = list(arrays[2])
    W, hop = _capi.TEMPO_WINDOW, _capi.TEMPO_WINDOW_HOP
    k = rg.fingerprint_codes(frames)
    windows = (k - 2 * W) // hop + 1 if k >= 2 * W else 0
    acf_macs = n * windows * W * W
    acf_t = acf_macs / 1e12 / (med(acf) / 1e3)
    tempo = dict(stage(acf), multiply_adds=acf_macs, tera_multiply_adds_per_s=acf_t)
    best = next(x for x in legs if x["format"] == "s16" and x["radius"] == 64)["lags"]["tera_multiply_adds_per_s"]
    print(f"tempo window kernel: {med(acf):.2f} ms ({min(acf):.2f} .. {max(acf):.2f}); {acf_t:.2f} T multiply-adds/s; the lag kernel at R = 64 runs at "
          f"{best / acf_t:.2f} of that per multiply-add", flush=True)
    result = {"tool": "stereo_rate", "rate": 44100, "channels": 2, "seconds_per_track": a.seconds, "reps": a.reps, "warm_ms": a.warm_ms,
              "hbm_peak_gb_per_s": HBM_PEAK_GB_S, "legs": legs, "dr": dr_legs, "tempo_window_kernel": tempo, "lags_over_tempo_per_multiply_add": best / acf_t,
              "mismatches": mismatches}
    print(f"mismatches {mismatches}")
    Path(a.json).parent.mkdir(parents=True, exist_ok=True)
    Path(a.json).write_text(json.dumps(result, indent=1) + "\n")
    if mismatches:
        raise SystemExit(f"{mismatches} host records or lag sums differ from the kernels'")


if __name__ == "__main__":
    main()
