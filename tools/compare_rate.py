#!/usr/bin/env python3
"""The rates of the null test's kernels (MI355X) and of their serial host twin: 500 pairs out of 1000 tracks of three minutes of
44.1 kHz 16-bit stereo filled on the device, then the same frames as 32-bit float (rg_compare_rate), beside the stereo scan's
moments pair and lag kernel at radius 64 (rg_stereo_rate) and DR's read floor (rg_dr_rate) run by the same process.

    tools/compare_rate.py [--tracks 1000] [--seconds 180] [--host-pairs 16] [--threads 16] [--reps 5] [--warm-ms 400]
                          [--json profiles/compare_rate.json]

Per call of a hook: after a warm-up (the legs launched in turn for `warm-ms` milliseconds), `reps` rounds alternate over one
arena, HIP events around the launches alone; medians and the spread (min .. max) are reported.
  1. moments + fold over every pair's overlap, as bytes per second, beside the stereo scan's moments pair and DR's read-floor
     kernel over an arena of the same shape (each hook fills its own: the legs do not share rounds, only the process);
  2. the lag kernel at the defaults (radius 1024, 4 segments of 262144 frames) and at radius 64, as multiply-adds of the definition
     per second and as a share of the FP64 vector FMA peak (39.3 T fused multiply-adds per second), beside the stereo scan's lag
     kernel at radius 64 in the same process;
  3. the serial host twin on `threads` threads over a host copy of the first `host-pairs` pairs, its time scaled to the count.
     Every host pair's lag rows, lag, polarity, block rows and totals must equal the kernels': `mismatches` must be 0, the one hard
     condition of this tool."""
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
    ap.add_argument("--host-pairs", type=int, default=16)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warm-ms", type=float, default=400.0)
    ap.add_argument("--json", default=str(ROOT / "profiles" / "compare_rate.json"))
    a = ap.parse_args()
    import torch  # noqa: F401  (torch first: one HIP runtime per process)

    import mp3rgain_amd as rg
    from mp3rgain_amd import _capi
    from mp3rgain_amd.replaygain import _compare_opts

    L = _capi.load()
    n, frames = a.tracks, int(44100 * a.seconds)
    pairs = n // 2
    host_n = min(pairs, a.host_pairs)
    med = statistics.median
    stage = lambda x: {"ms": med(x), "ms_min": min(x), "ms_max": max(x), "ms_all": list(x)}  # noqa: E731
    legs, mismatches = [], 0
    with rg.Analyzer(0) as an:
        for fmt, name, radius, hosts in ((_capi.FMT_S16_PLANAR, "s16", 1024, host_n), (_capi.FMT_S16_PLANAR, "s16", 64, 0),
                                         (_capi.FMT_F32_PLANAR, "f32", 1024, 0), (_capi.FMT_F32_PLANAR, "f32", 64, host_n)):
            mom, lag, host = ((C.c_double * a.reps)() for _ in range(3))
            bad, nbytes, macs = C.c_size_t(), C.c_uint64(), C.c_uint64()
            o, _ = _compare_opts(radius=radius, align=_capi.CMP_ALIGN_HINT)
            an._check(L.rg_compare_rate(an.handle, n, pairs, frames, fmt, C.byref(o), hosts, a.threads, a.reps, a.warm_ms, mom, lag, host, C.byref(bad),
                                        C.byref(nbytes), C.byref(macs)))
            gb = nbytes.value / 1e9
            mismatches += bad.value if hosts else 0
            leg = {"format": name, "radius": radius, "segments": o.segments, "segment_frames": o.segment_frames, "tracks": n, "pairs": pairs, "frames": frames,
                   "arena_gb": gb, "moments_and_fold": stage(mom), "lags": stage(lag), "multiply_adds": macs.value}
            leg["moments_and_fold"].update(gb_per_s=gb / (med(mom) / 1e3), fraction_of_hbm_peak=gb / (med(mom) / 1e3) / HBM_PEAK_GB_S)
            t = macs.value / 1e12 / (med(lag) / 1e3)
            leg["lags"].update(tera_multiply_adds_per_s=t, fp64_fma_peak_tera_per_s=FP64_FMA_PEAK_T, share_of_fp64_fma_peak=t / FP64_FMA_PEAK_T)
            line = (f"{name} R={radius} {pairs} pairs of {a.seconds:.0f} s ({gb:.1f} GB): moments + fold {med(mom):.2f} ms ({min(mom):.2f} .. {max(mom):.2f}; "
                    f"{leg['moments_and_fold']['gb_per_s']:.0f} GB/s); lags {med(lag):.1f} ms ({min(lag):.1f} .. {max(lag):.1f}); {t:.2f} T multiply-adds/s = "
                    f"{100 * t / FP64_FMA_PEAK_T:.1f} % of the FP64 vector FMA peak")
            if hosts:
                hm = med(host) * pairs / hosts
                leg.update(host_threads=a.threads, host_pairs_scanned=hosts, host_ms=hm, host_ms_all_unscaled=list(host),
                           host_over_kernels=hm / (med(mom) + med(lag)), host_mismatches=bad.value)
                line += f"; host x{a.threads} {hm:.0f} ms ({leg['host_over_kernels']:.0f} x), {bad.value} mismatches"
            print(line, flush=True)
            legs.append(leg)
        # the stereo scan's moments pair and lag kernel at radius 64, same process, an arena of the same shape
        st_legs = []
        for fmt, name in ((_capi.FMT_S16_PLANAR, "s16"), (_capi.FMT_F32_PLANAR, "f32")):
            mom, lag, host = ((C.c_double * a.reps)() for _ in range(3))
            bad, nbytes, macs = C.c_size_t(), C.c_uint64(), C.c_uint64()
            an._check(L.rg_stereo_rate(an.handle, n, frames, fmt, 64, 0, a.threads, a.reps, a.warm_ms, mom, lag, host, C.byref(bad), C.byref(nbytes), C.byref(macs)))
            gb = nbytes.value / 1e9
            t = macs.value / 1e12 / (med(lag) / 1e3)
            st_legs.append({"format": name, "radius": 64, "arena_gb": gb, "moments_and_fold": dict(stage(mom), gb_per_s=gb / (med(mom) / 1e3)),
                            "lags": dict(stage(lag), tera_multiply_adds_per_s=t), "multiply_adds": macs.value})
            print(f"stereo {name} R=64: moments + fold {med(mom):.2f} ms ({gb / (med(mom) / 1e3):.0f} GB/s); lags {med(lag):.1f} ms, {t:.2f} T multiply-adds/s", flush=True)
        # DR's read floor, same process
        floors = []
        for fmt, name in ((_capi.FMT_S16_PLANAR, "s16"), (_capi.FMT_F32_PLANAR, "f32")):
            dr, stats, floor, host = ((C.c_double * a.reps)() for _ in range(4))
            bad, nbytes = C.c_size_t(), C.c_uint64()
            an._check(L.rg_dr_rate(an.handle, n, frames, fmt, 0, a.threads, a.reps, a.warm_ms, dr, stats, floor, host, C.byref(bad), C.byref(nbytes)))
            gb = nbytes.value / 1e9
            mine = next(x for x in legs if x["format"] == name and x["radius"] == 1024)["moments_and_fold"]
            st = next(x for x in st_legs if x["format"] == name)["moments_and_fold"]
            d = {"format": name, "arena_gb": gb, "read_floor": dict(stage(floor), gb_per_s=gb / (med(floor) / 1e3))}
            d.update(moments_share_of_read_floor=mine["gb_per_s"] / d["read_floor"]["gb_per_s"], stereo_moments_share_of_read_floor=st["gb_per_s"] / d["read_floor"]["gb_per_s"])
            print(f"{name}: read floor {med(floor):.2f} ms ({d['read_floor']['gb_per_s']:.0f} GB/s): moments + fold at {100 * d['moments_share_of_read_floor']:.0f} % of it, "
                  f"the stereo pair at {100 * d['stereo_moments_share_of_read_floor']:.0f} %", flush=True)
            floors.append(d)
    ratios = {}
    for name in ("s16", "f32"):
        st = next(x for x in st_legs if x["format"] == name)["lags"]["tera_multiply_adds_per_s"]
        for radius in (1024, 64):
            mine = next(x for x in legs if x["format"] == name and x["radius"] == radius)["lags"]["tera_multiply_adds_per_s"]
            ratios[f"{name}_r{radius}_over_stereo_r64"] = mine / st
    print("lag kernel over the stereo lag kernel at radius 64, per multiply-add:", {k: round(v, 3) for k, v in ratios.items()})
    result = {"tool": "compare_rate", "rate": 44100, "channels": 2, "seconds_per_track": a.seconds, "reps": a.reps, "warm_ms": a.warm_ms,
              "hbm_peak_gb_per_s": HBM_PEAK_GB_S, "legs": legs, "stereo": st_legs, "read_floor": floors, "lags_over_stereo_lags": ratios, "mismatches": mismatches}
    print(f"mismatches {mismatches}")
    Path(a.json).parent.mkdir(parents=True, exist_ok=True)
    Path(a.json).write_text(json.dumps(result, indent=1) + "\n")
    if mismatches:
        raise SystemExit(f"{mismatches} host pairs differ from the kernels'")


if __name__ == "__main__":
    main()
