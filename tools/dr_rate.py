#!/usr/bin/env python3
"""The dynamic range kernels against the PCM stats kernels, a read-only kernel and their own serial host twin (MI355X): 1000
tracks of three minutes of 44.1 kHz 16-bit stereo filled on the device, then the same frames as 32-bit float (rg_dr_rate).

    tools/dr_rate.py [--tracks 1000] [--seconds 180] [--host-tracks 16] [--threads 16] [--reps 7] [--warm-ms 400]
                     [--json profiles/dr_rate.json]

All three legs read every byte of the arena once.  After a warm-up (a fresh process runs slower for a while after a large
allocation: the three legs are launched in turn for `warm-ms` milliseconds first), `reps` rounds alternate, in one process and
over one arena: the DR pieces + fold kernels; the stats tile + fold kernels (the project's fastest PCM scan so far); and a
kernel that only adds up the 16-byte words of the same planes, cut into the DR kernels' pieces with the same loads in flight (the
read floor of this access pattern).  HIP events lie around the launches alone.  The serial host twin runs on `threads` threads
over a host copy of the first `host-tracks` tracks, its time scaled to the count (tracks are independent and equally long).
Medians and the spread (min .. max) are reported, as milliseconds, bytes per second and the share of the 8 TB/s HBM peak, with
the DR kernels' ratio to the stats pair and their share of the read floor.  Every host plane record must equal the kernels'."""
import argparse
import ctypes as C
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

HBM_PEAK_GB_S = 8000.0  # MI355X: 8 TB/s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tracks", type=int, default=1000)
    ap.add_argument("--seconds", type=float, default=180.0)
    ap.add_argument("--host-tracks", type=int, default=16)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warm-ms", type=float, default=400.0)
    ap.add_argument("--json", default=str(ROOT / "profiles" / "dr_rate.json"))
    a = ap.parse_args()
    import torch  # noqa: F401  (torch first: one HIP runtime per process)

    import mp3rgain_amd as rg
    from mp3rgain_amd import _capi

    L = _capi.load()
    n, frames = a.tracks, int(44100 * a.seconds)
    host_n = min(n, a.host_tracks)

    def timing(ms_all, gb):
        ms = statistics.median(ms_all)
        return {"ms": ms, "ms_min": min(ms_all), "ms_max": max(ms_all), "ms_all": list(ms_all), "gb_per_s": gb / (ms / 1e3),
                "gb_per_s_min": gb / (max(ms_all) / 1e3), "gb_per_s_max": gb / (min(ms_all) / 1e3),
                "fraction_of_hbm_peak": gb / (ms / 1e3) / HBM_PEAK_GB_S}

    legs, mismatches = [], 0
    with rg.Analyzer(0) as an:
        for fmt, name in ((_capi.FMT_S16_PLANAR, "s16"), (_capi.FMT_F32_PLANAR, "f32")):
            dr, stats, floor, host = ((C.c_double * a.reps)() for _ in range(4))
            bad, nbytes = C.c_size_t(), C.c_uint64()
            an._check(L.rg_dr_rate(an.handle, n, frames, fmt, host_n, a.threads, a.reps, a.warm_ms, dr, stats, floor, host, C.byref(bad), C.byref(nbytes)))
            gb = nbytes.value / 1e9
            mismatches += bad.value if host_n else 0
            leg = {"format": name, "tracks": n, "frames": frames, "arena_gb": gb, "dr": timing(list(dr), gb), "stats": timing(list(stats), gb),
                   "read_floor": timing(list(floor), gb)}
            leg["dr_over_stats_bytes_per_s"] = leg["dr"]["gb_per_s"] / leg["stats"]["gb_per_s"]
            leg["dr_share_of_read_floor"] = leg["dr"]["gb_per_s"] / leg["read_floor"]["gb_per_s"]
            # outside the run-to-run spread: the slowest DR round against the fastest stats round
            leg["dr_beats_stats_outside_the_spread"] = leg["dr"]["ms_max"] < leg["stats"]["ms_min"]
            if host_n:
                hm = statistics.median(host) * n / host_n
                leg.update(host_threads=a.threads, host_tracks_scanned=host_n, host_ms=hm, host_ms_all_unscaled=list(host), host_gb_per_s=gb / (hm / 1e3),
                           host_mismatches=bad.value)
            line = f"{name} {n} x {a.seconds:.0f} s ({gb:.1f} GB):"
            for key in ("dr", "stats", "read_floor"):
                s = leg[key]
                line += (f" {key} {s['ms']:.3f} ms ({s['ms_min']:.3f} .. {s['ms_max']:.3f}; {s['gb_per_s']:.0f} GB/s = "
                         f"{100 * s['fraction_of_hbm_peak']:.1f} % of the 8 TB/s HBM peak);")
            line += f" dr / stats {leg['dr_over_stats_bytes_per_s']:.2f}, dr / floor {leg['dr_share_of_read_floor']:.2f}"
            if host_n:
                line += f"; host x{a.threads} {leg['host_ms']:.0f} ms ({leg['host_gb_per_s']:.2f} GB/s), {bad.value} mismatches"
            print(line, flush=True)
            legs.append(leg)
    result = {"tool": "dr_rate", "rate": 44100, "channels": 2, "seconds_per_track": a.seconds, "reps": a.reps, "warm_ms": a.warm_ms,
              "hbm_peak_gb_per_s": HBM_PEAK_GB_S, "legs": legs, "mismatches": mismatches}
    print(f"mismatches {mismatches}")
    Path(a.json).parent.mkdir(parents=True, exist_ok=True)
    Path(a.json).write_text(json.dumps(result, indent=1) + "\n")
    if mismatches:
        raise SystemExit(f"{mismatches} host records differ from the kernels'")


if __name__ == "__main__":
    main()
