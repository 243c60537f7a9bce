#!/usr/bin/env python3
"""The PCM stats kernels against the rip checksum kernels and their own serial host twin (MI355X): BASELINE configs[2]-sized data,
1000 tracks of three minutes of 44.1 kHz 16-bit stereo filled on the device (rg_pcm_stats_rate).

    tools/pcm_stats_rate.py [--tracks 1000] [--seconds 180] [--host-tracks 16] [--threads 16] [--reps 7] [--warm-ms 400]
                            [--json profiles/pcm_stats_rate.json]

Both pairs of kernels read every byte of the arena once, so the yardstick is the rip tile + fold pair in the same process: after
a warm-up (a fresh process runs slower for a while after a large allocation: the stats kernels are launched for `warm-ms`
milliseconds first), `reps` rounds alternate the stats tile + fold kernels (HIP events around the launches) with the rip tile +
fold kernels over the same arena, and with the serial host twin on `threads` threads over a host copy of the first
`host-tracks` tracks, whose time is scaled to the count (tracks are independent and equally long).  Medians and the spread
(min .. max) are reported, as milliseconds, bytes per second and the share of the 8 TB/s HBM peak.  Both forms of a lane's walk
are timed: with the any-test over four samples in front of the stretch bookkeeping, and without.  A 32-bit float leg of the same
frame count follows (twice the bytes; no rip kernels: they take 16-bit PCM).  Every host record must equal the kernels'."""
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
    ap.add_argument("--json", default=str(ROOT / "profiles" / "pcm_stats_rate.json"))
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
        for fmt, name, bps, with_rip in ((_capi.FMT_S16_PLANAR, "s16", 2, True), (_capi.FMT_F32_PLANAR, "f32", 4, False)):
            gb = n * frames * 2 * bps / 1e9
            leg = {"format": name, "tracks": n, "frames": frames, "arena_gb": gb}
            for any_test in (1, 0):
                stats = (C.c_double * a.reps)()
                rip = (C.c_double * a.reps)() if with_rip else None
                host = (C.c_double * a.reps)()
                bad = C.c_size_t()
                hn = host_n if any_test else 0  # the host twin does not depend on the form of the device's walk
                an._check(L.rg_pcm_stats_rate(an.handle, n, frames, fmt, any_test, hn, a.threads, a.reps, a.warm_ms, stats, rip, host, C.byref(bad)))
                mismatches += bad.value if hn else 0
                key = "any_test" if any_test else "plain_walk"
                leg[key] = {"stats": timing(list(stats), gb)}
                if with_rip:
                    leg[key]["rip"] = timing(list(rip), gb)
                    leg[key]["stats_over_rip_bytes_per_s"] = leg[key]["stats"]["gb_per_s"] / leg[key]["rip"]["gb_per_s"]
                if hn:
                    hm = statistics.median(host) * n / hn
                    leg.update(host_threads=a.threads, host_tracks_scanned=hn, host_ms=hm, host_ms_all_unscaled=list(host), host_gb_per_s=gb / (hm / 1e3),
                               host_mismatches=bad.value)
                s = leg[key]["stats"]
                line = (f"{name} {n} x {a.seconds:.0f} s ({gb:.1f} GB), {key}: stats {s['ms']:.3f} ms ({s['ms_min']:.3f} .. {s['ms_max']:.3f}; "
                        f"{s['gb_per_s']:.0f} GB/s = {100 * s['fraction_of_hbm_peak']:.1f} % of the 8 TB/s HBM peak)")
                if with_rip:
                    r = leg[key]["rip"]
                    line += f", rip {r['ms']:.3f} ms ({r['ms_min']:.3f} .. {r['ms_max']:.3f}; {r['gb_per_s']:.0f} GB/s)"
                if hn:
                    line += f", host x{a.threads} {leg['host_ms']:.0f} ms ({leg['host_gb_per_s']:.2f} GB/s), {bad.value} mismatches"
                print(line, flush=True)
            leg["faster_walk"] = "any_test" if leg["any_test"]["stats"]["ms"] < leg["plain_walk"]["stats"]["ms"] else "plain_walk"
            legs.append(leg)
    s16 = legs[0]
    product = "any_test"  # RG_STATS_ANY_TEST of rg_stats.h
    # outside the run-to-run spread: the slowest stats round against the fastest rip round
    ahead = s16[product]["stats"]["gb_per_s_min"] >= s16[product]["rip"]["gb_per_s_max"]
    result = {"tool": "pcm_stats_rate", "rate": 44100, "channels": 2, "seconds_per_track": a.seconds, "reps": a.reps, "warm_ms": a.warm_ms,
              "hbm_peak_gb_per_s": HBM_PEAK_GB_S, "legs": legs, "product_walk": product, "mismatches": mismatches,
              "stats_reach_rip_bytes_per_s_outside_the_spread": ahead}
    print(f"mismatches {mismatches}; stats at least the rip kernels' bytes/s outside the spread: {ahead}")
    Path(a.json).parent.mkdir(parents=True, exist_ok=True)
    Path(a.json).write_text(json.dumps(result, indent=1) + "\n")
    if mismatches:
        raise SystemExit(f"{mismatches} host records differ from the kernels'")


if __name__ == "__main__":
    main()
