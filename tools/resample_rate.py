#!/usr/bin/env python3
"""The rate of the rational resampler (MI355X) and of its host twin: 1000 tracks of three minutes of 16-bit stereo filled on the
device (rg_resample_rate), at 44100 Hz (L = 1: the key scan's decimation kernel at D = 4, 65 taps) and at 48000 Hz (L = 147,
M = 640, 70 taps per output: the resampler's own kernel).

    tools/resample_rate.py [--tracks 1000] [--seconds 180] [--rates 44100,48000] [--host-tracks 16] [--threads 16] [--reps 5]
                           [--warm-ms 400] [--json profiles/resample_rate.json]

Per rate, after a warm-up (the launches repeated for `warm-ms` milliseconds: a fresh process runs slower for a while after a
large allocation), `reps` rounds in which the resampler's launches over all tracks and a read-only pass over the same planes
alternate, HIP events around the launches alone.  The host leg runs the kernel's arithmetic (route 2) on `threads` threads over
the first `host-tracks` tracks, scaled to the track count (tracks are independent and equally long); every resampled sample of
those tracks must equal the kernels'.  Medians and the spread (min .. max) are reported.  The arithmetic is counted as outputs x
taps multiplications and as many additions (they are not fused: the contract), set against the f32 vector peak of 256 CUs x 4
SIMDs x 32 lanes x 2.4 GHz = 78.6 T lane-operations per second; the tap table's loads as outputs x taps words."""
import argparse
import ctypes as C
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

VECTOR_PEAK_TOPS = 256 * 4 * 32 * 2.4e9 / 1e12  # lane-operations per second of the vector ALUs, in T


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tracks", type=int, default=1000)
    ap.add_argument("--seconds", type=float, default=180.0)
    ap.add_argument("--rates", default="44100,48000")
    ap.add_argument("--host-tracks", type=int, default=16)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warm-ms", type=float, default=400.0)
    ap.add_argument("--json", default=str(ROOT / "profiles" / "resample_rate.json"))
    a = ap.parse_args()
    import torch  # noqa: F401  (torch first: one HIP runtime per process)

    import mp3rgain_amd as rg
    from mp3rgain_amd import _capi

    L = _capi.load()
    n, hn = a.tracks, min(a.tracks, a.host_tracks)
    med = statistics.median
    out = {"tool": "resample_rate", "channels": 2, "format": "s16", "tracks": n, "seconds_per_track": a.seconds, "reps": a.reps, "warm_ms": a.warm_ms,
           "vector_peak_tera_lane_ops_per_s": VECTOR_PEAK_TOPS, "rates": {}}
    worst = 0
    with rg.Analyzer(0) as an:
        for rate in [int(r) for r in a.rates.split(",")]:
            frames = int(rate * a.seconds)
            up, down, taps, ok = rg.resample_plan(rate)
            m = rg.resample_count(rate, frames)
            arrays = [(C.c_double * a.reps)() for _ in range(3)]
            bad = C.c_size_t()
            an._check(L.rg_resample_rate(an.handle, n, frames, rate, hn, a.threads, a.reps, a.warm_ms, *arrays, C.byref(bad)))
            rs, read, host = (list(x) for x in arrays)
            ops, gb = 2 * n * m * taps, 4.0 * n * frames / 1e9
            h = med(host) * n / hn if hn else None
            out["rates"][str(rate)] = dict(
                up=up, down=down, taps=taps, frames=frames, resampled_per_track=m, kernel="key decimation" if up == 1 else "resample", ms=med(rs),
                ms_min=min(rs), ms_max=max(rs), ms_all=rs, read_only_ms=med(read), read_only_ms_all=read, read_only_over_resampler=med(read) / med(rs),
                pcm_gb=gb, pcm_gb_per_s=gb / (med(rs) / 1e3), lane_operations=ops, tera_lane_ops_per_s=ops / 1e12 / (med(rs) / 1e3),
                share_of_vector_peak=ops / 1e12 / (med(rs) / 1e3) / VECTOR_PEAK_TOPS, table_bytes=4 * up * taps if up > 1 else 4 * taps,
                table_words_loaded=n * m * taps, table_words_per_s=n * m * taps / (med(rs) / 1e3), host_threads=a.threads, host_tracks=hn, host_ms=h,
                host_ms_all_unscaled=host, kernels_over_host=(h / med(rs)) if hn else None, mismatches=bad.value)
            worst = max(worst, bad.value)
            print(f"{rate} Hz (L = {up}, M = {down}, {taps} taps): {n} x {a.seconds:.0f} s: {med(rs):.2f} ms ({min(rs):.2f} .. {max(rs):.2f}) = "
                  f"{gb / (med(rs) / 1e3):.0f} GB/s of PCM, {ops / 1e12 / (med(rs) / 1e3):.1f} T lane-operations/s = "
                  f"{100 * ops / 1e12 / (med(rs) / 1e3) / VECTOR_PEAK_TOPS:.1f} % of the vector peak; a read-only pass {med(read):.2f} ms = "
                  f"{100 * med(read) / med(rs):.1f} % of it" + (f"; host x{a.threads}: {h:.0f} ms ({h / med(rs):.0f} x); {bad.value} mismatching tracks" if hn else ""),
                  flush=True)
    Path(a.json).parent.mkdir(parents=True, exist_ok=True)
    Path(a.json).write_text(json.dumps(out, indent=1) + "\n")
    if worst:
        raise SystemExit(f"{worst} host signals differ from the kernels'")


if __name__ == "__main__":
    main()
