#!/usr/bin/env python3
"""The ancestry kernels' rate (MI355X) and their serial host twin's: 1000 tracks of three minutes of 44.1 kHz 16-bit stereo
filled on the device (rg_ancestry_rate).

    tools/ancestry_rate.py [--tracks 1000] [--seconds 180] [--whole-tracks 20] [--host-tracks 4] [--threads 16] [--reps 5]
                           [--warm-ms 400] [--json profiles/ancestry_rate.json]

Three legs.  `defaults`: every track at the default options (16 segments of 32 granules, 4 views of a stereo track).  `whole`:
`whole-tracks` tracks with segments = 0, every granule of the file.  After a warm-up (the launch repeated for `warm-ms`
milliseconds: a fresh process runs slower for a while after a large allocation), `reps` timed launches, HIP events around the
launches alone.  `host`: the serial host twin on `threads` threads over a host copy of the first `host-tracks` tracks at the
defaults, its time scaled to the count (tracks are independent and equally long); every one of its counts must equal the
kernels'.  Medians and the spread (min .. max) are reported, with the fused multiply-adds per sample of a view, counted from the
tile structure (rg_anc_fma_per_sample: slots x (512 + 2048) and (alignment, granule) pairs x (32 x 648 + 496 + 576) per
workgroup), the rate they make and its share of the 157.3 TFLOP/s (78.65 T fused multiply-adds per second) f32 vector peak."""
import argparse
import ctypes as C
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

VECTOR_PEAK_TFMA_S = 157.3 / 2.0  # MI355X: 157.3 TFLOP/s of f32 on the vector pipe, two operations per fused multiply-add


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tracks", type=int, default=1000)
    ap.add_argument("--seconds", type=float, default=180.0)
    ap.add_argument("--whole-tracks", type=int, default=20)
    ap.add_argument("--host-tracks", type=int, default=4)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warm-ms", type=float, default=400.0)
    ap.add_argument("--json", default=str(ROOT / "profiles" / "ancestry_rate.json"))
    a = ap.parse_args()
    import torch  # noqa: F401  (torch first: one HIP runtime per process)

    import mp3rgain_amd as rg
    from mp3rgain_amd import _capi

    L = _capi.load()
    frames = int(44100 * a.seconds)

    def leg(an, name, n, opts, host_n):
        ms, host = (C.c_double * a.reps)(), (C.c_double * a.reps)()
        bad, fma = C.c_size_t(), C.c_double()
        an._check(L.rg_ancestry_rate(an.handle, n, frames, C.byref(opts) if opts is not None else None, host_n, a.threads, a.reps, a.warm_ms, ms, host,
                                     C.byref(bad), C.byref(fma)))
        ms = list(ms)
        med = statistics.median(ms)
        samples = 4.0 * n * frames  # samples of all views: 2 channels, mid and side
        tfma = fma.value * samples / 1e12
        out = {"leg": name, "tracks": n, "frames": frames, "views": 4 * n, "ms": med, "ms_min": min(ms), "ms_max": max(ms), "ms_all": ms,
               "fma_per_view_sample": fma.value, "tera_fma": tfma, "tera_fma_per_s": tfma / (med / 1e3),
               "share_of_f32_vector_peak": tfma / (med / 1e3) / VECTOR_PEAK_TFMA_S, "tracks_per_s": n / (med / 1e3),
               "audio_seconds_per_s": n * a.seconds / (med / 1e3)}
        line = (f"{name}: {n} x {a.seconds:.0f} s: {med:.1f} ms ({min(ms):.1f} .. {max(ms):.1f}); {fma.value:.0f} FMA per sample of a view, "
                f"{out['tera_fma_per_s']:.1f} TFMA/s = {100 * out['share_of_f32_vector_peak']:.1f} % of the f32 vector peak; {out['tracks_per_s']:.0f} tracks/s")
        if host_n:
            hm = statistics.median(host) * n / host_n
            out.update(host_threads=a.threads, host_tracks_scanned=host_n, host_ms=hm, host_ms_all_unscaled=list(host), host_mismatches=bad.value,
                       kernels_over_host=hm / med)
            line += f"; host x{a.threads} {hm:.0f} ms ({hm / med:.0f} x), {bad.value} mismatching views"
        print(line, flush=True)
        return out, (bad.value if host_n else 0)

    with rg.Analyzer(0) as an:
        d, bad = leg(an, "defaults", a.tracks, None, min(a.tracks, a.host_tracks))
        whole = _capi.AncestryOpts(0, 1, 0.0, 0.0, 0.0, 0)
        w, _ = leg(an, "whole", min(a.tracks, a.whole_tracks), whole, 0)
    result = {"tool": "ancestry_rate", "rate": 44100, "channels": 2, "seconds_per_track": a.seconds, "reps": a.reps, "warm_ms": a.warm_ms,
              "f32_vector_peak_tera_fma_per_s": VECTOR_PEAK_TFMA_S, "legs": [d, w], "mismatches": bad}
    print(f"mismatches {bad}")
    Path(a.json).parent.mkdir(parents=True, exist_ok=True)
    Path(a.json).write_text(json.dumps(result, indent=1) + "\n")
    if bad:
        raise SystemExit(f"{bad} host views differ from the kernels'")


if __name__ == "__main__":
    main()
