#!/usr/bin/env python3
"""The rates of the tempo scan's stages (MI355X) and of their host twins: 1000 tracks of three minutes of 44.1 kHz 16-bit stereo
filled on the device (rg_tempo_rate).

    tools/tempo_rate.py [--tracks 1000] [--seconds 180] [--host-tracks 16] [--threads 16] [--reps 5] [--warm-ms 400]
                        [--json profiles/tempo_rate.json]

After a warm-up (the launches repeated for `warm-ms` milliseconds: a fresh process runs slower for a while after a large
allocation), `reps` rounds in which the four launches alternate, HIP events around the launches alone: the onset kernels over
all tracks, a read-only pass over the same planes, the window kernel (with the clearing of the sums C) and the finish kernel at
the default options.  The host legs run on `threads` threads over the first `host-tracks` tracks: the kernels' arithmetic (route
2) and the serial stage 2, scaled to the track count (tracks are independent and equally long); every onset and every finish
record of those tracks must equal the kernels'.  Medians and the spread (min .. max) are reported.  The window kernel's work
is counted in multiply-adds of R_w: tracks x windows x W x W; its rate is set against the integer vector peak of 256 CUs x 4
SIMDs x 32 lanes x 2.4 GHz = 78.6 T lane-operations per second, one of which a multiply-add needs at the least."""
import argparse
import ctypes as C
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

INT_PEAK_TOPS = 256 * 4 * 32 * 2.4e9 / 1e12  # lane-operations per second of the vector ALUs, in T


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tracks", type=int, default=1000)
    ap.add_argument("--seconds", type=float, default=180.0)
    ap.add_argument("--host-tracks", type=int, default=16)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warm-ms", type=float, default=400.0)
    ap.add_argument("--json", default=str(ROOT / "profiles" / "tempo_rate.json"))
    a = ap.parse_args()
    import torch  # noqa: F401  (torch first: one HIP runtime per process)

    import mp3rgain_amd as rg
    from mp3rgain_amd import _capi

    L = _capi.load()
    frames = int(44100 * a.seconds)
    n, hn = a.tracks, min(a.tracks, a.host_tracks)
    arrays = [(C.c_double * a.reps)() for _ in range(6)]
    bad = C.c_size_t()
    with rg.Analyzer(0) as an:
        an._check(L.rg_tempo_rate(an.handle, n, frames, None, hn, a.threads, a.reps, a.warm_ms, *arrays, C.byref(bad)))
    onset, read, acf, finish, host_onset, host_finish = (list(x) for x in arrays)
    med = statistics.median
    W, hop = _capi.TEMPO_WINDOW, _capi.TEMPO_WINDOW_HOP
    k = rg.fingerprint_codes(frames)
    windows = (k - 2 * W) // hop + 1 if k >= 2 * W else 0
    macs = n * windows * W * W
    stage = lambda x: {"ms": med(x), "ms_min": min(x), "ms_max": max(x), "ms_all": x}  # noqa: E731
    out = {"tool": "tempo_rate", "rate": 44100, "channels": 2, "format": "s16", "tracks": n, "seconds_per_track": a.seconds, "frames": frames,
           "onsets_per_track": k, "windows_per_track": windows, "reps": a.reps, "warm_ms": a.warm_ms, "mismatches": bad.value,
           "onsets": dict(stage(onset), read_only_ms=med(read), read_only_ms_all=read, read_only_over_onsets=med(read) / med(onset),
                          pcm_gb_per_s=4.0 * n * frames / 1e9 / (med(onset) / 1e3), audio_seconds_per_s=n * a.seconds / (med(onset) / 1e3)),
           "windows": dict(stage(acf), multiply_adds=macs, tera_multiply_adds_per_s=macs / 1e12 / (med(acf) / 1e3),
                           int_peak_tera_lane_ops_per_s=INT_PEAK_TOPS, share_of_int_peak=macs / 1e12 / (med(acf) / 1e3) / INT_PEAK_TOPS),
           "finish": stage(finish), "all_stages_ms": med(onset) + med(acf) + med(finish),
           "audio_seconds_per_s": n * a.seconds / ((med(onset) + med(acf) + med(finish)) / 1e3)}
    line = (f"onsets: {n} x {a.seconds:.0f} s: {med(onset):.1f} ms ({min(onset):.1f} .. {max(onset):.1f}); a read-only pass {med(read):.1f} ms = "
            f"{100 * med(read) / med(onset):.1f} % of it\nwindows: {n * windows} of {W} onsets: {med(acf):.1f} ms ({min(acf):.1f} .. {max(acf):.1f}); "
            f"{out['windows']['tera_multiply_adds_per_s']:.2f} T multiply-adds/s = {100 * out['windows']['share_of_int_peak']:.1f} % of the integer vector peak\n"
            f"finish: {med(finish):.2f} ms ({min(finish):.2f} .. {max(finish):.2f})")
    if hn:
        ho, hf = med(host_onset) * n / hn, med(host_finish) * n / hn
        out["onsets"].update(host_threads=a.threads, host_tracks=hn, host_ms=ho, host_ms_all_unscaled=host_onset, kernels_over_host=ho / med(onset))
        out["host_stage2"] = dict(host_threads=a.threads, host_tracks=hn, host_ms=hf, host_ms_all_unscaled=host_finish,
                                  kernels_over_host=hf / (med(acf) + med(finish)))
        line += (f"\nhost x{a.threads}: onsets {ho:.0f} ms ({ho / med(onset):.0f} x), stage 2 {hf:.0f} ms ({hf / (med(acf) + med(finish)):.0f} x); "
                 f"{bad.value} mismatching onsets or records")
    print(line, flush=True)
    Path(a.json).parent.mkdir(parents=True, exist_ok=True)
    Path(a.json).write_text(json.dumps(out, indent=1) + "\n")
    if bad.value:
        raise SystemExit(f"{bad.value} host onsets or finish records differ from the kernels'")


if __name__ == "__main__":
    main()
