#!/usr/bin/env python3
"""The rates of the key scan's stages (MI355X) and of their host twins: 1000 tracks of three minutes of 44.1 kHz 16-bit stereo
filled on the device (rg_key_rate).

    tools/key_rate.py [--tracks 1000] [--seconds 180] [--host-tracks 16] [--threads 16] [--reps 5] [--warm-ms 400]
                      [--json profiles/key_rate.json]

After a warm-up (the launches repeated for `warm-ms` milliseconds: a fresh process runs slower for a while after a large
allocation), `reps` rounds in which the four launches alternate, HIP events around the launches alone: the decimation kernel
over all tracks (D = 8: 129 taps per output), a read-only pass over the same planes, the tiles kernel over the decimated signals
and the finish kernel at the default options.  The host legs run on `threads` threads over the first `host-tracks` tracks: the
kernels' arithmetic (route 2) and the serial stage 2, scaled to the track count (tracks are independent and equally long); every
decimated sample, every row and every finish record of those tracks must equal the kernels'.  Medians and the spread
(min .. max) are reported.  The decimation's arithmetic is counted as outputs x taps multiplications and as many additions (they
are not fused: the contract), set against the f32 vector peak of 256 CUs x 4 SIMDs x 32 lanes x 2.4 GHz = 78.6 T lane-operations
per second."""
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
    ap.add_argument("--host-tracks", type=int, default=16)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warm-ms", type=float, default=400.0)
    ap.add_argument("--json", default=str(ROOT / "profiles" / "key_rate.json"))
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
        an._check(L.rg_key_rate(an.handle, n, frames, None, hn, a.threads, a.reps, a.warm_ms, *arrays, C.byref(bad)))
    decim, read, tiles, finish, host_stage1, host_finish = (list(x) for x in arrays)
    med = statistics.median
    D = 44100 // _capi.KEY_TARGET_RATE
    taps = _capi.KEY_TAPS_PER_DECIM * D + 1
    M = (frames - taps) // D + 1 if frames >= taps else 0
    F = (M - _capi.KEY_FRAME) // _capi.KEY_HOP + 1 if M >= _capi.KEY_FRAME else 0
    ops = 2 * n * M * taps
    gb = 4.0 * n * frames / 1e9
    stage = lambda x: {"ms": med(x), "ms_min": min(x), "ms_max": max(x), "ms_all": x}  # noqa: E731
    out = {"tool": "key_rate", "rate": 44100, "channels": 2, "format": "s16", "tracks": n, "seconds_per_track": a.seconds, "frames": frames, "decim": D,
           "taps": taps, "decimated_per_track": M, "rows_per_track": F, "reps": a.reps, "warm_ms": a.warm_ms, "mismatches": bad.value,
           "decimation": dict(stage(decim), read_only_ms=med(read), read_only_ms_all=read, read_only_over_decimation=med(read) / med(decim), pcm_gb=gb,
                              pcm_gb_per_s=gb / (med(decim) / 1e3), read_only_gb_per_s=gb / (med(read) / 1e3), lane_operations=ops,
                              tera_lane_ops_per_s=ops / 1e12 / (med(decim) / 1e3), vector_peak_tera_lane_ops_per_s=VECTOR_PEAK_TOPS,
                              share_of_vector_peak=ops / 1e12 / (med(decim) / 1e3) / VECTOR_PEAK_TOPS),
           "tiles": dict(stage(tiles), frames=n * F), "finish": stage(finish), "all_stages_ms": med(decim) + med(tiles) + med(finish),
           "audio_seconds_per_s": n * a.seconds / ((med(decim) + med(tiles) + med(finish)) / 1e3)}
    line = (f"decimation: {n} x {a.seconds:.0f} s: {med(decim):.2f} ms ({min(decim):.2f} .. {max(decim):.2f}) = {out['decimation']['pcm_gb_per_s']:.0f} GB/s of PCM, "
            f"{out['decimation']['tera_lane_ops_per_s']:.1f} T lane-operations/s = {100 * out['decimation']['share_of_vector_peak']:.1f} % of the vector peak; "
            f"a read-only pass {med(read):.2f} ms = {100 * med(read) / med(decim):.1f} % of it\n"
            f"tiles: {n * F} frames: {med(tiles):.2f} ms ({min(tiles):.2f} .. {max(tiles):.2f})\n"
            f"finish: {med(finish):.3f} ms ({min(finish):.3f} .. {max(finish):.3f})")
    if hn:
        h1, hf = med(host_stage1) * n / hn, med(host_finish) * n / hn
        out["host_stage1"] = dict(host_threads=a.threads, host_tracks=hn, host_ms=h1, host_ms_all_unscaled=host_stage1, kernels_over_host=h1 / (med(decim) + med(tiles)))
        out["host_stage2"] = dict(host_threads=a.threads, host_tracks=hn, host_ms=hf, host_ms_all_unscaled=host_finish, kernels_over_host=hf / med(finish))
        line += (f"\nhost x{a.threads}: stage 1 {h1:.0f} ms ({h1 / (med(decim) + med(tiles)):.0f} x), stage 2 {hf:.1f} ms ({hf / med(finish):.0f} x); "
                 f"{bad.value} mismatching tracks, rows or records")
    print(line, flush=True)
    Path(a.json).parent.mkdir(parents=True, exist_ok=True)
    Path(a.json).write_text(json.dumps(out, indent=1) + "\n")
    if bad.value:
        raise SystemExit(f"{bad.value} host signals, rows or finish records differ from the kernels'")


if __name__ == "__main__":
    main()
