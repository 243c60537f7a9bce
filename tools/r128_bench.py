#!/usr/bin/env python3
"""EBU R 128 analysis against the ReplayGain 1.0 analysis on the same arena, in one process, alternating.

The arena is BASELINE.json configs[2]: 1000 synthetic 3-minute 44.1 kHz stereo F32 tracks, generated on the device
(rg_synth_fill_device).  After a warm-up (bench.py's pre-roll: the shader clock settles) the three synchronous calls take
turns -- rg_analyze_pcm_batch (ReplayGain 1.0), rg_r128_analyze_pcm_batch without and with true peak -- and the median of
each is reported: ms, stereo samples per second, and bytes read / time as a share of 8 TB/s, where the bytes come from the
launch shapes: 8 per stereo frame x (1 + 3 / S) for the loudness kernel (a lane re-reads three warm-up hops per S hops),
twice the arena in total with the true peak.

    python tools/r128_bench.py [--tracks 1000] [--minutes 3] [--reps 11] [--s 0,16,32,64] [--out profiles/r128_bench.json]
"""
import argparse
import ctypes as C
import json
import statistics
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

RATE = 44100
HBM_BYTES_PER_S = 8e12


def auto_S(channel_hops: int) -> int:
    """rg_r128.hip choose_S: about three waves per SIMD, at least 4 and at most 64 hops per lane."""
    target = 256 * 4 * 3 * 64
    return min(max((channel_hops + target - 1) // target, 4), 64)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--tracks", type=int, default=1000)
    ap.add_argument("--minutes", type=float, default=3.0)
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--s", default="0", help="hops per lane to measure, comma separated; 0 = chosen by the library")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    import mp3rgain_amd as rg
    from mp3rgain_amd import _capi

    lib = _capi.load()
    an = rg.Analyzer(0)
    n, frames = args.tracks, int(round(args.minutes * 60 * RATE))
    pcm = torch.empty(2 * frames * n, dtype=torch.float32, device="cuda")
    descs = (_capi.TrackDesc * n)()
    for t in range(n):
        for c in range(2):
            an.synth_fill_device(pcm[(2 * t + c) * frames:].data_ptr(), 0x5EED0000 + t, c, RATE, 0, frames)
        descs[t].offset_bytes = 2 * t * frames * 4
        descs[t].frames = frames
        descs[t].sample_rate = RATE
        descs[t].channels = 2
        descs[t].format = _capi.FMT_F32_PLANAR
    torch.cuda.synchronize()
    nbytes = 2 * frames * n * 4
    out1 = (_capi.TrackResult * n)()
    out2 = (_capi.R128TrackResult * n)()

    def rg1():
        assert lib.rg_analyze_pcm_batch(an.handle, descs, n, pcm.data_ptr(), nbytes, 1, out1, None) == 0

    def r128(tp):
        assert lib.rg_r128_analyze_pcm_batch(an.handle, descs, n, pcm.data_ptr(), nbytes, 1, int(tp), out2, None) == 0

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()  # synchronous: results are on the host when it returns
        return (time.perf_counter() - t0) * 1e3

    for _ in range(6):  # warm-up: tables, buffers, clocks
        rg1()
        r128(False)
    r128(True)
    hop = (RATE + 5) // 10
    channel_hops = 2 * n * (frames // hop)
    stereo_frames = n * frames
    result = {"workload": f"{n} x {args.minutes:g} min x {RATE} Hz stereo F32, device arena", "reps": args.reps, "runs": []}
    for S in [int(v) for v in args.s.split(",")]:
        an.set_tuning_r128(1, S)
        r128(False)
        t = {"rg1": [], "r128": [], "r128_tp": []}
        for _ in range(args.reps):
            t["rg1"].append(timed(rg1))
            t["r128"].append(timed(lambda: r128(False)))
            t["r128_tp"].append(timed(lambda: r128(True)))
        used = S or auto_S(channel_hops)
        med = {k: statistics.median(v) for k, v in t.items()}
        loud_bytes = 8.0 * stereo_frames * (1.0 + 3.0 / used)
        run = {"S": S, "S_used": used,
               "rg1_ms": med["rg1"], "r128_ms": med["r128"], "r128_true_peak_ms": med["r128_tp"],
               "rg1_min_ms": min(t["rg1"]), "r128_min_ms": min(t["r128"]), "r128_true_peak_min_ms": min(t["r128_tp"]),
               "rg1_stereo_samples_per_s": stereo_frames / med["rg1"] * 1e3,
               "r128_stereo_samples_per_s": stereo_frames / med["r128"] * 1e3,
               "r128_true_peak_stereo_samples_per_s": stereo_frames / med["r128_tp"] * 1e3,
               "r128_bytes_read": loud_bytes,
               "r128_share_of_8TBps": loud_bytes / (med["r128"] * 1e-3) / HBM_BYTES_PER_S,
               "r128_true_peak_bytes_read": loud_bytes + 8.0 * stereo_frames,
               "r128_true_peak_share_of_8TBps": (loud_bytes + 8.0 * stereo_frames) / (med["r128_tp"] * 1e-3) / HBM_BYTES_PER_S,
               "loudness_lufs_track0": out2[0].loudness_lufs}
        result["runs"].append(run)
    an.set_tuning_r128(1, 0)
    line = json.dumps(result)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")
    an.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
