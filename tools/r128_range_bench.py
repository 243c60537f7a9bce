#!/usr/bin/env python3
"""What loudness range and the momentary / short-term maxima add to an EBU R 128 call, on the arena of tools/r128_bench.py.

The arena is BASELINE.json configs[2]: 1000 synthetic 3-minute 44.1 kHz stereo F32 tracks, generated on the device.  After a
warm-up the synchronous calls take turns in one process -- rg_r128_analyze_pcm_batch and rg_r128_analyze_album_pcm, each
plain and as *_dynamics; the album's selection both as one workgroup and as wide counting passes (tuning key 2 = 1, 2) --
and the median of each is reported with the difference to the plain call of the same kind.  The bytes come from the launch
shapes: the block kernel reads every hop energy once and writes every short-term block once; a selection makes 2 gate passes
and 6 counting passes over the block values (per track, and once more over all of them for the album).

    python tools/r128_range_bench.py [--tracks 1000] [--minutes 3] [--reps 11] [--out profiles/r128_range_bench.json]
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
PASSES = 8  # 2 gate passes + 6 counting passes of the radix select


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--tracks", type=int, default=1000)
    ap.add_argument("--minutes", type=float, default=3.0)
    ap.add_argument("--reps", type=int, default=11)
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
    out = (_capi.R128TrackResult * n)()
    alb = _capi.R128AlbumResult()
    dyn = (_capi.R128Dynamics * n)()
    adyn = _capi.R128Dynamics()
    args_ = (an.handle, descs, n, pcm.data_ptr(), nbytes, 1, 0)

    def batch():
        assert lib.rg_r128_analyze_pcm_batch(*args_, out, None) == 0

    def batch_dyn():
        assert lib.rg_r128_analyze_pcm_batch_dynamics(*args_, out, None, dyn, None) == 0

    def album():
        assert lib.rg_r128_analyze_album_pcm(*args_, out, C.byref(alb), None) == 0

    def album_dyn(mode):
        an.set_tuning_r128(2, mode)
        assert lib.rg_r128_analyze_album_pcm_dynamics(*args_, out, C.byref(alb), None, dyn, C.byref(adyn), None) == 0

    # the album alone, its tracks' hop energies already analysed: not separable through the ABI; the three album calls differ
    # only in the selection
    calls = {"batch": batch, "batch_dynamics": batch_dyn, "album": album,
             "album_dynamics_one_workgroup": lambda: album_dyn(1), "album_dynamics_wide": lambda: album_dyn(2)}

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()  # synchronous: results are on the host when it returns
        return (time.perf_counter() - t0) * 1e3

    for _ in range(4):  # warm-up: tables, buffers, clocks
        for fn in calls.values():
            fn()
    t = {k: [] for k in calls}
    album_values = {}
    for _ in range(args.reps):
        for k, fn in calls.items():
            t[k].append(timed(fn))
            if k.startswith("album_dynamics"):
                album_values[k] = [adyn.loudness_range_lu, adyn.range_low_lufs, adyn.range_high_lufs, adyn.st_blocks, adyn.st_blocks_gated]
    an.set_tuning_r128(2, 0)
    med = {k: statistics.median(v) for k, v in t.items()}
    hop = (RATE + 5) // 10
    H = frames // hop
    st_blocks = n * max(H - 29, 0)
    result = {
        "workload": f"{n} x {args.minutes:g} min x {RATE} Hz stereo F32, device arena", "reps": args.reps,
        "median_ms": med, "min_ms": {k: min(v) for k, v in t.items()},
        "added_ms": {"batch_dynamics": med["batch_dynamics"] - med["batch"],
                     "album_dynamics_one_workgroup": med["album_dynamics_one_workgroup"] - med["album"],
                     "album_dynamics_wide": med["album_dynamics_wide"] - med["album"]},
        "short_term_blocks": st_blocks,
        "bytes": {"pcm_read_by_the_loudness_kernel_not_again": nbytes,
                  "hop_energies_read_once": 2 * n * H * 8, "block_values_written_once": st_blocks * 8,
                  "block_values_read_per_selection": PASSES * st_blocks * 8, "passes": PASSES},
        "album_values_equal_in_both_modes": album_values.get("album_dynamics_one_workgroup") == album_values.get("album_dynamics_wide"),
        "album": dict(zip(("loudness_range_lu", "range_low_lufs", "range_high_lufs", "st_blocks", "st_blocks_gated"),
                          album_values.get("album_dynamics_wide", []))),
        "track0": {"loudness_range_lu": dyn[0].loudness_range_lu, "max_momentary_lufs": dyn[0].max_momentary_lufs,
                   "max_short_term_lufs": dyn[0].max_short_term_lufs},
    }
    line = json.dumps(result)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")
    an.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
