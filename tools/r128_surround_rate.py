#!/usr/bin/env python3
"""The weighted (multichannel) EBU R 128 call against the plain stereo call on the same PCM bytes, in one process, alternating.

The arena holds 200 three-minute 48 kHz S16 tracks of six channels, on the device.  The weighted call
(rg_r128_analyze_pcm_weighted, the 5.1 layout's weights) reads it as those 200 tracks; the plain call
(rg_r128_analyze_pcm_batch) reads the very same bytes as 600 stereo tracks of the same length.  After a warm-up (tables,
buffers, clocks) the two take turns and the median of each is reported: ms, and GB/s of PCM (arena bytes / time).  What the
weighted call adds is one fold launch over 8 bytes per channel-hop (4800 frames x 2 bytes = 9600 bytes of PCM): its device
time comes from a kernel trace of a run of its own (--trace: rocprofv3 --kernel-trace --stats around `--child`).

    python tools/r128_surround_rate.py [--tracks 200] [--minutes 3] [--reps 11] [--trace] [--out profiles/r128_surround_rate.json]
    python tools/r128_surround_rate.py --plain-only          # the plain call alone (a tree without the weighted entry)
    python tools/r128_surround_rate.py --parent parent.json  # record a --plain-only result of the parent commit beside the others
"""
import argparse
import csv
import json
import shutil
import statistics
import subprocess
import sys
import tempfile
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

RATE = 48000
CHANNELS = 6


def fold_trace(args) -> dict:
    """Device time of the fold launches (and of the main kernel beside them) from a kernel trace of one more process."""
    prof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    with tempfile.TemporaryDirectory() as d:
        cmd = [prof, "--kernel-trace", "--stats", "-d", d, "--output-format", "csv", "--", sys.executable, str(Path(__file__).resolve()),
               "--child", "--tracks", str(args.tracks), "--minutes", str(args.minutes), "--reps", str(args.reps)]
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
        if p.returncode != 0:
            return {"error": (p.stderr or p.stdout)[-400:]}
        rows = []
        for f in Path(d).rglob("*kernel_stats.csv"):
            rows += list(csv.DictReader(f.open()))
    out = {}
    for r in rows:
        for key, name in (("fold", "rg_r128_fold_kernel"), ("main_s16", "rg_r128_main_kernel")):
            if name in r.get("Name", ""):
                calls = int(r["Calls"])
                out[key] = {"kernel": r["Name"], "calls": calls, "total_us": float(r["TotalDurationNs"]) / 1e3,
                            "mean_us": float(r["TotalDurationNs"]) / 1e3 / max(calls, 1)}
    return out or {"error": "no kernel statistics found"}


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--tracks", type=int, default=200)
    ap.add_argument("--minutes", type=float, default=3.0)
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--child", action="store_true", help="the traced run: warm-up, then `reps` weighted calls and nothing else")
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--parent", default=None, help="a --plain-only result measured on the parent commit")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch

    import mp3rgain_amd as rg
    from mp3rgain_amd import _capi

    lib = _capi.load()
    an = rg.Analyzer(0)
    n, frames = args.tracks, int(round(args.minutes * 60 * RATE))
    total = n * CHANNELS * frames
    pcm = torch.empty(total, dtype=torch.int16, device="cuda")
    gen = torch.Generator(device="cuda").manual_seed(0x5128)
    step = 1 << 28
    for a in range(0, total, step):  # noise at about -14 dBFS, every sample of its own
        k = min(step, total - a)
        pcm[a:a + k] = (torch.randn(k, generator=gen, device="cuda") * 6500.0).clamp_(-32768, 32767).to(torch.int16)
    torch.cuda.synchronize()
    nbytes = total * 2

    def descs_of(count, channels):
        d = (_capi.TrackDesc * count)()
        for t in range(count):
            d[t].offset_bytes = t * channels * frames * 2
            d[t].frames = frames
            d[t].sample_rate = RATE
            d[t].channels = channels
            d[t].format = _capi.FMT_S16_PLANAR
        return d

    n_plain = n * CHANNELS // 2
    d_plain, d_six = descs_of(n_plain, 2), descs_of(n, CHANNELS)
    out_plain = (_capi.R128TrackResult * n_plain)()
    out_six = (_capi.R128TrackResult * n)()

    def plain():
        assert lib.rg_r128_analyze_pcm_batch(an.handle, d_plain, n_plain, pcm.data_ptr(), nbytes, 1, 0, out_plain, None) == 0

    weighted = None
    if not args.plain_only:
        weights = (_capi.R128ChannelWeights * n)()
        for t in range(n):
            for k, v in enumerate(rg.r128_layout_weights(CHANNELS)):
                weights[t].w[k] = v

        def weighted():
            assert lib.rg_r128_analyze_pcm_weighted(an.handle, d_six, weights, n, None, 0, pcm.data_ptr(), nbytes, 1, 0, out_six, None,
                                                    None, None, None, None) == 0

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()  # synchronous: results are on the host when it returns
        return (time.perf_counter() - t0) * 1e3

    for _ in range(6):
        plain()
        if weighted:
            weighted()
    if args.child:
        for _ in range(args.reps):
            weighted()
        an.close()
        return 0
    t = {"plain": [], "weighted": []}
    for _ in range(args.reps):
        t["plain"].append(timed(plain))
        if weighted:
            t["weighted"].append(timed(weighted))
    result = {"workload": f"{n} x {args.minutes:g} min x {RATE} Hz x {CHANNELS} channels S16, device arena, {nbytes} bytes; the plain "
                          f"call reads them as {n_plain} stereo tracks", "reps": args.reps, "pcm_bytes": nbytes}
    for k, v in t.items():
        if v:
            med = statistics.median(v)
            result[k] = {"ms": med, "min_ms": min(v), "max_ms": max(v), "gb_per_s": nbytes / (med * 1e-3) / 1e9}
    result["plain"]["loudness_lufs_track0"] = out_plain[0].loudness_lufs
    if weighted:
        result["weighted"]["loudness_lufs_track0"] = out_six[0].loudness_lufs
        hops = frames // ((RATE + 5) // 10)
        result["fold_bytes"] = {"read": 8 * CHANNELS * hops * n, "written": 8 * hops * n}
    an.close()
    if args.trace and weighted:
        del pcm
        torch.cuda.empty_cache()
        result["fold_device_time"] = fold_trace(args)
    if args.parent:
        parent = json.loads(Path(args.parent).read_text())
        result["plain_on_parent_commit"] = parent["plain"]
    line = json.dumps(result)
    print(line)
    if args.out:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
