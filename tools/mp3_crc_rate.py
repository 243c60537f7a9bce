#!/usr/bin/env python3
"""The MP3 CRC kernels against their host twin (MI355X): 64, 256 and 1000 streams of 5 MB of pseudo-random bytes filled on
the device (rg_mp3_crc_rate).  The chunk and fold kernels hash all streams in one launch each; the frame-CRC kernel checks
`--frames` synthetic protected frames.

    tools/mp3_crc_rate.py [--counts 64,256,1000] [--mb 5] [--threads 16] [--reps 5] [--frames 1000000] [--json profiles/mp3_crc_rate.json]

Per count, after a warm-up of both sides, `reps` rounds alternate the kernels (HIP events around the launches) with the host
twin on `threads` threads over a host copy of the same bytes; medians are reported.  The host copy is capped at 64 streams and
its time scaled to the count (streams are independent and equally long).  Every host result must equal the device's."""
import argparse
import ctypes as C
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

HOST_CAP = 64


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--counts", default="64,256,1000")
    ap.add_argument("--mb", type=float, default=5.0)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--frames", type=int, default=1000000)
    ap.add_argument("--json", default=str(ROOT / "profiles" / "mp3_crc_rate.json"))
    a = ap.parse_args()
    import torch  # noqa: F401  (torch first: one HIP runtime per process)

    import mp3rgain_amd as rg
    from mp3rgain_amd import mp3verify

    L = mp3verify._lib()
    stream_bytes = int(a.mb * 1e6)
    rows = []
    with rg.Analyzer(0) as an:
        for n in [int(x) for x in a.counts.split(",")]:
            host_n = min(n, HOST_CAP)
            dev, host, fdev, fhost = ((C.c_double * a.reps)() for _ in range(4))
            bad = C.c_size_t()
            an._check(L.rg_mp3_crc_rate(an.handle, n, stream_bytes, host_n, a.threads, a.reps, a.frames, dev, host, fdev, fhost, C.byref(bad)))
            if bad.value:
                raise SystemExit(f"{bad.value} host results differ from the device's")
            dev_ms = statistics.median(dev)
            host_ms = statistics.median(host) * n / host_n
            row = {"streams": n, "stream_mb": stream_bytes / 1e6, "device_ms": dev_ms, "device_ms_all": list(dev),
                   "device_gb_per_s": n * stream_bytes / 1e6 / dev_ms, "host_threads": a.threads, "host_streams_hashed": host_n,
                   "host_ms": host_ms, "host_ms_all_unscaled": list(host), "host_gb_per_s": n * stream_bytes / 1e6 / host_ms,
                   "host_over_device": host_ms / dev_ms, "frames": a.frames, "frame_device_ms": statistics.median(fdev),
                   "frame_host_ms": statistics.median(fhost), "frame_host_over_device": statistics.median(fhost) / statistics.median(fdev)}
            rows.append(row)
            print(f"{n:5d} streams x {row['stream_mb']:.1f} MB: device {dev_ms:8.2f} ms ({row['device_gb_per_s']:.1f} GB/s), host x{a.threads} "
                  f"{host_ms:8.1f} ms ({row['host_gb_per_s']:.2f} GB/s), host / device {row['host_over_device']:.1f}; {a.frames} frame CRCs: "
                  f"device {row['frame_device_ms']:.3f} ms, host {row['frame_host_ms']:.2f} ms", flush=True)
    result = {"tool": "mp3_crc_rate", "reps": a.reps, "rows": rows, "device_ahead_at": [r["streams"] for r in rows if r["device_ms"] < r["host_ms"]]}
    print(f"device ahead at {result['device_ahead_at']} streams (kernel time against host time; the copy to the device is not in it)")
    Path(a.json).parent.mkdir(parents=True, exist_ok=True)
    Path(a.json).write_text(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
