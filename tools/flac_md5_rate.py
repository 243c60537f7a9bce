#!/usr/bin/env python3
"""The FLAC MD5 kernel against its host twin (MI355X): arenas of 64, 256 and 1000 streams of three minutes of 44.1 kHz
16-bit stereo, filled on the device; one lane hashes one stream, one launch hashes the arena (rg_flac_md5_rate).

    tools/flac_md5_rate.py [--counts 64,256,1000] [--seconds 180] [--threads 16] [--reps 5] [--json profiles/flac_md5_rate.json]

Per count, after a warm-up of both sides, `reps` rounds alternate the kernel over all streams (HIP events around the launch)
with the host twin on `threads` threads over a host copy of the same bytes; medians are reported.  The host copy is capped
at 256 streams and its time scaled to the count (streams are independent and equally long).  Every host digest must equal
the kernel's."""
import argparse
import ctypes as C
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

HOST_CAP = 256


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--counts", default="64,256,1000")
    ap.add_argument("--seconds", type=float, default=180.0)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--json", default=str(ROOT / "profiles" / "flac_md5_rate.json"))
    a = ap.parse_args()
    import torch  # noqa: F401  (torch first: one HIP runtime per process)

    import mp3rgain_amd as rg
    from mp3rgain_amd import flacdec

    L = flacdec._lib()
    frames, channels = int(44100 * a.seconds), 2
    stream_mb = frames * channels * 2 / 1e6
    rows = []
    with rg.Analyzer(0) as an:
        for n in [int(x) for x in a.counts.split(",")]:
            host_n = min(n, HOST_CAP)
            dev = (C.c_double * a.reps)()
            host = (C.c_double * a.reps)()
            bad = C.c_size_t()
            an._check(L.rg_flac_md5_rate(an.handle, n, frames, channels, host_n, a.threads, a.reps, dev, host, C.byref(bad)))
            if bad.value:
                raise SystemExit(f"{bad.value} of {host_n} host digests differ from the kernel's")
            dev_ms = statistics.median(dev)
            host_ms = statistics.median(host) * n / host_n
            row = {"streams": n, "stream_mb": stream_mb, "device_ms": dev_ms, "device_ms_all": list(dev),
                   "device_mb_per_s_per_stream": stream_mb / (dev_ms / 1e3), "device_mb_per_s": n * stream_mb / (dev_ms / 1e3),
                   "host_threads": a.threads, "host_streams_hashed": host_n, "host_ms": host_ms,
                   "host_ms_all_unscaled": list(host), "host_mb_per_s": n * stream_mb / (host_ms / 1e3),
                   "host_mb_per_s_per_thread": n * stream_mb / (host_ms / 1e3) / a.threads, "device_over_host": host_ms / dev_ms}
            rows.append(row)
            print(f"{n:5d} streams x {stream_mb:.1f} MB: device {dev_ms:9.1f} ms ({row['device_mb_per_s_per_stream']:.1f} MB/s per stream, "
                  f"{row['device_mb_per_s']:.0f} MB/s), host x{a.threads} {host_ms:9.1f} ms ({row['host_mb_per_s']:.0f} MB/s), "
                  f"host / device {row['device_over_host']:.2f}", flush=True)
    # the count from which the device is ahead: the device's time is flat in the count while every lane of its waves has a
    # stream and the host's grows with it, so it is where the host's per-stream time times n crosses the device's time
    per_stream_host = statistics.median(r["host_ms"] / r["streams"] for r in rows)
    flat_dev = statistics.median(r["device_ms"] for r in rows)
    result = {"tool": "flac_md5_rate", "seconds_per_stream": a.seconds, "rate": 44100, "channels": channels, "bits": 16, "reps": a.reps,
              "rows": rows, "host_ms_per_stream": per_stream_host, "break_even_streams_estimate": flat_dev / per_stream_host,
              "device_ahead_at": [r["streams"] for r in rows if r["device_ms"] < r["host_ms"]]}
    print(f"host {per_stream_host:.2f} ms per stream on {a.threads} threads; device ahead at {result['device_ahead_at']} "
          f"(estimated break-even {result['break_even_streams_estimate']:.0f} streams)")
    Path(a.json).parent.mkdir(parents=True, exist_ok=True)
    Path(a.json).write_text(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
