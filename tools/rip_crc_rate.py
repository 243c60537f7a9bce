#!/usr/bin/env python3
"""The rip checksum kernels against their serial host twin (MI355X): discs of 1 to 64 tracks of four minutes of 44.1 kHz 16-bit
stereo, filled on the device; one launch of the tile kernel and one of the fold kernel hash the arena (rg_rip_rate).

    tools/rip_crc_rate.py [--counts 1,2,4,12,64] [--seconds 240] [--threads 16] [--reps 7] [--warm-ms 400] [--json profiles/rip_crc_rate.json]

Per count, after a warm-up (a fresh process runs slower for a while after a large allocation: the kernels are launched for
`warm-ms` milliseconds first), `reps` rounds alternate the two kernels over all tracks (HIP events around the two launches) with
the serial host twin on `threads` threads over a host copy of the same bytes; medians and the spread (min .. max) are reported.
Both layouts of the plain CRC's table are timed: 0 = one byte table, 1 = slice-by-4.  The host copy is capped at 32 tracks and
its time scaled to the count (tracks are independent and equally long).  Every host record must equal the kernels'.  The FLAC
MD5 kernel (rg_flac_md5_rate: one lane per stream) runs on the same shape at --md5-count tracks for comparison."""
import argparse
import ctypes as C
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

HOST_CAP = 32
HBM_PEAK_GB_S = 8000.0  # MI355X: 8 TB/s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--counts", default="1,2,4,12,64")
    ap.add_argument("--seconds", type=float, default=240.0)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warm-ms", type=float, default=400.0)
    ap.add_argument("--md5-count", type=int, default=12)
    ap.add_argument("--json", default=str(ROOT / "profiles" / "rip_crc_rate.json"))
    a = ap.parse_args()
    import torch  # noqa: F401  (torch first: one HIP runtime per process)

    import mp3rgain_amd as rg
    from mp3rgain_amd import _capi, flacdec

    L = _capi.load()
    frames = int(44100 * a.seconds)
    track_mb = frames * 4 / 1e6
    rows = []
    with rg.Analyzer(0) as an:
        for n in [int(x) for x in a.counts.split(",")]:
            row = {"tracks": n, "track_mb": track_mb}
            for layout, name in ((0, "byte_table"), (1, "slice4")):
                host_n = min(n, HOST_CAP) if layout == 0 else 0  # the host twin does not depend on the device's table layout
                dev = (C.c_double * a.reps)()
                host = (C.c_double * a.reps)()
                bad = C.c_size_t()
                an._check(L.rg_rip_rate(an.handle, n, frames, layout, host_n, a.threads, a.reps, a.warm_ms, dev, host, C.byref(bad)))
                if bad.value:
                    raise SystemExit(f"{bad.value} of {host_n} host records differ from the kernels'")
                ms = statistics.median(dev)
                gbs = n * track_mb / 1e3 / (ms / 1e3)
                row[name] = {"device_ms": ms, "device_ms_min": min(dev), "device_ms_max": max(dev), "device_ms_all": list(dev),
                             "device_gb_per_s": gbs, "fraction_of_hbm_peak": gbs / HBM_PEAK_GB_S}
                if host_n:
                    hm = statistics.median(host) * n / host_n
                    row.update(host_threads=a.threads, host_tracks_hashed=host_n, host_ms=hm, host_ms_all_unscaled=list(host),
                               host_gb_per_s=n * track_mb / 1e3 / (hm / 1e3))
            rows.append(row)
            b, s = row["byte_table"], row["slice4"]
            print(f"{n:3d} tracks x {track_mb:.1f} MB: byte table {b['device_ms']:8.3f} ms ({b['device_ms_min']:.3f} .. {b['device_ms_max']:.3f}; "
                  f"{b['device_gb_per_s']:.0f} GB/s = {100 * b['fraction_of_hbm_peak']:.1f} % of HBM peak), slice-by-4 {s['device_ms']:8.3f} ms "
                  f"({s['device_ms_min']:.3f} .. {s['device_ms_max']:.3f}; {s['device_gb_per_s']:.0f} GB/s), host x{a.threads} {row['host_ms']:9.1f} ms "
                  f"({row['host_gb_per_s']:.2f} GB/s)", flush=True)
        md5 = None
        if a.md5_count:
            n = a.md5_count
            dev = (C.c_double * 3)()
            an._check(flacdec._lib().rg_flac_md5_rate(an.handle, n, frames, 2, 0, a.threads, 3, dev, None, None))
            ms = statistics.median(dev)
            md5 = {"streams": n, "device_ms": ms, "device_ms_all": list(dev), "device_gb_per_s": n * track_mb / 1e3 / (ms / 1e3)}
            print(f"FLAC MD5 kernel, {n} streams of the same shape: {ms:.1f} ms ({md5['device_gb_per_s']:.2f} GB/s)")
    best = "slice4" if statistics.median(r["slice4"]["device_ms"] / r["byte_table"]["device_ms"] for r in rows) < 1.0 else "byte_table"
    result = {"tool": "rip_crc_rate", "seconds_per_track": a.seconds, "rate": 44100, "channels": 2, "bits": 16, "reps": a.reps, "warm_ms": a.warm_ms,
              "hbm_peak_gb_per_s": HBM_PEAK_GB_S, "rows": rows, "faster_table_layout": best,
              "device_ahead_at": [r["tracks"] for r in rows if r[best]["device_ms"] < r["host_ms"]], "flac_md5_kernel": md5}
    print(f"faster table layout: {best}; device ahead of the host twin at {result['device_ahead_at']} tracks")
    Path(a.json).parent.mkdir(parents=True, exist_ok=True)
    Path(a.json).write_text(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
