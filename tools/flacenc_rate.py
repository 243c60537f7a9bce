#!/usr/bin/env python3
"""The rates of the FLAC encoder's kernels (MI355X) and of their serial host twin, on the workload of profiles/flac_rate.json:
256 tracks of 60 s of 44.1 kHz 16-bit stereo, and the same audio as 24-bit.

    tools/flacenc_rate.py [--tracks 256] [--seconds 60] [--distinct 16] [--host-tracks 16] [--threads 16] [--reps 5]
                          [--json profiles/flacenc_rate.json]

The audio is the project's music-like synthesis (include/rg_synth.h through oracle/pyoracle.py), `distinct` different tracks
repeated to fill the list (the synthesis on the host is what limits this); 24-bit: the float signal rounded to 24 bits.  Per leg
(rg_flac_encode_rate): a first round finds the streams' size, a second warms up, then `reps` rounds run the analyse, layout, write
and MD5 kernels in turn over one arena with HIP events around each launch alone, then a read-only pass over the same arena
(after a warm-up of its own); medians are reported.
  1. the three kernels and the MD5 kernel at max_lpc_order 8, beside the read-only pass and the device decode of that album
     (50.2 ms, profiles/flac_rate.json);
  2. stream bytes over PCM bytes at max_lpc_order 0, 8 and 12;
  3. the serial host twin on `threads` threads over the first `host-tracks` tracks, its time scaled to the count; every byte of
     its streams must equal the kernels'.
Compression is not compared with libFLAC: it is on no machine this project has."""
import argparse
import ctypes as C
import json
import sys
import time
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

FLAC_DECODE_MS = 50.2  # profiles/flac_rate.json: the device decode of this album


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tracks", type=int, default=256)
    ap.add_argument("--seconds", type=float, default=60.0)
    ap.add_argument("--distinct", type=int, default=16)
    ap.add_argument("--host-tracks", type=int, default=16)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--json", default=str(ROOT / "profiles" / "flacenc_rate.json"))
    a = ap.parse_args()
    import torch  # noqa: F401  (torch first: one HIP runtime per process)

    import mp3rgain_amd as rg
    from mp3rgain_amd import _capi
    from oracle import pyoracle as po

    L = _capi.load()
    n, frames = a.tracks, int(44100 * a.seconds)
    distinct = min(a.distinct, n)
    floats = [[po.synth_f32(0xF1AC0000 + k, ch, 44100, frames) for ch in range(2)] for k in range(distinct)]
    legs, differing = [], 0
    with rg.Analyzer(0) as an:
        for bps in (16, 24):
            dt, width = (np.int16, 16) if bps == 16 else (np.int32, 32)
            full = (1 << (bps - 1)) - 1
            planes = [[(np.clip(np.round(x.astype(np.float64) * full), -full - 1, full).astype(np.int64) << (width - bps)).astype(dt) for x in t] for t in floats]
            track_bytes = 2 * frames * (width // 8)
            stride = (track_bytes + 15) // 16 * 16
            arena = np.zeros(n * stride, dtype=np.uint8)
            descs = (_capi.TrackDesc * n)()
            for i in range(n):
                p = planes[i % distinct]
                arena[i * stride:i * stride + track_bytes] = np.concatenate(p).view(np.uint8)
                descs[i].offset_bytes, descs[i].frames, descs[i].sample_rate, descs[i].channels = i * stride, frames, 44100, 2
                descs[i].format = _capi.FMT_S16_PLANAR if bps == 16 else _capi.FMT_S32_PLANAR
            b = (C.c_uint32 * n)(*([bps] * n))
            pcm_bytes = n * frames * 2 * ((bps + 7) // 8)
            for lpc in (8, 0, 12):
                ms = (C.c_double * 5)()
                total = C.c_uint64()
                opts = _capi.FlacEncodeOptions(C.sizeof(_capi.FlacEncodeOptions), 0, lpc, 0)
                an._check(L.rg_flac_encode_rate(an.handle, n, descs, b, arena.ctypes.data, arena.size, C.byref(opts), a.reps, ms, C.byref(total)))
                leg = {"bits_per_sample": bps, "max_lpc_order": lpc, "tracks": n, "seconds": a.seconds, "distinct_tracks": distinct, "reps": a.reps,
                       "analyse_ms": ms[0], "layout_ms": ms[1], "write_ms": ms[2], "md5_ms": ms[3], "read_only_ms": ms[4],
                       "encode_ms": ms[0] + ms[1] + ms[2], "arena_bytes": int(arena.size), "pcm_bytes": pcm_bytes, "stream_bytes": int(total.value),
                       "ratio": total.value / pcm_bytes, "arena_gb_per_s_encode": arena.size / 1e6 / (ms[0] + ms[1] + ms[2]),
                       "arena_gb_per_s_read_only": arena.size / 1e6 / ms[4], "flac_decode_ms_of_this_album": FLAC_DECODE_MS if bps == 16 else None}
                if lpc == 8:  # the twin on `threads` threads, and its bytes against the kernels'
                    hn = min(n, a.host_tracks)
                    hd = [descs[i] for i in range(hn)]
                    dev = an.flac_encode_arena(1, hd, [bps] * hn, arena[:hn * stride], None, lpc)[0]

                    def one(i):
                        return rg.flac_encode_arena(None, 0, [descs[i]], [bps], arena, None, lpc)[0][0]

                    t0 = time.perf_counter()
                    with ThreadPoolExecutor(a.threads) as pool:
                        host = list(pool.map(one, range(hn)))
                    dt_s = time.perf_counter() - t0
                    bad = sum(sum(1 for x, y in zip(p, q) if x != y) + abs(len(p) - len(q)) for p, q in zip(dev, host) if p != q)
                    differing += bad
                    leg.update(host_tracks=hn, host_threads=a.threads, host_ms=1e3 * dt_s, host_ms_scaled_to_all_tracks=1e3 * dt_s * n / hn,
                               differing_bytes=bad)
                legs.append(leg)
                print(json.dumps(leg), flush=True)
    doc = {"tool": "tools/flacenc_rate.py", "device": "MI355X", "legs": legs, "differing_bytes": differing,
           "note": "compression is not compared with libFLAC: it is on no machine this project has"}
    Path(a.json).write_text(json.dumps(doc, indent=1) + "\n")
    return 1 if differing else 0


if __name__ == "__main__":
    sys.exit(main())
