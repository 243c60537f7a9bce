#!/usr/bin/env python3
"""The plain EBU R 128 calls, once each, for a kernel trace: rg_r128_analyze_pcm_batch and rg_r128_analyze_album_pcm without
and with true peak on a small host arena (six tracks, three sample formats, two rates).  It binds only the symbols those
calls need, so it runs on any build of the library that has the R 128 path:

    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -- python tools/r128_plain_calls.py [--lib <libmp3rgain_amd.so>]

Two builds launch the same work for these calls exactly if their kernel_stats files list the same kernels with the same
call counts (profiles/r128_plain_calls_*.csv).
"""
import argparse
import ctypes as C
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent


class TrackDesc(C.Structure):
    _fields_ = [("offset_bytes", C.c_uint64), ("frames", C.c_uint64), ("sample_rate", C.c_uint32), ("channels", C.c_uint16),
                ("format", C.c_uint16)]


class TrackResult(C.Structure):
    _fields_ = [("loudness_lufs", C.c_double), ("gain_db", C.c_double), ("sample_peak", C.c_double), ("true_peak", C.c_double),
                ("sample_rate", C.c_uint32), ("blocks", C.c_uint32), ("blocks_gated", C.c_uint32), ("flags", C.c_uint32)]


class AlbumResult(C.Structure):
    _fields_ = [("loudness_lufs", C.c_double), ("gain_db", C.c_double), ("sample_peak", C.c_double), ("true_peak", C.c_double),
                ("blocks", C.c_uint32), ("blocks_gated", C.c_uint32)]


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--lib", default=str(ROOT / "mp3rgain_amd" / "libmp3rgain_amd.so"))
    args = ap.parse_args()
    L = C.CDLL(args.lib)
    L.rg_create.restype = C.c_void_p
    L.rg_create.argtypes = [C.c_int]
    L.rg_destroy.argtypes = [C.c_void_p]
    batch_args = [C.c_void_p, C.POINTER(TrackDesc), C.c_size_t, C.c_void_p, C.c_size_t, C.c_int, C.c_int, C.POINTER(TrackResult)]
    L.rg_r128_analyze_pcm_batch.argtypes = batch_args + [C.c_void_p]
    L.rg_r128_analyze_album_pcm.argtypes = batch_args + [C.POINTER(AlbumResult), C.c_void_p]

    rng = np.random.default_rng(1)
    parts, descs, off = [], [], 0
    for i, (rate, dtype, fmt, nch) in enumerate(((44100, np.float32, 0, 2), (48000, np.int16, 1, 2), (96000, np.int32, 2, 1),
                                                 (44100, np.int16, 1, 1), (192000, np.float32, 0, 2), (48000, np.float32, 0, 2))):
        frames = 6 * rate + 13 * i
        x = 0.2 * rng.standard_normal((nch, frames))
        if dtype is not np.float32:
            x = np.round(x.clip(-1, 1) * (32767 if dtype is np.int16 else 2147483647))
        raw = x.astype(dtype).tobytes()
        off = (off + 3) & ~3
        descs.append((off, frames, rate, nch, fmt))
        parts.append((off, raw))
        off += len(raw)
    arena = np.zeros(off, dtype=np.uint8)
    for o, raw in parts:
        arena[o:o + len(raw)] = np.frombuffer(raw, dtype=np.uint8)
    n = len(descs)
    d = (TrackDesc * n)(*[TrackDesc(*t) for t in descs])
    out = (TrackResult * n)()
    alb = AlbumResult()
    ctx = L.rg_create(0)
    assert ctx
    for tp in (0, 1):
        assert L.rg_r128_analyze_pcm_batch(ctx, d, n, arena.ctypes.data, arena.nbytes, 0, tp, out, None) == 0
        print("batch", tp, [round(out[i].loudness_lufs, 6) for i in range(n)])
        assert L.rg_r128_analyze_album_pcm(ctx, d, n, arena.ctypes.data, arena.nbytes, 0, tp, out, C.byref(alb), None) == 0
        print("album", tp, round(alb.loudness_lufs, 6), alb.blocks, alb.blocks_gated)
    L.rg_destroy(ctx)
    return 0


if __name__ == "__main__":
    sys.exit(main())
