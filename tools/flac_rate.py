#!/usr/bin/env python3
"""FLAC album against its WAV twin, in one process: paths to album gain through rg_analyze_album, each route warmed up,
median of `reps` calls; plus the host's frame-index pass alone (one thread) and the host-decoder route (tuning key 14 = 0).

    tools/flac_rate.py [--distinct 16] [--copies 16] [--seconds 60] [--reps 3] [--json out.json]

16 distinct tracks, each behind `copies` paths (the file route does not de-duplicate).  Run the device decode chain's
per-kernel times with `rocprofv3 --kernel-trace --stats -- python tools/flac_rate.py ...` in a run of its own."""
import argparse
import json
import statistics
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import flacenc as fe  # noqa: E402
from wavutil import wav_bytes  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--distinct", type=int, default=16)
    ap.add_argument("--copies", type=int, default=16)
    ap.add_argument("--seconds", type=float, default=60.0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import torch  # noqa: F401

    import mp3rgain_amd as rg
    from mp3rgain_amd import flacdec

    tmp = Path(tempfile.mkdtemp())
    rng = np.random.default_rng(0xF1AC)
    flacs, wavs, srcs = [], [], []
    n = int(44100 * a.seconds)
    t0 = time.perf_counter()
    for k in range(a.distinct):
        pcm = fe.test_pcm(rng, 2, n + k, 16)
        f, w = tmp / f"s{k}.flac", tmp / f"s{k}.wav"
        f.write_bytes(fe.encode(pcm, 44100, 16, fe.Options(stereo="mid_side", subframe="auto", partition_order=4)))
        w.write_bytes(wav_bytes([pcm[0], pcm[1]], 44100, "s16"))
        srcs.append(f)
        for j in range(a.copies):
            (tmp / f"t{k}_{j}.flac").symlink_to(f)
            (tmp / f"t{k}_{j}.wav").symlink_to(w)
            flacs.append(str(tmp / f"t{k}_{j}.flac"))
            wavs.append(str(tmp / f"t{k}_{j}.wav"))
    enc_s = time.perf_counter() - t0
    flac_bytes = sum(Path(p).stat().st_size for p in flacs)
    wav_bytes_total = sum(Path(p).stat().st_size for p in wavs)
    data = [s.read_bytes() for s in srcs]
    t0 = time.perf_counter()
    for d in data:
        flacdec.index(d)
    index_s_per_file = (time.perf_counter() - t0) / len(data)
    res = {"files": len(flacs), "seconds_per_track": a.seconds, "flac_bytes": flac_bytes, "wav_bytes": wav_bytes_total,
           "compression": flac_bytes / wav_bytes_total, "encode_s": enc_s, "host_index_ms_per_file_one_thread": index_s_per_file * 1e3}
    with rg.Analyzer(0) as an:
        def timed(paths, route=1):
            an.set_tuning(14, route)
            an.analyze_album_files(paths)  # warm-up
            ts = []
            for _ in range(a.reps):
                t = time.perf_counter()
                r = an.analyze_album_files(paths)
                ts.append(time.perf_counter() - t)
            return statistics.median(ts), r
        tf, rf = timed(flacs)
        tw, rw = timed(wavs)
        th, rh = timed(flacs, 0)
        an.set_tuning(14, 1)
    assert (rf.album_loudness_db, rf.album_peak) == (rw.album_loudness_db, rw.album_peak) == (rh.album_loudness_db, rh.album_peak)
    pcm_bytes = len(flacs) * n * 2 * 2
    res.update({"album_flac_device_ms": tf * 1e3, "album_wav_ms": tw * 1e3, "album_flac_host_decoder_ms": th * 1e3,
                "flac_over_wav": tf / tw, "flac_device_gb_per_s_of_pcm": pcm_bytes / tf / 1e9, "same_album_result": True})
    print(json.dumps(res))
    if a.json:
        Path(a.json).write_text(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
