#!/usr/bin/env python3
"""A library scan in album mode (GPU box): N albums x k files as ONE rg_analyze_albums call against N rg_analyze_album calls, in
one warm process, for VBR MP3, 128 kb/s MP3 and FLAC, with 1, 2 and 4 loader threads (tuning key 7).  Prints per case the time
of both forms in the C calls alone (the one call; the sum of the N calls: no Python wrapper time in either), median of `reps`,
stereo samples/s and the ratio; records whether both forms gave the same albums (and exits non-zero when not).

    tools/albums_rate.py [--albums 64] [--per-album 12] [--seconds 60] [--threads 1,2,4] [--reps 3] [--json out.json]

Every file is a path of its own (symlinks to a few distinct streams: the file route reads every path, nothing is de-duplicated)."""
import argparse
import json
import shutil
import statistics
import sys
import tempfile
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import flacenc as fe  # noqa: E402


def mp3_stream(src: Path, seconds: float):
    from mp3rgain_amd import mp3dec

    data = src.read_bytes()
    body = data[int(mp3dec.scan(data).first_frame_offset):]
    one = mp3dec.scan(body)
    stream = body * max(1, int(round(seconds / (one.frames / one.sample_rate))))
    return stream, int(mp3dec.scan(stream).frames)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--albums", type=int, default=64)
    ap.add_argument("--per-album", type=int, default=12)
    ap.add_argument("--seconds", type=float, default=60.0)
    ap.add_argument("--threads", default="1,2,4")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--distinct", type=int, default=4)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import torch  # noqa: F401

    import mp3rgain_amd as rg

    tmp = Path(tempfile.mkdtemp(prefix="rg_albums_rate_"))
    try:
        return run(a, rg, tmp)
    finally:
        shutil.rmtree(tmp, ignore_errors=True)


def run(a, rg, tmp):
    n_files = a.albums * a.per_album
    sources = {}
    vbr, vbr_frames = mp3_stream(ROOT / "tests/golden/fixtures/test_vbr.mp3", a.seconds)
    d128, d128_frames = mp3_stream(ROOT / "tests/golden/mp3/dense_44k_joint_128.mp3", a.seconds)
    sources["mp3_vbr"] = ([vbr], "mp3", vbr_frames)
    sources["mp3_128k"] = ([d128], "mp3", d128_frames)
    rng = np.random.default_rng(0xA1B)
    n = int(44100 * a.seconds)
    flacs = [fe.encode(fe.test_pcm(rng, 2, n, 16), 44100, 16, fe.Options(stereo="mid_side", subframe="auto", partition_order=4))
             for _ in range(a.distinct)]
    sources["flac"] = (flacs, "flac", n)
    res = {"albums": a.albums, "files_per_album": a.per_album, "seconds_per_file": a.seconds, "reps": a.reps, "cases": []}
    with rg.Analyzer(0) as an:
        for label, (streams, ext, frames) in sources.items():
            srcs = []
            for k, s in enumerate(streams):
                p = tmp / f"{label}_src{k}.{ext}"
                p.write_bytes(s)
                srcs.append(p)
            albums = []
            for al in range(a.albums):
                files = []
                for t in range(a.per_album):
                    p = tmp / f"{label}_a{al:04d}_t{t:02d}.{ext}"
                    p.symlink_to(srcs[(al * a.per_album + t) % len(srcs)])
                    files.append(p)
                albums.append(files)
            file_bytes = sum(s.stat().st_size for s in srcs) / len(srcs) * n_files
            for threads in [int(x) for x in a.threads.split(",")]:
                an.set_tuning(7, threads)
                one = an.analyze_albums_files(albums)  # warm-up of both forms
                each = [an.analyze_album_files(f) for f in albums]
                same = len(one) == len(each) and all(isinstance(g, rg.AlbumGainResult) and g == w for g, w in zip(one, each))
                t_one, t_each = [], []
                for _ in range(a.reps):  # the two forms in turn: what disturbs one disturbs the other
                    tm = {}
                    r = an.analyze_albums_files(albums, timing=tm)
                    t_one.append(tm["c_call_seconds"])
                    same = same and r == one
                    total = 0.0
                    for f, w in zip(albums, each):
                        r = an.analyze_album_files(f, timing=tm)
                        total += tm["c_call_seconds"]
                        same = same and r == w
                    t_each.append(total)
                one_s, each_s = statistics.median(t_one), statistics.median(t_each)
                case = {"format": label, "loader_threads": threads, "files": n_files, "file_mb": file_bytes / 1e6,
                        "albums_call_ms": one_s * 1e3, "album_calls_ms": each_s * 1e3,
                        "albums_call_stereo_samples_per_s": n_files * frames / one_s,
                        "album_calls_stereo_samples_per_s": n_files * frames / each_s, "speedup": each_s / one_s,
                        "same_results": same}
                res["cases"].append(case)
                print(f"{label:9s} threads {threads}: one rg_analyze_albums call {one_s * 1e3:8.1f} ms "
                      f"({case['albums_call_stereo_samples_per_s'] / 1e9:.2f} G stereo samples/s) | {a.albums} rg_analyze_album calls "
                      f"{each_s * 1e3:8.1f} ms ({case['album_calls_stereo_samples_per_s'] / 1e9:.2f} G/s) | x{case['speedup']:.2f}"
                      f"{'' if same else ' | RESULTS DIFFER'}", flush=True)
        an.set_tuning(7, 0)
    if a.json:
        Path(a.json).write_text(json.dumps(res, indent=1) + "\n")
    return 0 if all(c["same_results"] for c in res["cases"]) else 1


if __name__ == "__main__":
    sys.exit(main())
