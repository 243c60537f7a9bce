#!/usr/bin/env python3
"""A ReplayGain 2.0 library scan in album mode (GPU box): N albums x k files as ONE rg_r128_analyze_albums[_dynamics] call
against N rg_r128_analyze_album[_dynamics] calls, in one warm process, for VBR MP3, 128 kb/s MP3 and FLAC, with 1, 2 and 4
loader threads (tuning key 7), without and with loudness range.  Prints per case the time of both forms in the C calls alone
(the one call; the sum of the N calls: no Python wrapper time in either), median of `reps`, the two forms in turn, stereo
samples/s and the ratio.

Equality is checked where the contract promises it: in a pass of both forms under a fixed number of hops per lane (R 128
tuning key 1), every album of the one call must equal its single-album call bit for bit (the tool exits non-zero when
not).  The timed passes run under the library's own choice, which depends on the batch's size; the largest difference in
album loudness between the forms there is recorded.

    tools/r128_albums_rate.py [--albums 64] [--per-album 12] [--seconds 60] [--threads 1,2,4] [--dynamics 0,1] [--reps 3]
                              [--json out.json]

Every file is a path of its own (symlinks to a few distinct streams: the file route reads every path, nothing is de-duplicated)."""
import argparse
import json
import shutil
import statistics
import struct
import sys
import tempfile
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
import flacenc as fe  # noqa: E402
from albums_rate import mp3_stream  # noqa: E402

FIXED_S = 8


def record(r):
    """An album's numbers as bytes: NaN compares equal to itself."""
    vals = [r.loudness_lufs, r.gain_db, r.sample_peak, r.true_peak, float(r.blocks), float(r.blocks_gated)]
    for t in r.tracks:
        vals += [t.loudness_lufs, t.gain_db, t.sample_peak, t.true_peak]
    for d in [r.dynamics] + [t.dynamics for t in r.tracks]:
        if d is not None:
            vals += [d.loudness_range_lu, d.range_low_lufs, d.range_high_lufs, d.max_momentary_lufs, d.max_short_term_lufs,
                     float(d.st_blocks), float(d.st_blocks_gated)]
    return struct.pack(f"<{len(vals)}d", *vals)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--albums", type=int, default=64)
    ap.add_argument("--per-album", type=int, default=12)
    ap.add_argument("--seconds", type=float, default=60.0)
    ap.add_argument("--threads", default="1,2,4")
    ap.add_argument("--dynamics", default="0,1")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--distinct", type=int, default=4)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import torch  # noqa: F401

    import mp3rgain_amd as rg

    tmp = Path(tempfile.mkdtemp(prefix="rg_r128_albums_rate_"))
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
    res = {"albums": a.albums, "files_per_album": a.per_album, "seconds_per_file": a.seconds, "reps": a.reps, "true_peak": True,
           "cases": []}
    ok = True
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
            for dynamics in [bool(int(x)) for x in a.dynamics.split(",")]:
                kw = {"true_peak": True, "dynamics": dynamics}
                for threads in [int(x) for x in a.threads.split(",")]:
                    an.set_tuning(7, threads)
                    # warm-up of both forms, under fixed hops per lane: here the two must agree bit for bit
                    an.set_tuning_r128(1, FIXED_S)
                    one = an.analyze_albums_files_r128(albums, **kw)
                    each = [an.analyze_album_files_r128(f, **kw) for f in albums]
                    same = len(one) == len(each) and all(isinstance(g, rg.R128AlbumResult) and record(g) == record(w)
                                                         for g, w in zip(one, each))
                    an.set_tuning_r128(1, 0)
                    t_one, t_each, diff = [], [], 0.0
                    for _ in range(a.reps):  # the two forms in turn: what disturbs one disturbs the other
                        tm = {}
                        r_one = an.analyze_albums_files_r128(albums, timing=tm, **kw)
                        t_one.append(tm["c_call_seconds"])
                        total = 0.0
                        for f, g in zip(albums, r_one):
                            w = an.analyze_album_files_r128(f, timing=tm, **kw)
                            total += tm["c_call_seconds"]
                            diff = max(diff, abs(g.loudness_lufs - w.loudness_lufs))
                        t_each.append(total)
                    one_s, each_s = statistics.median(t_one), statistics.median(t_each)
                    case = {"format": label, "dynamics": dynamics, "loader_threads": threads, "files": n_files, "file_mb": file_bytes / 1e6,
                            "albums_call_ms": one_s * 1e3, "album_calls_ms": each_s * 1e3, "albums_call_ms_all": [t * 1e3 for t in t_one],
                            "album_calls_ms_all": [t * 1e3 for t in t_each],
                            "albums_call_stereo_samples_per_s": n_files * frames / one_s,
                            "album_calls_stereo_samples_per_s": n_files * frames / each_s, "speedup": each_s / one_s,
                            "same_results_at_fixed_hops_per_lane": same, "fixed_hops_per_lane": FIXED_S,
                            "max_album_loudness_difference_lu_at_default": diff}
                    ok = ok and same
                    res["cases"].append(case)
                    print(f"{label:9s} {'range' if dynamics else 'plain'} threads {threads}: one albums call {one_s * 1e3:8.1f} ms "
                          f"({case['albums_call_stereo_samples_per_s'] / 1e9:.2f} G stereo samples/s) | {a.albums} album calls "
                          f"{each_s * 1e3:8.1f} ms ({case['album_calls_stereo_samples_per_s'] / 1e9:.2f} G/s) | x{case['speedup']:.2f}"
                          f" | default S differs by {diff:.1e} LU{'' if same else ' | RESULTS DIFFER'}", flush=True)
                    if a.json:  # after every case: a run that is cut short leaves what it measured
                        Path(a.json).write_text(json.dumps(res, indent=1) + "\n")
        an.set_tuning(7, 0)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
