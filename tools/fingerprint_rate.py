#!/usr/bin/env python3
"""The rates of the duplicate finder's two stages (MI355X) and of their host twins: 1000 tracks of three minutes of 44.1 kHz
16-bit stereo filled on the device (rg_fingerprint_rate).

    tools/fingerprint_rate.py [--tracks 1000] [--seconds 180] [--host-tracks 16] [--threads 16] [--reps 5] [--warm-ms 400]
                              [--json profiles/fingerprint_rate.json]

After a warm-up (the launches repeated for `warm-ms` milliseconds: a fresh process runs slower for a while after a large
allocation), `reps` rounds in which the three launches alternate, HIP events around the launches alone: the fingerprint
kernels over all tracks, a read-only pass over the same planes, the match kernel over all pairs at the default options.  The
host legs run on `threads` threads over the first `host-tracks` tracks: the kernels' arithmetic (route 2), scaled to the track
count, and the serial match of their pairs, scaled to the pair count (tracks and pairs are independent and equally long); every
code and every pair record of those tracks must equal the kernels'.  Medians and the spread (min .. max) are reported.  The
match stage's work is counted in word operations, one XOR + popcount + add of a 32-bit word at one lag: pairs x lags x probes
x block, where every lag of every probe counts (all tracks are equally long, so a few lags at the ends lose probes: the count
is an upper bound by less than 1 %); its rate is set against the integer vector peak of 256 CUs x 4 SIMDs x 32 lanes x 2.4
GHz = 78.6 T lane-operations per second (the rate behind the 157.3 TFLOP/s of f32 fused multiply-adds), three of which (XOR,
popcount, add) a word operation needs at the least."""
import argparse
import ctypes as C
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

INT_PEAK_TOPS = 256 * 4 * 32 * 2.4e9 / 1e12  # lane-operations per second of the vector ALUs, in T


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tracks", type=int, default=1000)
    ap.add_argument("--seconds", type=float, default=180.0)
    ap.add_argument("--host-tracks", type=int, default=16)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warm-ms", type=float, default=400.0)
    ap.add_argument("--json", default=str(ROOT / "profiles" / "fingerprint_rate.json"))
    a = ap.parse_args()
    import torch  # noqa: F401  (torch first: one HIP runtime per process)

    import mp3rgain_amd as rg
    from mp3rgain_amd import _capi

    L = _capi.load()
    frames = int(44100 * a.seconds)
    n, hn = a.tracks, min(a.tracks, a.host_tracks)
    arrays = [(C.c_double * a.reps)() for _ in range(5)]
    bad = C.c_size_t()
    with rg.Analyzer(0) as an:
        an._check(L.rg_fingerprint_rate(an.handle, n, frames, None, hn, a.threads, a.reps, a.warm_ms, *arrays, C.byref(bad)))
    fp, read, match, host_fp, host_match = (list(x) for x in arrays)
    med = statistics.median
    codes = rg.fingerprint_codes(frames)
    pairs, host_pairs = n * (n - 1) // 2, hn * (hn - 1) // 2
    word_ops = pairs * (2 * _capi.FP_RADIUS + 1) * _capi.FP_PROBES * _capi.FP_BLOCK
    out = {"tool": "fingerprint_rate", "rate": 44100, "channels": 2, "format": "s16", "tracks": n, "seconds_per_track": a.seconds, "frames": frames,
           "codes_per_track": codes, "pairs": pairs, "reps": a.reps, "warm_ms": a.warm_ms, "mismatches": bad.value,
           "fingerprint": {"ms": med(fp), "ms_min": min(fp), "ms_max": max(fp), "ms_all": fp, "read_only_ms": med(read), "read_only_ms_all": read,
                           "read_only_over_fingerprint": med(read) / med(fp), "pcm_gb_per_s": 4.0 * n * frames / 1e9 / (med(fp) / 1e3),
                           "audio_seconds_per_s": n * a.seconds / (med(fp) / 1e3)},
           "match": {"ms": med(match), "ms_min": min(match), "ms_max": max(match), "ms_all": match, "word_ops": word_ops,
                     "tera_word_ops_per_s": word_ops / 1e12 / (med(match) / 1e3), "int_peak_tera_lane_ops_per_s": INT_PEAK_TOPS,
                     "share_of_int_peak_at_3_ops_per_word": 3.0 * word_ops / 1e12 / (med(match) / 1e3) / INT_PEAK_TOPS,
                     "pairs_per_s": pairs / (med(match) / 1e3)}}
    line = (f"fingerprint: {n} x {a.seconds:.0f} s: {med(fp):.1f} ms ({min(fp):.1f} .. {max(fp):.1f}); a read-only pass {med(read):.1f} ms = "
            f"{100 * med(read) / med(fp):.1f} % of it\nmatch: {pairs} pairs: {med(match):.1f} ms ({min(match):.1f} .. {max(match):.1f}); "
            f"{out['match']['tera_word_ops_per_s']:.2f} T word operations/s = {100 * out['match']['share_of_int_peak_at_3_ops_per_word']:.1f} % of the "
            f"integer vector peak at 3 operations per word")
    if hn:
        hf = med(host_fp) * n / hn
        out["fingerprint"].update(host_threads=a.threads, host_tracks=hn, host_ms=hf, host_ms_all_unscaled=host_fp, kernels_over_host=hf / med(fp))
        line += f"\nhost x{a.threads}: fingerprint {hf:.0f} ms ({hf / med(fp):.0f} x)"
        if host_pairs:
            hm = med(host_match) * pairs / host_pairs
            out["match"].update(host_threads=a.threads, host_pairs=host_pairs, host_ms=hm, host_ms_all_unscaled=host_match, kernel_over_host=hm / med(match))
            line += f", match {hm:.0f} ms ({hm / med(match):.0f} x)"
        line += f"; {bad.value} mismatching codes or pair records"
    print(line, flush=True)
    Path(a.json).parent.mkdir(parents=True, exist_ok=True)
    Path(a.json).write_text(json.dumps(out, indent=1) + "\n")
    if bad.value:
        raise SystemExit(f"{bad.value} host codes or pair records differ from the kernels'")


if __name__ == "__main__":
    main()
