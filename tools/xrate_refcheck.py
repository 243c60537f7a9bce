#!/usr/bin/env python3
"""The float64 reference of the rational resampler (tests/resample_cases.py) over the shared case list, against the host
routes (rg_resample_arena routes 0 and 2; never the kernels against themselves), and the cross-rate match threshold.

    python tools/xrate_refcheck.py            print the figures and compare with tests/golden/xrate_measured.json
    python tools/xrate_refcheck.py --record   write that file

Recorded:
 1. y: the largest error of routes 0 and 2 against the reference over the shared cases, relative to the track's largest |y|,
    per rate (resample_cases.y_error);
 2. flipped bits: the share of code bits where route 2 of rg_xrate_fingerprint_arena differs from route 0, over the threshold
    material below;
 3. the threshold: the SEEDS seeds of tools/fingerprint_refcheck.py's material (each seed's original and degraded copies at
    44100 Hz) with copies of the original resampled to 48000 and 96000 Hz (an FFT resampler in numpy, not the one under test),
    and PIECES continuous-time pieces rendered at six rates, one rendering again delayed by 133.7 ms; codes by route 2, the
    match by the serial host twin at the cross-rate call's default block, probes and radius: the largest best-lag BER over
    same-recording pairs (pairs of one seed or piece), the smallest over unrelated pairs, the default max_ber_permille = their
    rounded midpoint, and whether every same-recording pair's lag is one of the two whole codes next to the true shift
    (and how many are not the nearer of the two).
No GPU."""
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT / "oracle"))
sys.path.insert(0, str(ROOT / "tools"))
sys.path.insert(0, str(ROOT))

import numpy as np  # noqa: E402

import fingerprint_refcheck as fr  # noqa: E402
import resample_cases as rc  # noqa: E402

SEEDS = fr.SEEDS
PIECES = 3
OTHER_RATES = (48000, 96000)


def fft_resample(x, rate_in, rate_out):
    """x (float64) at rate_in -> at rate_out, band-limited, by zero-padding its spectrum."""
    n = len(x)
    m = int(round(n * rate_out / rate_in))
    X = np.fft.rfft(x)
    Y = np.zeros(m // 2 + 1, dtype=complex)
    k = min(len(X), len(Y))
    Y[:k] = X[:k]
    return np.fft.irfft(Y, m) * (m / n)


def seed_tracks(seed):
    """-> [(name, rate, plane, seconds later than in the original the common audio lies, which recording)]"""
    out = []
    for name, plane, shift in fr.material(seed):
        out.append((name, fr.RATE, plane, shift / fr.RATE, seed))
        if name == "original":
            x = plane.astype(np.float64)
            for rate in OTHER_RATES:
                out.append((f"original@{rate}", rate, fft_resample(x, fr.RATE, rate).astype(np.float32), 0.0, seed))
    return out


def piece_tracks(k):
    out = [(f"piece@{r}", r, rc.piece(r, seed=10 + k), 0.0, 1000 + k) for r in rc.PIECE_RATES]
    out.append(("piece@48000+133.7ms", 48000, rc.piece(48000, delay=rc.DELAY_SECONDS, seed=10 + k, noise_seed=77), rc.DELAY_SECONDS, 1000 + k))
    return out


def shared_cases():
    import mp3rgain_amd as rg

    cs = rc.cases()
    arena, descs = rc.pack(cs)
    err = {0: {}, 2: {}}
    for route in (0, 2):
        recs, y = rg.resample_arena(None, route, descs, arena)
        for c, r in zip(cs, recs):
            ref = rc.reference(c)
            assert len(ref) == r.resampled, c.name
            e = rc.y_error(y[r.y_at:r.y_at + r.resampled], ref)
            err[route][str(c.sample_rate)] = max(err[route].get(str(c.sample_rate), 0.0), e)
    return err


def measure():
    err = shared_cases()
    print("shared cases: y error", err, flush=True)
    t0 = time.time()
    sets = []
    flips = bits = 0
    for s in range(SEEDS + PIECES):
        tracks = seed_tracks(s) if s < SEEDS else piece_tracks(s - SEEDS)
        codes, _ = rc.xrate_codes(tracks, 2)
        ref, _ = rc.xrate_codes(tracks, 0)
        flips += sum(int(rc.fc.popcount(a ^ b).sum()) for a, b in zip(codes, ref))
        bits += sum(32 * len(a) for a in codes)
        sets.append((tracks, codes))
        print(f"set {s}: {len(tracks)} tracks, {time.time() - t0:.0f} s", flush=True)
    same_max, wrong_lags, rows, off_nearest = 0.0, [], {}, 0
    for s, (tracks, codes) in enumerate(sets):  # every pair of one set is the same recording
        rec = rc.match(codes)
        k = 0
        for i in range(len(tracks)):
            for j in range(i + 1, len(tracks)):
                r = rec[k]
                k += 1
                if tracks[i][1] == tracks[j][1] and s < SEEDS:
                    continue  # a same-rate pair of the seeds' material: the same-rate finder's ground
                assert r["flags"] & 1, (s, tracks[i][0], tracks[j][0])
                ber = int(r["errors"]) / int(r["bits"])
                want = rc.expected_lag(int(r["flags"]), tracks[i][3], tracks[j][3])
                # the expected lag: one of the two whole codes next to the true shift.  (The nearest alone is not a fair demand
                # here: the coded copies' 1057 samples of delay are 0.516 codes of 46.4 ms, 0.016 from the midpoint, where both
                # neighbours overlap the frames almost equally and the coding decides; those pairs are counted.)
                if abs(int(r["lag"]) - want) > 0.5 + 1e-9:
                    off_nearest += 1
                if abs(int(r["lag"]) - want) >= 1.0:
                    wrong_lags.append((s, tracks[i][0], tracks[j][0], int(r["lag"]), round(want, 3)))
                name = f"{tracks[i][0]} ~ {tracks[j][0]}"
                rows[name] = max(rows.get(name, 0.0), round(ber, 4))
                same_max = max(same_max, ber)
    # unrelated: some tracks of every set, pairs of different sets only
    keep = ("original", "original@48000", "original@96000", "cut0.8", "cut0.5+noise+silence+trim137+s16", "mp3_128k", "mp3_64k", "piece@44100",
            "piece@8000", "piece@96000", "piece@48000+133.7ms")
    pick = [(s, t) for s in range(len(sets)) for t in range(len(sets[s][0])) if sets[s][0][t][0] in keep]
    rec = rc.match([sets[s][1][t] for s, t in pick])
    other_min, k = 1.0, 0
    for i in range(len(pick)):
        for j in range(i + 1, len(pick)):
            r = rec[k]
            k += 1
            if pick[i][0] != pick[j][0] and r["flags"] & 1:
                other_min = min(other_min, int(r["errors"]) / int(r["bits"]))
    return dict(y_error_route0=err[0], y_error_route2=err[2], flipped_bits=flips, code_bits=bits, flipped_share=flips / bits, seeds=SEEDS, pieces=PIECES,
                same_recording_max_ber=round(same_max, 4), unrelated_min_ber=round(other_min, 4), overlap=bool(same_max >= other_min),
                wrong_lags=wrong_lags, lags_not_the_nearest=off_nearest, max_ber_permille=int(round(1000 * (round(same_max, 4) + round(other_min, 4)) / 2)), block=rc._capi.XR_BLOCK,
                probes=rc._capi.XR_PROBES, radius=rc._capi.XR_RADIUS, same_recording_ber_by_pair=rows)


def main():
    m = measure()
    head = {k: v for k, v in m.items() if k != "same_recording_ber_by_pair"}
    print(json.dumps(head, indent=1))
    worst = sorted(m["same_recording_ber_by_pair"].items(), key=lambda kv: -kv[1])[:8]
    print("largest same-recording rates:", worst)
    if "--record" in sys.argv:
        rc.MEASURED.write_text(json.dumps(m, indent=1, sort_keys=True) + "\n")
        return 0
    old = json.loads(rc.MEASURED.read_text())
    same = all(old[k] == v for k, v in head.items())
    print("the recorded file", "agrees" if same else "DIFFERS")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
