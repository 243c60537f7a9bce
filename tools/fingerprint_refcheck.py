#!/usr/bin/env python3
"""The float64 reference of the fingerprint (tests/fingerprint_cases.py, numpy.fft.rfft) over the shared case list, against
the host routes (rg_fingerprint_arena routes 0 and 2; never the kernels against themselves), and the match threshold.

    python tools/fingerprint_refcheck.py            print the figures and compare with tests/golden/fingerprint_measured.json
    python tools/fingerprint_refcheck.py --record   write that file

Recorded:
 1. band energies: the largest error of E from routes 0 and 2 against the reference over the shared cases, relative to the
    frame's largest band energy (fingerprint_cases.band_error);
 2. flipped bits: the share of code bits where route 2 differs from the reference, over the shared cases and the threshold
    material below, and the largest reference margin |d| / (the two frames' band energy) among the differing bits;
 3. the threshold: SEEDS seeds of tests/ancestry_cases.music of SECONDS s, each with degraded copies (short_cut coding at zero
    shares 0.5 and 0.8, white noise at 20 dB SNR, -6 dB, 16-bit quantisation, trims of 137, 256 and 1105 samples, 1 s of
    silence in front, and two combinations); codes by route 2, the match by the serial host twin at the default block, probes
    and radius: the largest best-lag BER over same-recording pairs, the smallest over unrelated pairs (different seeds), the
    default max_ber_permille = their rounded midpoint, and whether every same-recording pair's lag is the expected one.
The first REAL_STREAMS seeds also get a real oracle/mp3_encoder.encode stream (128 and 64 kb/s in turn) decoded by the library's
own decoder.  No GPU."""
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT / "oracle"))
sys.path.insert(0, str(ROOT))

import numpy as np  # noqa: E402

import fingerprint_cases as fc  # noqa: E402

SEEDS = 20
SECONDS = 6.5
RATE = 44100
DELAY = 1057  # of short_cut's decoder and of a decoded stream
REAL_STREAMS = 4  # seeds that also get a real stream (128 and 64 kb/s in turn)


def material(seed):
    """-> [(name, plane of the track, how many samples later than in the original the common audio lies)]"""
    import ancestry_cases as ac

    n = int(SECONDS * RATE)
    x = ac.music(n, 1000 + seed)
    rng = np.random.default_rng(5000 + seed)
    cut5 = ac.short_cut(x, 0.5)[0]
    cut8 = ac.short_cut(x, 0.8)[0]
    noisy = x + rng.standard_normal(n) * np.sqrt(np.mean(x * x) / 100.0)
    f32 = lambda y: (y / 32768.0).astype(np.float32)  # noqa: E731
    silence = np.zeros(RATE)
    real = []
    if seed < REAL_STREAMS:  # a real stream of the project's encoder, decoded by the library's own decoder
        import mp3_encoder as E
        from mp3rgain_amd import _capi, mp3dec

        _capi.load()
        kbps = (128, 64)[seed % 2]
        dec, info = mp3dec.decode(E.encode((x / 32768.0)[None, :], RATE, kbps, seed=seed, allow_ms=False, allow_short=True))
        assert info.skipped_frames == 0
        real = [(f"mp3_{kbps}k", np.ascontiguousarray(dec[0], dtype=np.float32), DELAY)]
    return real + [
        ("original", f32(x), 0),
        ("cut0.5", f32(cut5), DELAY),
        ("cut0.8", f32(cut8), DELAY),
        ("noise20dB", f32(noisy), 0),
        ("gain-6dB", f32(x * 10 ** (-6 / 20)), 0),
        ("s16", ac.to_s16(x), 0),
        ("trim137", f32(x[137:]), -137),
        ("trim256", f32(x[256:]), -256),
        ("trim1105", f32(x[1105:]), -1105),
        ("silence1s", f32(np.concatenate([silence, x])), RATE),
        ("cut0.8+gain+trim1105", f32(cut8[1105:] * 10 ** (-6 / 20)), DELAY - 1105),
        ("cut0.5+noise+silence+trim137+s16", ac.to_s16(np.concatenate([silence, (cut5 + rng.standard_normal(len(cut5)) *
                                                                               np.sqrt(np.mean(x * x) / 100.0))[137:]])), RATE + DELAY - 137),
    ]


def fingerprints(tracks):
    """Route 2 of the (name, plane, shift) tracks -> (their code arrays, flipped bits against the reference, bits, worst margin)"""
    import mp3rgain_amd as rg

    cs = [fc.Case(name, [plane], RATE) for name, plane, _ in tracks]
    arena, descs = fc.pack(cs)
    recs, codes, _ = rg.fingerprint_arena(None, 2, descs, arena, bands=False)
    out, flips, bits, worst = [], 0, 0, 0.0
    for c, r in zip(cs, recs):
        mine = codes[r.codes_at:r.codes_at + r.codes]
        f, m = fc.flipped(mine, fc.reference(c))
        flips, bits, worst = flips + f, bits + 32 * len(mine), max(worst, m)
        out.append(mine)
    return out, flips, bits, worst


def shared_cases():
    import mp3rgain_amd as rg

    cs = fc.cases()
    arena, descs = fc.pack(cs)
    err, flips, bits, worst = {0: 0.0, 2: 0.0}, 0, 0, 0.0
    for route in (0, 2):
        recs, codes, bands = rg.fingerprint_arena(None, route, descs, arena)
        for c, r in zip(cs, recs):
            ref = fc.reference(c)
            assert (r.fp_frames, r.nonfinite_frames) == (ref.frames, ref.nonfinite), c.name
            err[route] = max(err[route], fc.band_error(bands[r.frames_at:r.frames_at + r.fp_frames].astype(np.float64), ref.bands))
            if route == 2:
                f, m = fc.flipped(codes[r.codes_at:r.codes_at + r.codes], ref)
                flips, bits, worst = flips + f, bits + 32 * int(r.codes), max(worst, m)
    return err, flips, bits, worst


def measure():
    import mp3rgain_amd as rg

    err, flips, bits, worst = shared_cases()
    print("shared cases: band error", err, "flipped", flips, "of", bits, flush=True)
    t0 = time.time()
    sets = []
    for seed in range(SEEDS):
        tracks = material(seed)
        codes, f, b, m = fingerprints(tracks)
        flips, bits, worst = flips + f, bits + b, max(worst, m)
        sets.append((tracks, codes))
        print(f"seed {seed}: {len(tracks)} tracks, {time.time() - t0:.0f} s", flush=True)
    same_max, wrong_lags, rows = 0.0, [], {}
    for seed, (tracks, codes) in enumerate(sets):  # every pair of one seed is the same recording
        rec = rg.fingerprint_match_codes(None, 0, codes, [RATE] * len(codes))
        k = 0
        for i in range(len(tracks)):
            for j in range(i + 1, len(tracks)):
                r = rec[k]
                k += 1
                assert r["flags"] & 1, (seed, tracks[i][0], tracks[j][0])
                ber = int(r["errors"]) / int(r["bits"])
                # the lag of the longer against the shorter, in codes: the nearest to the shift in samples / 512
                probe_j = bool(r["flags"] & 8)
                shift = (tracks[i][2] - tracks[j][2]) if probe_j else (tracks[j][2] - tracks[i][2])
                if abs(int(r["lag"]) - shift / fc.H) > 0.5 + 1e-9:
                    wrong_lags.append((seed, tracks[i][0], tracks[j][0], int(r["lag"]), shift / fc.H))
                name = f"{tracks[i][0]} ~ {tracks[j][0]}"
                rows[name] = max(rows.get(name, 0.0), round(ber, 4))
                same_max = max(same_max, ber)
    # unrelated: the originals and two degraded copies of every seed, pairs of different seeds only
    pick = [(s, t) for s in range(SEEDS) for t in range(len(sets[s][0])) if sets[s][0][t][0] in
            ("original", "cut0.8", "cut0.5+noise+silence+trim137+s16", "mp3_128k", "mp3_64k")]
    rec = rg.fingerprint_match_codes(None, 0, [sets[s][1][t] for s, t in pick], [RATE] * len(pick))
    other_min, k = 1.0, 0
    for i in range(len(pick)):
        for j in range(i + 1, len(pick)):
            r = rec[k]
            k += 1
            if pick[i][0] != pick[j][0]:
                other_min = min(other_min, int(r["errors"]) / int(r["bits"]))
    m = dict(band_error_route0=err[0], band_error_route2=err[2], flipped_bits=flips, code_bits=bits, flipped_share=flips / bits,
             flipped_margin_max=worst, seeds=SEEDS, seconds=SECONDS, same_recording_max_ber=round(same_max, 4),
             unrelated_min_ber=round(other_min, 4), overlap=bool(same_max >= other_min), wrong_lags=wrong_lags,
             max_ber_permille=int(round(1000 * (same_max + other_min) / 2)), real_encoder_streams=REAL_STREAMS,
             same_recording_ber_by_pair=rows)
    return m


def main():
    m = measure()
    head = {k: v for k, v in m.items() if k != "same_recording_ber_by_pair"}
    print(json.dumps(head, indent=1))
    if "--record" in sys.argv:
        fc.MEASURED.write_text(json.dumps(m, indent=1, sort_keys=True) + "\n")
        return 0
    old = json.loads(fc.MEASURED.read_text())
    same = all(old[k] == v for k, v in head.items())
    print("the recorded file", "agrees" if same else "DIFFERS")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
