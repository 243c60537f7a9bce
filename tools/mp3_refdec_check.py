#!/usr/bin/env python3
"""The MP3 decoders against the float64 reference decoder (oracle/mp3_refdec.py): streams, bar and recorded figures.

    tools/mp3_refdec_check.py                      host decoder: worst ratios per input kind, perturbation table
    tools/mp3_refdec_check.py --record             ... and write them to tests/golden/mp3_refdec_measured.json ("cpu")
    tools/mp3_refdec_check.py --device --record    the HIP decoder (every route of tuning key 6): the "device" section
    tools/mp3_refdec_check.py --out FILE           write there instead (other sections are carried over from the golden file)

tests/test_mp3_refdec.py and tests/test_gpu_mp3_refdec.py import the stream lists and the bar from here; they compute
every floor live and never read the recorded file.

The bar.  floor = reference in float32 - reference in float64: the error of the operation itself when every table
and intermediate is a float32, which is what both decoders work in.  A decoder is held to
    rms(dec - ref64) <= MARGIN * rms(floor)   and   max |dec - ref64| <= MARGIN * max |floor|
over the whole stream and over every block of 576 output samples of every channel; where a floor is exactly zero the
decoder's output must be exactly zero.  MARGIN = 4 covers what two float32 evaluations of the same sums may differ by
(summation order of the fast IMDCT / DCT against the matrix product, rounding of twiddle tables, fused multiply-adds);
a table entry wrong in its last digit is 10 to 2000 floors away (the perturbation table).
"""
import argparse
import functools
import json
import random
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
for p in (ROOT, ROOT / "oracle", ROOT / "tools", ROOT / "tests"):
    if str(p) not in sys.path:
        sys.path.insert(0, str(p))

import make_mp3_golden as M  # noqa: E402
import mp3_bitstream as B  # noqa: E402
import mp3_refdec as R  # noqa: E402

MARGIN = 4.0
BLOCK = 576
MEASURED = ROOT / "tests" / "golden" / "mp3_refdec_measured.json"

# ---- generated streams ---------------------------------------------------------------------------------------------
RATES = [44100, 48000, 32000, 22050, 24000, 16000, 11025, 12000, 8000]
MODES = [("mono", 3, 0), ("stereo", 0, 0), ("dual", 2, 0), ("joint0", 1, 0), ("joint_is", 1, 1), ("joint_ms", 1, 2), ("joint_is_ms", 1, 3)]
# block-type sequences that follow the window-switching state machine, the wrap-around included
SEQUENCES = [(0,), (0, 1, 2, 3), (0, 0, 1, 2, 2, 3), (1, 2, 2, 2, 3), (1, 2, 3, 0, 0), (0, 1, 2, 2, 2, 2, 3, 1, 2, 3)]
GAINS = [("low", (60, 110)), ("usual", (120, 200)), ("high", (200, 255))]
FRAMES = 24


def generated_cases():
    """63 streams: every rate row x every channel mode / mode_ext; block-type sequence, global_gain range, mixed blocks,
    sub-block gains, CRC, reservoir depth, linbits escapes and spikes walk through their values along the list."""
    cases = []
    k = 0
    for ri, rate in enumerate(RATES):
        lsf = rate < 32000
        table = B.BITRATES_V2 if lsf else B.BITRATES_V1
        for mi, (mname, mode, ext) in enumerate(MODES):
            gname, gg = GAINS[(ri + mi) % 3]
            seq = SEQUENCES[k % len(SEQUENCES)]
            opts = dict(block_types=seq, gg=gg, crc=(k % 4 == 1), sbg=(k % 2 == 0), mixed_prob=(0.0, 0.5, 1.0)[k % 3],
                        bitrate=table[-1] if k % 5 else table[-2], padding_every=(3 if k % 7 == 2 else 0),
                        stuffing=(k % 6 != 5))
            if k % 3 == 1:
                opts["huge_every"] = 7
                opts["lines"] = (60, 260)
            if k % 3 == 2:
                opts["spikes"] = (10, 128, 8000)
                opts["big"] = 3
                opts["lines"] = (200, 576)
            if ext & 1:
                opts["is_cut"] = (96, 140, 200)[k % 3]
            name = f"gen_{rate}_{mname}_{gname}_s{k % len(SEQUENCES)}"
            cases.append(dict(name=name, rate=rate, mode=mode, mode_ext=ext, seed=7000 + k, opts=opts,
                              illegal_lsf=bool(lsf and (ext & 1) and ri % 2 == 0)))
            k += 1
    return cases


def build_generated(case):
    """-> (stream bytes, reference Stream from the writer's own specs).  A stream that cannot be assembled is an error."""
    try:
        data, frames = M.build_case(case["name"], case["rate"], case["mode"], case["mode_ext"], FRAMES, case["seed"],
                                    return_specs=True, **case["opts"])
    except SystemExit as ex:
        raise RuntimeError(f"{case['name']}: {ex}") from None
    if case["illegal_lsf"]:
        # 13818-3 2.4.3.2: an intensity position of 2^slen - 1 means 'not intensity coded'.  Same widths, same bits.
        rng = random.Random(case["seed"] + 5)
        for f in frames:
            for chans in f.granules:
                g = chans[1]
                widths = B.scalefactor_widths(g, True, True, 0)
                g.scalefacs = [((1 << w) - 1 if (w and rng.random() < 0.3) else v) for v, w in zip(g.scalefacs, widths)]
        data = B.write_stream(frames, case["rate"], random.Random(case["seed"] + 1), stuffing=case["opts"]["stuffing"])
    return data, R.from_specs(frames, case["rate"])


ENCODED = [("enc_v1_44k_joint_128", 44100, 128, 3.0, 41), ("enc_v2_22k_joint_64", 22050, 64, 4.0, 42), ("enc_v25_11k_joint_32", 11025, 32, 6.0, 43)]


def build_encoded(name, rate, bitrate, seconds, seed):
    """A few seconds of the synthetic piece of tools/make_mp3_dense.py through oracle/mp3_encoder.py, window switching and
    mid/side on; narrowed towards the centre so that the encoder does choose mid/side frames."""
    import make_mp3_dense as MD
    import mp3_encoder as E

    pcm = MD.piece(rate, seconds, 2, seed)
    mid = 0.5 * (pcm[0] + pcm[1])
    pcm = np.stack([mid + 0.35 * (pcm[0] - mid), mid + 0.35 * (pcm[1] - mid)])
    return E.encode(pcm, rate, bitrate, seed=seed, allow_ms=True, allow_short=True)


def reference_from_bytes(data):
    """Streams that exist only as bytes: stage A by the library's parser (held to the writer by tests/test_mp3dec.py)."""
    from mp3rgain_amd import mp3dec

    return R.from_units(*mp3dec.parse_units(data))


# ---- the bar -------------------------------------------------------------------------------------------------------
def _rms(x, axis=None):
    return np.sqrt((x * x).mean(axis=axis))


def measure(dec, ref64, ref32):
    """Ratios of the decoder's error to the float32 floor -> dict; `bad` lists what misses the bar, in words."""
    assert dec.shape == ref64.shape == ref32.shape, (dec.shape, ref64.shape, ref32.shape)
    assert dec.shape[1] % BLOCK == 0
    d = dec.astype(np.float64)
    e = d - ref64
    f = ref32.astype(np.float64) - ref64
    bad = []
    out = dict(peak=float(np.abs(ref64).max()), zero_floor_blocks=0)
    if not np.isfinite(d).all():
        bad.append("decoder output is not finite")
    if f.any():
        out["stream_rms"] = float(_rms(e) / _rms(f))
        out["stream_max"] = float(np.abs(e).max() / np.abs(f).max())
    else:
        out["stream_rms"] = out["stream_max"] = 0.0
    eb = e.reshape(e.shape[0], -1, BLOCK)
    fb = f.reshape(f.shape[0], -1, BLOCK)
    fr, fm = _rms(fb, axis=2), np.abs(fb).max(axis=2)
    er, em = _rms(eb, axis=2), np.abs(eb).max(axis=2)
    zero = fm == 0
    out["zero_floor_blocks"] = int(zero.sum())
    db = d.reshape(eb.shape)
    for c, b in np.argwhere(zero):
        if db[c, b].any():
            bad.append(f"channel {c} block {b}: the floor is zero, the decoder's output is not")
    with np.errstate(divide="ignore", invalid="ignore"):
        rr = np.where(zero, 0.0, er / fr)
        rm = np.where(zero, 0.0, em / fm)
    out["block_rms"] = float(rr.max())
    out["block_max"] = float(rm.max())
    out["worst_block"] = [int(x) for x in np.unravel_index(int(np.argmax(rm)), rm.shape)]
    for key in ("stream_rms", "stream_max", "block_rms", "block_max"):
        if not out[key] <= MARGIN:
            bad.append(f"{key} = {out[key]:.2f} floors (bar {MARGIN:g})")
    out["bad"] = bad
    return out


def name_stage(stream, dec, ref64):
    """For a finding: the first block beyond the bar and the content of that granule (the reference's intermediates tell
    which stage carries energy there)."""
    stages = {}
    R.decode(stream, np.float64, stages=stages)
    e = np.abs(dec.astype(np.float64) - ref64).reshape(dec.shape[0], -1, BLOCK).max(axis=2)
    c, b = np.unravel_index(int(np.argmax(e)), e.shape)
    g = stream.granules[b].chans[c]
    return (f"channel {c} granule {b}: block_type {g.block_type} mixed {g.mixed} gg {g.global_gain} sbg {g.subblock_gain} "
            f"|is|max {int(np.abs(g.values).max())} ms {stream.granules[b].ms} is {stream.granules[b].intensity}; "
            f"|xr|max {np.abs(stages['stereo'][c, b]).max():.3g} |subband|max {np.abs(stages['subband'][c, 18 * b:18 * b + 18]).max():.3g}")


def worst(rows):
    keys = ("stream_rms", "stream_max", "block_rms", "block_max")
    out = {k: max(r[k] for r in rows) for k in keys}
    out["streams"] = len(rows)
    out["zero_floor_blocks"] = sum(r["zero_floor_blocks"] for r in rows)
    out["worst_block_stream"] = max(rows, key=lambda r: r["block_max"])["name"]
    return {k: (round(v, 3) if isinstance(v, float) else v) for k, v in out.items()}


# which stream shows each deliberate error (golden ones, so that the ffmpeg figures can be given next to the bar's)
PERTURB_STREAMS = {
    "window_tap": "v1_44k_mono_crc_reservoir", "centre_tap": "v1_44k_mono_crc_reservoir", "exponent": "v1_44k_mono_crc_reservoir",
    "imdct_window": "v1_44k_mono_crc_reservoir", "alias": "v1_44k_mono_crc_reservoir", "synthesis_matrix": "v1_44k_mono_crc_reservoir",
    "ms_scale": "v1_48k_ms_blocktypes", "short_window": "v1_48k_ms_blocktypes", "subblock_gain": "v1_48k_ms_blocktypes",
    "intensity_ratio": "v1_32k_intensity",
}


def input_names():
    """(kind, name) of everything the decoders are held to: the golden streams and the reference project's damaged
    test_stereo.mp3, the generated streams, the encoder-made ones."""
    import mp3gold

    return ([("golden", p.stem) for p in mp3gold.STREAMS + [mp3gold.FIX / "test_stereo.mp3"]]
            + [("generated", c["name"]) for c in generated_cases()] + [("encoded", e[0]) for e in ENCODED])


@functools.lru_cache(maxsize=None)
def load_input(kind, name):
    """-> (stream bytes, reference Stream)"""
    import mp3gold

    if kind == "golden":
        path = next(p for p in mp3gold.STREAMS + [mp3gold.FIX / "test_stereo.mp3"] if p.stem == name)
        data = path.read_bytes()
        return data, reference_from_bytes(data)
    if kind == "generated":
        return build_generated(next(c for c in generated_cases() if c["name"] == name))
    data = build_encoded(*next(e for e in ENCODED if e[0] == name))
    return data, reference_from_bytes(data)


@functools.lru_cache(maxsize=None)
def references(kind, name):
    """-> (float64 reference PCM, the same code in float32)"""
    _, st = load_input(kind, name)
    return R.decode(st, np.float64), R.decode(st, np.float32)


def all_inputs():
    for kind, name in input_names():
        data, st = load_input(kind, name)
        yield kind, name, data, st


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--record", action="store_true")
    ap.add_argument("--device", action="store_true")
    ap.add_argument("--out", default=str(MEASURED))
    args = ap.parse_args()
    import mp3gold
    from mp3rgain_amd import mp3dec

    t0 = time.time()
    an = None
    if args.device:
        import torch  # noqa: F401

        import mp3rgain_amd as rg

        an = rg.Analyzer(0)
    rows = {}
    failures = 0
    for kind, name, data, st in all_inputs():
        r64, r32 = references(kind, name)
        decs = []
        if an is None:
            decs.append(("host", mp3dec.decode(data)[0]))
        else:
            for route in (1, 2, 3):
                an.set_tuning(6, route)
                decs.append((f"route{route}", an.decode_mp3_device(data)[0]))
        for tag, dec in decs:
            m = measure(dec, r64, r32)
            m["name"] = name
            rows.setdefault((tag, kind), []).append(m)
            if m["bad"]:
                failures += 1
                print("BEYOND THE BAR", tag, name, m["bad"], name_stage(st, dec, r64))
    if an is not None:
        an.close()
    section = {}
    for (tag, kind), rs in sorted(rows.items()):
        section.setdefault(tag, {})[kind] = worst(rs)
        print(tag, kind, section[tag][kind])
    result = {"margin": MARGIN, "block": BLOCK}
    if Path(MEASURED).exists():
        result.update(json.loads(Path(MEASURED).read_text()))
    if an is None:
        result["cpu"] = section["host"]
        table = {}
        for pert, sname in PERTURB_STREAMS.items():
            p = mp3gold.GOLD / f"{sname}.mp3"
            data = p.read_bytes()
            st = reference_from_bytes(data)
            dec, info = mp3dec.decode(data)
            mut = R.decode(st, np.float64, perturb=pert)
            m = measure(dec, mut, R.decode(st, np.float32) - R.decode(st, np.float64) + mut)
            mx, rms, _, _ = mp3gold.compare_with_gold(mut, info.info_frame, mp3gold.load_gold(p))
            table[pert] = dict(stream=sname, stream_rms=round(m["stream_rms"], 1), stream_max=round(m["stream_max"], 1),
                               block_max=round(m["block_max"], 1), ffmpeg_max_steps=round(mx, 3), ffmpeg_rms_steps=round(rms, 3),
                               passes_ffmpeg_bar=bool(mx <= mp3gold.MAX_STEPS and rms <= mp3gold.RMS_STEPS))
            print("perturbation", pert, table[pert])
        result["perturbations"] = table
    else:
        result["device"] = {k: v for k, v in section.items()}
    result["seconds"] = dict(result.get("seconds", {}), **{"device" if args.device else "cpu": round(time.time() - t0, 1)})
    if args.record:
        Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        Path(args.out).write_text(json.dumps(result, indent=1, sort_keys=True) + "\n")
        print("wrote", args.out)
    print("%.1f s, %d beyond the bar" % (time.time() - t0, failures))
    return 1 if failures else 0


if __name__ == "__main__":
    sys.exit(main())
