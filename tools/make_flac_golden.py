#!/usr/bin/env python3
"""FLAC fixtures for the decoder tests, and the evidence that they are conformant.

Writes tests/golden/flac/<name>.flac (tests/flacenc.py, covering bit depths 8-24, mono / stereo / 6 channels, every
ReplayGain rate and 192 kHz, every channel assignment, variable blocking, LPC up to order 32) plus the damaged variants of
flacenc.damaged_variants, and tests/golden/flac/expected.json: per stream the sha256 of the PCM it must decode to (the
encoder's input, int32 little-endian, planar [channels][samples]), its length and its dropped-frame count.

Every undamaged stream is also decoded by an independent decoder: ffmpeg's FLAC decoder inside the headless Chromium of the
`kaleido` wheel (tools/ffmpeg_golden.py drives its Web Audio decodeAudioData).  Its float output maps back to integers
exactly: up to 16 bits ffmpeg hands Chromium s16 (<< 16 - bps), which it turns into float as x / 32767 above zero and
x / 32768 below; above 16 bits s32 (<< 32 - bps), turned into x / 2^31.  The JSON records whether that PCM equals the
encoder's input ("ffmpeg_equal").  kaleido does not travel with the repository: only the outputs are committed.

    tools/make_flac_golden.py [out_dir]
"""
import hashlib
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT / "tools"))
import flacenc as fe  # noqa: E402

O = fe.Options

# (name, rate, channels, bps, samples, options)
STREAMS = [
    ("s8_mono_22k", 22050, 1, 8, 6000, O(subframe="auto")),
    ("s12_stereo_16k_ls", 16000, 2, 12, 6000, O(stereo="left_side")),
    ("s16_stereo_44k_alt", 44100, 2, 16, 12000, O(stereo="alternate", block_size=1152)),
    ("s20_stereo_88k_rs", 88200, 2, 20, 8000, O(stereo="right_side")),
    ("s24_stereo_96k_ms_rice2", 96000, 2, 24, 8000, O(stereo="mid_side", rice2=True, escape_every=3)),
    ("s16_6ch_48k", 48000, 6, 16, 5000, O(subframe="fixed", order=2)),
    ("s16_mono_64k_khz", 64000, 1, 16, 6000, O()),
    ("s16_mono_32k", 32000, 1, 16, 6000, O(order=12, precision=15, shift=13)),
    ("s16_mono_24k_verbatim", 24000, 1, 16, 3000, O(subframe="verbatim")),
    ("s16_mono_12k_khz", 12000, 1, 16, 6000, O(block_size=576)),
    ("s16_mono_11k_hz", 11025, 1, 16, 6000, O(bs_code="explicit16", block_size=1000)),
    ("s16_mono_8k", 8000, 1, 16, 6000, O(bs_code="explicit8", block_size=192)),
    ("s16_stereo_44k_variable", 44100, 2, 16, 9000, O(variable=True, blocks=[4096, 100, 1, 2000, 2803])),
    ("s16_stereo_48k_lpc32", 48000, 2, 16, 8000, O(order=32, precision=15, shift=13, partition_order=4)),
    ("s16_stereo_192k", 192000, 2, 16, 8000, O()),
]


def pcm_sha(pcm) -> str:
    return hashlib.sha256(np.ascontiguousarray(np.asarray(pcm, dtype="<i4")).tobytes()).hexdigest()


def from_ffmpeg(f32: np.ndarray, bps: int) -> np.ndarray:
    p = f32.astype(np.float64)
    if bps <= 16:
        q = np.round(np.where(p > 0, p * 32767.0, p * 32768.0)).astype(np.int64)
        return q >> (16 - bps)
    return np.round(p * 2.0 ** (bps - 1)).astype(np.int64)


def main():
    out = Path(sys.argv[1]) if len(sys.argv) > 1 else ROOT / "tests" / "golden" / "flac"
    out.mkdir(parents=True, exist_ok=True)
    import ffmpeg_golden

    record = {}
    for name, rate, ch, bps, n, opt in STREAMS:
        import zlib

        pcm = fe.test_pcm(np.random.default_rng(zlib.crc32(name.encode())), ch, n, bps)
        data = fe.encode(pcm, rate, bps, opt)
        (out / f"{name}.flac").write_bytes(data)
        dec, info = ffmpeg_golden.decode(data, rate)
        got = from_ffmpeg(dec, bps)
        equal = bool(got.shape == pcm.shape and np.array_equal(got, pcm))
        record[name] = {"rate": rate, "channels": ch, "bps": bps, "samples": n, "dropped": 0, "sha256": pcm_sha(pcm),
                        "ffmpeg_equal": equal, "ffmpeg_ua": info["ua"]}
        print(name, len(data), "bytes, ffmpeg equal:", equal)
    for name, data, want, dropped in fe.damaged_variants():
        (out / f"damaged_{name}.flac").write_bytes(data)
        record[f"damaged_{name}"] = {"rate": 44100, "channels": int(want.shape[0]), "bps": 16, "samples": int(want.shape[1]),
                                     "dropped": dropped, "sha256": pcm_sha(want), "ffmpeg_equal": None}
        print("damaged", name, len(data), "bytes")
    (out / "expected.json").write_text(json.dumps(record, indent=1, sort_keys=True) + "\n")


if __name__ == "__main__":
    main()
