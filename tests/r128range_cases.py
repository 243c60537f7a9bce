"""The signals of the loudness-range tests, in one place: long ones, because a short-term block is 3 s and the parity set of
tests/r128cases.py ends at 5 s.  tests/test_gpu_r128_range.py runs them through the library, tests/test_r128_range_cpu.py
checks on the checker alone that no block of them sits at a gate, and tools/r128_range_refcheck.py measures the float64
checker's own error on exactly these (tests/golden/r128_range_measured.json).  Not part of the product."""
import json
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent))
import r128cases  # noqa: E402
import r128range_ref as ref  # noqa: E402

# level steps in dB, one per segment; the segments of a signal are equally long
STEPS = [-6.0, -24.0, -12.0, -33.0, -9.0, -18.0, -40.0, -15.0]


def _stepped(kind, rate, frames, nch, seed, steps):
    chans = r128cases._f64(kind, rate, frames, nch, seed)
    seg = -(-frames // len(steps))
    env = np.repeat(10.0 ** (np.asarray(steps) / 20.0), seg)[:frames]
    return [c * env for c in chans]


def _quantise(chans, fmt):
    if fmt == "f32":
        return [c.astype(np.float32) for c in chans]
    if fmt == "s16":
        return [np.clip(np.round(c * 32767.0), -32768, 32767).astype(np.int16) for c in chans]
    if fmt == "s24":  # 24-bit samples in the upper bits of an int32, as the library's FLAC decoder delivers them
        return [(np.clip(np.round(c * 8388607.0), -8388608, 8388607).astype(np.int32) << 8).astype(np.int32) for c in chans]
    return [np.clip(np.round(c * 2147483647.0), -2147483648, 2147483647).astype(np.int32) for c in chans]


def range_cases():
    """[(id, kind, rate, frames, channels, format, seed)]; kind: "step-music", "step-noise", "loud_quiet", "noise" or
    "tech3342-caseN"."""
    cases = []
    for i, (rate, secs, fmt) in enumerate(((8000, 60, "s16"), (22050, 30, "f32"), (44100, 30, "s32"), (48000, 20, "f32"),
                                           (96000, 20, "s16"), (192000, 20, "f32"))):
        cases.append((f"step-music-{rate}-{fmt}", "step-music", rate, secs * rate + 11 * i, 2, fmt, 500 + i))
    cases.append(("step-noise-44100-s16", "step-noise", 44100, 20 * 44100 + 7, 2, "s16", 520))
    cases.append(("step-noise-48000-s32-mono", "step-noise", 48000, 25 * 48000, 1, "s32", 521))
    cases.append(("step-noise-11025-f32-mono", "step-noise", 11025, 40 * 11025 + 3, 1, "f32", 522))
    # more hops than one workgroup of the block kernel takes (1024): a track in several chunks
    cases.append(("step-noise-8000-s16-mono-long", "step-noise", 8000, 260 * 8000 + 77, 1, "s16", 523))
    cases.append(("loud_quiet-48000", "loud_quiet", 48000, 20 * 48000, 2, "f32", 530))
    cases.append(("loud_quiet-176400-s16", "loud_quiet", 176400, 8 * 176400, 2, "s16", 531))
    for name, _, _ in ref.TECH3342:
        cases.append((f"tech3342-{name}-48000", f"tech3342-{name}", 48000, 0, 2, "f32", 0))
    for rate, nch, fmt in ((48000, 2, "f32"), (44100, 1, "s16")):  # tracks around the shortest that has a short-term block
        h = r128cases.hop(rate)
        for name, frames in (("28hops", 28 * h), ("29hops", 29 * h), ("30hops-1", 30 * h - 1), ("30hops", 30 * h), ("31hops+1", 31 * h + 1)):
            cases.append((f"noise-{name}-{rate}-{fmt}", "noise", rate, frames, nch, fmt, 540))
    return cases


def make(kind, rate, frames, nch, fmt, seed):
    """-> list of `nch` arrays of dtype float32 / int16 / int32."""
    if kind.startswith("tech3342-"):
        segments = next(s for n, s, _ in ref.TECH3342 if kind.endswith(n))
        return _quantise(ref.tech3342_signal(rate, segments), fmt)
    if kind.startswith("step-"):
        return _quantise(_stepped(kind[5:], rate, frames, nch, seed, STEPS), fmt)
    return r128cases.make(kind, rate, frames, nch, fmt, seed)


def album_tracks():
    """[(channels, rate, container, kind)]: the album of the GPU tests, at four rates and in four sample formats.  The third
    track is about 45 dB under the first: wholly under the album's -20 LU gate, whole in itself (constant level).  The
    container says how the file tests write it: "wav" with tests/wavutil.py, "flac" with tests/flacenc.py (16 or 24 bit)."""
    loud = _quantise(_stepped("noise", 48000, 14 * 48000 + 5, 2, 600, [-3.0, -14.0, -8.0, -20.0]), "f32")
    mid = _quantise(_stepped("music", 44100, 12 * 44100, 2, 601, [-10.0, -16.0, -4.0]), "s16")
    quiet = _quantise([c * 10.0 ** (-48.0 / 20.0) for c in r128cases._f64("noise", 22050, 9 * 22050 + 1, 2, 602)], "s16")
    hires = _quantise(_stepped("noise", 96000, 8 * 96000, 1, 603, [-12.0, -6.0]), "s24")
    return [(loud, 48000, "wav", "f32"), (mid, 44100, "flac", "s16"), (quiet, 22050, "wav", "s16"), (hires, 96000, "flac", "s24")]


LARGE_ALBUM = (["step-noise-8000-s16-mono-long"] * 26 + ["step-music-8000-s16", "tech3342-case4-48000", "step-music-22050-f32",
                                                         "step-noise-11025-f32-mono"])


def large_album_ids():
    """The ids of range_cases() that make the large album of the GPU tests, in track order: 69029 short-term blocks, more
    than the size from which the library selects an album by wide passes, and a slice of 270 blocks for each of that form's
    256 workgroups (more than one 256-value iteration, full waves)."""
    return list(LARGE_ALBUM)


# Short-term block counts of an album's union at which the wide selection's partition changes shape: one block (255 of the
# 256 slices of the threshold's sum are empty), one fewer and one more than there are slices (slices of 1 with an empty last
# one; slices of 2, half of them empty), one fewer than a counting workgroup's least share of 4096 (one workgroup), and one
# more than twice that (two workgroups of 4097 and 4096).
EDGE_ALBUM_BLOCKS = (1, 255, 257, 4095, 8193)


def edge_album_tracks(n_blocks):
    """[(channels, rate)]: an album of two mono F32 tracks of stepped noise at 8 kHz, n_blocks // 2 short-term blocks in the
    first and the rest in the second (n_blocks = 1: the first has 29 hops and no block), each with a partial last hop.  The
    short tracks have two level steps instead of eight, so that a segment is longer than a block and the -20 LU gate has
    whole blocks to drop at every size."""
    rate, h = 8000, r128cases.hop(8000)
    out = []
    for k, blocks in enumerate((n_blocks // 2, n_blocks - n_blocks // 2)):
        frames = (blocks + ref.ST_HOPS - 1) * h + 3 + 2 * k
        steps = STEPS if blocks >= 1024 else [-6.0, -40.0]
        out.append((_quantise(_stepped("noise", rate, frames, 1, 700 + 10 * EDGE_ALBUM_BLOCKS.index(n_blocks) + k, steps), "f32"), rate))
    return out


def conformance_tracks():
    """[(case, rate, format, channels, expected LRA)]: the EBU Tech 3342 signals as the GPU conformance test runs them."""
    out = []
    for rate in (44100, 48000):
        for fmt in ("f32", "s16"):
            for name, segments, want in ref.TECH3342:
                out.append((name, rate, fmt, _quantise(ref.tech3342_signal(rate, segments), fmt), want))
    return out


def load_measured():
    return json.loads((Path(__file__).resolve().parent / "golden" / "r128_range_measured.json").read_text())
