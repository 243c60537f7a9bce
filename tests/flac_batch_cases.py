"""The streams of the batched FLAC decode tests (tests/test_flac_batch_cases_cpu.py, tests/test_gpu_flac_batch.py).  Not
part of the product; pure Python on tests/flacenc.py, no library.

A case is a Case: the encoded stream, the PCM it must decode to -- always the ENCODER'S INPUT, with the blocks of frames
that were damaged on purpose taken out -- and the number of frames a decoder must drop.  `planes(case)` is that PCM in the
analysis arena's format, by the rule the RIFF/WAVE twin of a FLAC file follows (tests/test_gpu_flac.py: _planar): up to 16
bits per sample int16 (x << 16 - bps), otherwise int32 (x << 32 - bps).

Only the fuzz variants (fuzz_streams) have no derivable answer: the tests take the host decoder's output for them.

Every list is built once per process (encoding all of them takes a few seconds of host time)."""
import functools
import sys
import zlib
from collections import namedtuple
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent))
if str(Path(__file__).resolve().parent.parent) not in sys.path:  # test_flacdec (MATRIX) imports the package
    sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import flacenc as fe  # noqa: E402

O = fe.Options
Case = namedtuple("Case", "name data pcm bps rate channels dropped")


def planes(case):
    """The expected planes of a case in the arena's format."""
    return to_planes(case.pcm, case.bps)


def to_planes(pcm, bps):
    if bps <= 16:
        return [(np.asarray(c, dtype=np.int64) << (16 - bps)).astype(np.int16) for c in pcm]
    return [(np.asarray(c, dtype=np.int64) << (32 - bps)).astype(np.int32) for c in pcm]


def _case(name, pcm, rate, bps, opt):
    pcm = np.asarray(pcm, dtype=np.int64)
    return Case(name, fe.encode(pcm, rate, bps, opt), pcm, bps, rate, pcm.shape[0], 0)


# ---- matrix: every entry of test_flacdec.MATRIX, from the same PCM ------------------------------------------------------
@functools.lru_cache(maxsize=None)
def matrix_cases():
    from test_flacdec import MATRIX, _pcm

    return tuple(_case(name, _pcm(name, ch, bps, n), rate, bps, opt) for name, opt, ch, bps, rate, n in MATRIX)


# ---- extremes: full scale through every stereo decorrelation, width and coding ------------------------------------------
EXT_BPS = (4, 8, 12, 16, 17, 20, 24)
EXT_STEREO = ("independent", "left_side", "right_side", "mid_side")
EXT_CODING = (("fixed2", "fixed", 2), ("lpc8", "lpc", 8), ("lpc20", "lpc", 20), ("verbatim", "verbatim", 0))
EXT_SIGNALS = ("alt", "opp", "min", "noise")
EXT_SAMPLES = 600


def _extreme_pcm(signal, bps, seed):
    hi, lo = (1 << (bps - 1)) - 1, -(1 << (bps - 1))
    n = EXT_SAMPLES
    if signal == "alt":  # L = max, min, max, ...; R the opposite: the side channel swings over all of its bps + 1 bits
        left = np.where(np.arange(n) % 2 == 0, hi, lo)
        return np.stack([left, hi + lo - left])
    if signal == "opp":  # side = max - min = 2^bps - 1, constant
        return np.stack([np.full(n, hi), np.full(n, lo)])
    if signal == "min":
        return np.full((2, n), lo)
    rng = np.random.default_rng(seed)
    pcm = rng.integers(lo, hi + 1, size=(2, n), dtype=np.int64)
    pcm[0, 0], pcm[1, 0], pcm[0, 1], pcm[1, 1] = hi, lo, lo, hi  # both rails are in it for certain
    if signal == "noise_wasted":
        pcm = (pcm >> 3) << 3
    return pcm


@functools.lru_cache(maxsize=None)
def extremes_cases():
    out = []
    for bps in EXT_BPS:
        signals = EXT_SIGNALS + (("noise_wasted",) if bps in (12, 16, 24) else ())
        for stereo in EXT_STEREO:
            for cname, sub, order in EXT_CODING:
                for signal in signals:
                    name = f"bps{bps}-{stereo}-{cname}-{signal}"
                    opt = O(block_size=192, rice2=True, partition_order=1, subframe=sub, order=order, stereo=stereo)
                    out.append(_case(name, _extreme_pcm(signal, bps, zlib.crc32(name.encode())), 44100, bps, opt))
    return tuple(out)


# ---- many frames: the 128-lane decode blocks, the 256-lane check blocks and the 256-wide layout scan ---------------------
def _music(name, ch, n, bps):
    return fe.test_pcm(np.random.default_rng(zlib.crc32(name.encode())), ch, n, bps)


def _long_inputs():
    """(name, pcm, rate, bps, options) of the three long streams; the damage cases re-encode two of them in parts."""
    return {
        "mono16_300x192": (_music("mono16_300x192", 1, 300 * 192, 16), 44100, 16, O(block_size=192, subframe="fixed", order=2)),
        "ms12_600x64": (_music("ms12_600x64", 2, 600 * 64, 12), 48000, 12, O(block_size=64, bs_code="explicit8", stereo="mid_side")),
        "stereo24_130x256": (_music("stereo24_130x256", 2, 130 * 256, 24), 96000, 24, O(block_size=256, stereo="alternate")),
    }


@functools.lru_cache(maxsize=None)
def many_frames_cases():
    """The long streams with the short ones between them, in the order they go into one call."""
    long = {k: _case(k, *v) for k, v in _long_inputs().items()}
    one_sample = _case("one_sample", _music("one_sample", 2, 1, 16), 44100, 16, O())
    hundred = _case("hundred_samples", _music("hundred_samples", 1, 100, 20), 32000, 20, O(subframe="fixed", order=3))
    variable = _case("variable", _music("variable", 2, 10000, 16), 44100, 16, O(variable=True, blocks=[100, 4096, 1, 576, 2000, 3227]))
    one_frame = _case("one_frame", _music("one_frame", 2, 4096, 16), 44100, 16, O(stereo="right_side"))
    no_frame = _case("no_frame", np.zeros((2, 0), dtype=np.int64), 44100, 16, O())
    return (long["mono16_300x192"], one_sample, long["ms12_600x64"], hundred, long["stereo24_130x256"], variable, one_frame, no_frame)


# ---- damage with a derivable answer -------------------------------------------------------------------------------------
def _recrc(frame: bytearray) -> bytes:
    frame[-2:] = fe.crc16(bytes(frame[:-2])).to_bytes(2, "big")
    return bytes(frame)


def _without_blocks(pcm, sizes, gone):
    at = np.concatenate(([0], np.cumsum(sizes)))
    keep = [pcm[:, at[k]:at[k + 1]] for k in range(len(sizes)) if k not in gone]
    return np.concatenate(keep, axis=1)


@functools.lru_cache(maxsize=None)
def damage_cases():
    out = []
    inputs = _long_inputs()
    # the 300-frame stream: a bit flip in frame 270 (its CRC-16 fails), and frame 140 with a reserved type in its first
    # subframe header and the CRC-16 made right again -- a parse failure behind a good CRC, which only the decode kernel
    # finds: the device lays out and decodes a second time
    pcm, rate, bps, opt = inputs["mono16_300x192"]
    meta, frames = fe.encode_parts(pcm, rate, bps, opt)
    assert len(frames) == 300
    frames = list(frames)
    flipped = bytearray(frames[270])
    flipped[len(flipped) // 2] ^= 0x10
    frames[270] = bytes(flipped)
    bad = bytearray(frames[140])
    header_len = 4 + len(fe._utf8_number(140)) + 1  # sync and codes, the frame number, CRC-8 (block size and rate from the tables)
    bad[header_len] = 0x04  # padding bit 0, type 000010 (reserved), no wasted bits
    frames[140] = _recrc(bad)
    out.append(Case("mono16_300x192-flip270-reserved140", meta + b"".join(frames), _without_blocks(pcm, [192] * 300, {140, 270}), bps, rate, 1, 2))
    # the 600-frame stream: its last frame cut short
    pcm, rate, bps, opt = inputs["ms12_600x64"]
    meta, frames = fe.encode_parts(pcm, rate, bps, opt)
    assert len(frames) == 600
    out.append(Case("ms12_600x64-truncated_last", meta + b"".join(frames[:-1]) + frames[-1][:-5], _without_blocks(pcm, [64] * 600, {599}), bps, rate, 2, 1))
    for name, data, want, dropped in fe.damaged_variants():
        want = np.asarray(want, dtype=np.int64)
        out.append(Case(f"variant-{name}", data, want, 16, 44100, want.shape[0], dropped))
    return tuple(out)


TRUNCATED = ("ms12_600x64-truncated_last", "variant-truncated_last")  # the cases whose last frame lacks its end


# ---- fuzz: no derivable answer, the host decoder is the reference --------------------------------------------------------
FUZZ_VARIANTS = 256


@functools.lru_cache(maxsize=None)
def fuzz_streams():
    """[(name, stream)]: 1-3 bit flips or short deletions behind the metadata of two small streams.  The metadata stays
    whole, so the host decoder takes every one of them (its error returns are about metadata and arguments)."""
    rng = np.random.default_rng(0xF1ACBA7C)
    bases = []
    for name, ch, n, bps, opt in (("s16", 2, 7000, 16, O(block_size=576, stereo="alternate", subframe="auto")),
                                  ("m24", 1, 5000, 24, O(block_size=256, order=6))):
        pcm = _music("fuzz-" + name, ch, n, bps)
        meta, frames = fe.encode_parts(pcm, 44100, bps, opt)
        bases.append((name, len(meta), meta + b"".join(frames)))
    out = []
    for k in range(FUZZ_VARIANTS):
        name, meta_len, base = bases[k % 2]
        b = bytearray(base)
        for _ in range(int(rng.integers(1, 4))):
            at = int(rng.integers(meta_len, len(b)))
            if (k // 2) % 2:
                b[at] ^= 1 << int(rng.integers(8))
            else:
                del b[at:at + int(rng.integers(1, 40))]
        out.append((f"fuzz{k}-{name}", bytes(b)))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def fuzz_bookends():
    """The two undamaged streams at the ends of every fuzz batch."""
    return (_case("bookend16", _music("bookend16", 2, 1500, 16), 44100, 16, O(block_size=576, stereo="left_side")),
            _case("bookend24", _music("bookend24", 2, 700, 24), 48000, 24, O(block_size=256, stereo="mid_side")))
