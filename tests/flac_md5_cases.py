"""Cases of the FLAC MD5 tests (tests/test_flac_md5_cpu.py, tests/test_gpu_flac_md5.py).  The oracle is hashlib.md5 over
bytes packed here with NumPy: frames in order, within a frame the channels in order, every sample a signed little-endian
integer of (bps + 7) // 8 bytes.  Nothing in this file calls the library."""
import hashlib
import math
from collections import namedtuple

import numpy as np

BPS = (4, 8, 12, 16, 17, 20, 24)
CHANNELS = (1, 2, 3, 8)
RESIDUES = (0, 1, 55, 56, 57, 63)  # message length mod 64: both sides of the padding's extra block
FMT_S16, FMT_S32 = 1, 2            # rg_sample_format

Stream = namedtuple("Stream", "name pcm bps")  # pcm: int32 [channels][frames], right-justified


def pack(pcm, bps: int) -> bytes:
    """The unencoded audio as FLAC's signature hashes it."""
    pcm = np.asarray(pcm, dtype=np.int64)
    nbytes = (bps + 7) // 8
    flat = pcm.T.reshape(-1)  # frame-major: the channels of a frame side by side
    out = np.empty((flat.size, nbytes), dtype=np.uint8)
    for k in range(nbytes):
        out[:, k] = (flat >> (8 * k)) & 0xFF
    return out.tobytes()


def md5(pcm, bps: int) -> bytes:
    return hashlib.md5(pack(pcm, bps)).digest()


def frame_counts(channels: int, bps: int):
    """Frame counts at which the message length (frames * channels * B) is 0, exactly 64 where that can be, and, for every
    residue of RESIDUES that channels * B can reach mod 64, the smallest such length and the one 64 / gcd frames later."""
    q = channels * ((bps + 7) // 8)
    period = 64 // math.gcd(q, 64)
    counts = {0}
    if 64 % q == 0:
        counts.add(64 // q)
    for r in RESIDUES:
        for f in range(1, period + 1):
            if f * q % 64 == r:
                counts.update((f, f + period))
                break
    return sorted(counts)


def stream_pcm(rng, channels: int, frames: int, bps: int) -> np.ndarray:
    lo, hi = -(1 << (bps - 1)), (1 << (bps - 1)) - 1
    pcm = rng.integers(lo, hi + 1, size=(channels, frames), dtype=np.int64)
    flat = pcm.reshape(-1)
    flat[:3] = [lo, hi, -1][:flat.size]          # the extremes, at the front ...
    if flat.size >= 6:
        flat[-3:] = [-1, hi, lo]                 # ... and where the padding follows
    return pcm.astype(np.int32)


def matrix(seed: int = 11):
    """bps x channels x frame_counts."""
    rng = np.random.default_rng(seed)
    out = []
    for bps in BPS:
        for ch in CHANNELS:
            for n in frame_counts(ch, bps):
                out.append(Stream(f"bps{bps}-ch{ch}-n{n}", stream_pcm(rng, ch, n, bps), bps))
    return out


def long_streams(seed: int = 12):
    """Lengths up to about 5000 frames, odd ones among them (plane 1 of a 16-bit stream then lies on a 2-byte boundary)."""
    rng = np.random.default_rng(seed)
    shapes = [(16, 2, 4999), (16, 2, 1153), (24, 2, 2047), (8, 1, 4097), (12, 3, 333), (20, 8, 129), (17, 1, 5000), (16, 8, 577),
              (4, 2, 3001), (24, 3, 1001)]
    return [Stream(f"long-bps{b}-ch{c}-n{n}", stream_pcm(rng, c, n, b), b) for b, c, n in shapes]


def elem_of(bps: int):
    return (2, np.int16, FMT_S16) if bps <= 16 else (4, np.int32, FMT_S32)


def planes_bytes(s: Stream) -> bytes:
    """The stream in the arena's form: left-justified elements, plane after plane."""
    eb, dt, _ = elem_of(s.bps)
    return (s.pcm.astype(np.int64) << (8 * eb - s.bps)).astype(dt).tobytes()


Arena = namedtuple("Arena", "bytes descs guards")  # descs: (offset_bytes, frames, channels, format) per stream; guards: bool mask


def arena(streams, seed: int = 13) -> Arena:
    """The streams one after the other at offsets that are only sample-aligned, guard samples (full scale) in the gaps.  The
    first stream starts at byte 0, the last one ends at the arena's last byte, and every fourth gap is empty (two streams
    abut); the other gaps hold 1, 3 or 5 16-bit guard samples, plus whatever a 32-bit stream behind them needs for its
    alignment, so 16-bit streams start on 2-byte boundaries that are no 4-byte boundaries."""
    rng = np.random.default_rng(seed)
    buf, guards, descs = bytearray(), bytearray(), []
    for k, s in enumerate(streams):
        eb, _, fmt = elem_of(s.bps)
        if k:
            gap = 0 if k % 4 == 0 else 2 * int(rng.choice((1, 3, 5)))
            gap += -(len(buf) + gap) % eb
            assert gap % 2 == 0
            for g in range(gap // 2):
                buf += (b"\xff\x7f", b"\x00\x80")[g & 1]
            guards += b"\x01" * gap
        assert len(buf) % eb == 0
        body = planes_bytes(s)
        descs.append((len(buf), s.pcm.shape[1], s.pcm.shape[0], fmt))
        buf += body
        guards += b"\x00" * len(body)
    return Arena(np.frombuffer(bytes(buf), dtype=np.uint8).copy(), descs, np.frombuffer(bytes(guards), dtype=np.uint8).astype(bool))


def gpu_streams():
    """What the kernel test hashes in one call: the matrix and the long streams, shuffled."""
    s = matrix() + long_streams()
    order = np.random.default_rng(14).permutation(len(s))
    return [s[i] for i in order]
