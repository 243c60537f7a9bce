"""A deliberately plain FLAC encoder (numpy) for the tests: every knob forces one feature of the format, so the decoders
can be held to the encoder's input exactly.

It chooses nothing clever.  LPC predictors are least-squares fits quantised with the given precision and shift (they may
be poor: any integer predictor gives a valid stream as long as the residual fits); Rice parameters come from the mean
magnitude of a partition.  What it does get right is the bitstream: STREAMINFO, frame headers (every block-size,
sample-rate and sample-size code, fixed and variable blocking, CRC-8), subframes (CONSTANT, VERBATIM, FIXED 0-4,
LPC 1-32, wasted bits), Rice / Rice2 partitions with escapes, the four channel assignments, CRC-16.
"""
from __future__ import annotations

import struct
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np


def crc8(data: bytes) -> int:
    c = 0
    for b in data:
        c ^= b
        for _ in range(8):
            c = ((c << 1) ^ 0x07) & 0xFF if c & 0x80 else (c << 1) & 0xFF
    return c


_CRC16 = []
for _b in range(256):
    _c = _b << 8
    for _ in range(8):
        _c = ((_c << 1) ^ 0x8005) if _c & 0x8000 else (_c << 1)
    _CRC16.append(_c & 0xFFFF)


def crc16(data: bytes) -> int:
    c = 0
    for b in data:
        c = ((c << 8) & 0xFFFF) ^ _CRC16[(c >> 8) ^ b]
    return c


class BitWriter:
    """Bits as numpy arrays of 0/1, packed at the end (vectorised: a three-minute track encodes in seconds)."""

    def __init__(self):
        self.parts: List[np.ndarray] = []

    def put(self, v: int, bits: int):
        if bits:
            self.put_many(np.array([int(v)], dtype=np.int64), bits)

    def put_many(self, vals, bits: int):
        if bits and len(vals):
            u = (np.asarray(vals, dtype=np.int64) & ((1 << bits) - 1)).astype(np.uint64)
            sh = np.arange(bits - 1, -1, -1, dtype=np.uint64)
            self.parts.append(((u[:, None] >> sh[None, :]) & np.uint64(1)).astype(np.uint8).ravel())

    def unary(self, q: int):
        b = np.zeros(q + 1, dtype=np.uint8)
        b[q] = 1
        self.parts.append(b)

    def rice(self, u: np.ndarray, k: int):
        """Rice codes of the non-negative values `u` with parameter k: unary quotient, then k remainder bits."""
        u = np.asarray(u, dtype=np.int64)
        if not len(u):
            return
        q = u >> k
        lens = q + 1 + k
        starts = np.concatenate(([0], np.cumsum(lens)[:-1]))
        b = np.zeros(int(lens.sum()), dtype=np.uint8)
        b[starts + q] = 1
        for t in range(k):
            b[starts + q + 1 + t] = (u >> (k - 1 - t)) & 1
        self.parts.append(b)

    def bytes(self) -> bytes:
        bits = np.concatenate(self.parts) if self.parts else np.zeros(0, dtype=np.uint8)
        return np.packbits(bits).tobytes()


def _utf8_number(v: int) -> bytes:
    if v < 0x80:
        return bytes([v])
    for extra, lead, cap in ((1, 0xC0, 11), (2, 0xE0, 16), (3, 0xF0, 21), (4, 0xF8, 26), (5, 0xFC, 31), (6, 0xFE, 36)):
        if v < (1 << cap):
            tail = [((v >> (6 * k)) & 0x3F) | 0x80 for k in range(extra)][::-1]
            return bytes([lead | (v >> (6 * extra))] + tail)
    raise ValueError(v)


RATE_CODES = {88200: 1, 176400: 2, 192000: 3, 8000: 4, 16000: 5, 22050: 6, 24000: 7, 32000: 8, 44100: 9, 48000: 10, 96000: 11}
BS_CODES = {192: 1, 576: 2, 1152: 3, 2304: 4, 4608: 5, 256: 8, 512: 9, 1024: 10, 2048: 11, 4096: 12, 8192: 13, 16384: 14, 32768: 15}
SS_CODES = {8: 1, 12: 2, 16: 4, 20: 5, 24: 6}
FIXED = {0: [], 1: [1], 2: [2, -1], 3: [3, -3, 1], 4: [4, -6, 4, -1]}


@dataclass
class Options:
    block_size: int = 4096
    variable: bool = False            # variable blocking strategy: sample numbers in the headers
    blocks: Optional[Sequence[int]] = None  # explicit block sizes (sum = length)
    subframe: str = "lpc"             # constant | verbatim | fixed | lpc | auto (cheapest FIXED order per subframe)
    order: int = 8                    # fixed: 0..4, lpc: 1..32
    precision: int = 12               # lpc coefficient bits (1..15)
    shift: int = 10                   # lpc quantisation shift (0..15)
    rice2: bool = False               # Rice2 partitions (5-bit parameters)
    partition_order: int = 2
    escape_every: int = 0             # every n-th partition is written raw (escape code)
    wasted: bool = True               # find and use wasted bits
    stereo: str = "independent"       # independent | left_side | right_side | mid_side | alternate
    bs_code: str = "table"            # table | explicit8 | explicit16
    rate_code: str = "table"          # table | streaminfo | khz | hz | dahz
    ss_code: str = "table"            # table | streaminfo
    extra_metadata: bool = True       # an APPLICATION and a PADDING block behind STREAMINFO


def _lpc_coefs(x: np.ndarray, order: int, precision: int, shift: int) -> List[int]:
    n = len(x)
    if n <= order * 2:
        return [0] * order
    xf = x.astype(np.float64)
    A = np.stack([xf[order - 1 - j:n - 1 - j] for j in range(order)], axis=1)
    sol, *_ = np.linalg.lstsq(A, xf[order:], rcond=None)
    lim = (1 << (precision - 1)) - 1
    return [int(v) for v in np.clip(np.round(sol * (1 << shift)), -lim - 1, lim)]


def _residual(x: np.ndarray, coefs: Sequence[int], shift: int) -> np.ndarray:
    order = len(coefs)
    x = x.astype(np.int64)
    pred = np.zeros(len(x) - order, dtype=np.int64)
    for j, c in enumerate(coefs):
        pred += int(c) * x[order - 1 - j:len(x) - 1 - j]
    return x[order:] - (pred >> shift)


def _write_residual(bw: BitWriter, res: np.ndarray, order: int, bs: int, opt: Options):
    porder = opt.partition_order
    while porder > 0 and ((bs >> porder) << porder != bs or (bs >> porder) < order):
        porder -= 1
    bw.put(1 if opt.rice2 else 0, 2)
    bw.put(porder, 4)
    pbits, escape = (5, 31) if opt.rice2 else (4, 15)
    psize = bs >> porder
    at = 0
    for p in range(1 << porder):
        cnt = psize - order if p == 0 else psize
        part = np.asarray(res[at:at + cnt], dtype=np.int64)
        at += cnt
        if opt.escape_every and p % opt.escape_every == opt.escape_every - 1:
            need = int(np.abs(part).max()) if len(part) else 0
            raw = 0 if need == 0 else need.bit_length() + 1
            bw.put(escape, pbits)
            bw.put(raw, 5)
            bw.put_many(part, raw)
            continue
        u = np.where(part >= 0, 2 * part, -2 * part - 1)
        mean = float(u.mean()) if len(u) else 0.0
        k = 0
        while k < escape - 1 and (1 << (k + 1)) <= mean:
            k += 1
        bw.put(k, pbits)
        bw.rice(u, k)


def _subframe(bw: BitWriter, x: np.ndarray, sbps: int, opt: Options):
    bs = len(x)
    x = x.astype(np.int64)
    wasted = 0
    if opt.wasted and np.any(x != 0):
        acc = int(np.bitwise_or.reduce(x[x != 0]))
        while wasted < sbps - 1 and not (acc >> wasted) & 1:
            wasted += 1
    y = x >> wasted
    ebps = sbps - wasted
    kind, order = opt.subframe, opt.order
    if kind == "constant" and not np.all(x == x[0]):
        kind = "verbatim"
    if kind == "auto":
        costs = [(int(np.abs(_residual(y, FIXED[o], 0)).sum()), o) for o in range(0, min(4, bs - 1) + 1)]
        kind, order = "fixed", min(costs)[1]
    if kind in ("fixed", "lpc") and order >= bs:
        kind = "verbatim"

    def header(t):
        bw.put(0, 1)
        bw.put(t, 6)
        if wasted:
            bw.put(1, 1)
            bw.unary(wasted - 1)
        else:
            bw.put(0, 1)

    if kind == "constant":
        header(0)
        bw.put(int(y[0]), ebps)
    elif kind == "verbatim":
        header(1)
        bw.put_many(y, ebps)
    elif kind == "fixed":
        header(8 + order)
        bw.put_many(y[:order], ebps)
        _write_residual(bw, _residual(y, FIXED[order], 0), order, bs, opt)
    else:
        coefs = _lpc_coefs(y, order, opt.precision, opt.shift)
        header(31 + order)
        bw.put_many(y[:order], ebps)
        bw.put(opt.precision - 1, 4)
        bw.put(opt.shift, 5)
        for cf in coefs:
            bw.put(cf, opt.precision)
        _write_residual(bw, _residual(y, coefs, opt.shift), order, bs, opt)


def encode_parts(pcm, rate: int, bps: int, opt: Optional[Options] = None) -> Tuple[bytes, List[bytes]]:
    """pcm: int [channels][n], right-justified `bps`-bit samples -> (metadata bytes, [frame bytes])."""
    opt = opt or Options()
    pcm = np.asarray(pcm, dtype=np.int64)
    ch, n = pcm.shape
    assert 1 <= ch <= 8 and 4 <= bps <= 32
    lim = 1 << (bps - 1)
    assert n == 0 or (pcm.min() >= -lim and pcm.max() < lim)
    sizes = list(opt.blocks) if opt.blocks is not None else []
    if opt.blocks is None:
        left = n
        while left > 0:
            sizes.append(min(opt.block_size, left))
            left -= sizes[-1]
    assert sum(sizes) == n
    frames, at = [], 0
    modes = ["independent", "left_side", "right_side", "mid_side"]
    for fi, bs in enumerate(sizes):
        x = pcm[:, at:at + bs]
        hdr = bytearray([0xFF, 0xF9 if opt.variable else 0xF8])
        if opt.bs_code == "table" and bs in BS_CODES:
            bcode, bextra = BS_CODES[bs], b""
        elif bs <= 256 and opt.bs_code != "explicit16":
            bcode, bextra = 6, bytes([bs - 1])
        else:
            bcode, bextra = 7, struct.pack(">H", bs - 1)
        rc = opt.rate_code
        if rc == "table" and rate not in RATE_CODES:
            rc = "khz" if rate % 1000 == 0 and rate // 1000 < 256 else ("hz" if rate < 65536 else "dahz")
        rcode, rextra = {"streaminfo": (0, b""), "khz": (12, bytes([rate // 1000 & 0xFF])), "hz": (13, struct.pack(">H", rate & 0xFFFF)),
                         "dahz": (14, struct.pack(">H", rate // 10 & 0xFFFF))}.get(rc, (RATE_CODES.get(rate, 0), b""))
        hdr.append((bcode << 4) | rcode)
        mode = opt.stereo if ch == 2 else "independent"
        if mode == "alternate":
            mode = modes[fi % 4]
        assign = {"independent": ch - 1, "left_side": 8, "right_side": 9, "mid_side": 10}[mode]
        scode = 0 if opt.ss_code == "streaminfo" or bps not in SS_CODES else SS_CODES[bps]
        hdr.append((assign << 4) | (scode << 1))
        hdr += _utf8_number(at if opt.variable else fi)
        hdr += bextra + rextra
        hdr.append(crc8(bytes(hdr)))
        bw = BitWriter()
        if mode == "independent":
            subs = [(x[c], bps) for c in range(ch)]
        else:
            l, r = x[0], x[1]
            side = l - r
            subs = {"left_side": [(l, bps), (side, bps + 1)], "right_side": [(side, bps + 1), (r, bps)],
                    "mid_side": [((l + r) >> 1, bps), (side, bps + 1)]}[mode]
        for s, sb in subs:
            _subframe(bw, s, sb, opt)
        body = bytes(hdr) + bw.bytes()
        frames.append(body + struct.pack(">H", crc16(body)))
        at += bs
    maxb = max(sizes) if sizes else opt.block_size
    minb = maxb if not opt.variable else (min(sizes[:-1]) if len(sizes) > 1 else maxb)
    fl = [len(f) for f in frames] or [0]
    si = struct.pack(">HH", minb & 0xFFFF, maxb & 0xFFFF) + min(fl).to_bytes(3, "big") + max(fl).to_bytes(3, "big")
    si += ((rate << 44) | ((ch - 1) << 41) | ((bps - 1) << 36) | n).to_bytes(8, "big") + bytes(16)
    blocks = [(0, si)]
    if opt.extra_metadata:
        blocks += [(2, b"test" + bytes(12)), (1, bytes(37))]
    meta = bytearray(b"fLaC")
    for k, (t, body) in enumerate(blocks):
        meta += bytes([(0x80 if k == len(blocks) - 1 else 0) | t]) + len(body).to_bytes(3, "big") + body
    return bytes(meta), frames


def encode(pcm, rate: int, bps: int, opt: Optional[Options] = None) -> bytes:
    meta, frames = encode_parts(pcm, rate, bps, opt)
    return meta + b"".join(frames)


def test_pcm(rng, channels: int, n: int, bps: int, kind: str = "music") -> np.ndarray:
    """Deterministic content: a few sines plus noise (compressible), or white noise; `bps`-bit integers."""
    lim = (1 << (bps - 1)) - 1
    if kind == "noise":
        return rng.integers(-lim - 1, lim + 1, size=(channels, n), dtype=np.int64)
    t = np.arange(n, dtype=np.float64)
    out = np.empty((channels, n), dtype=np.int64)
    for c in range(channels):
        s = np.zeros(n)
        for _ in range(3):
            s += rng.uniform(0.05, 0.3) * np.sin(2 * np.pi * rng.uniform(0.001, 0.05) * t + rng.uniform(0, 6.3))
        s += rng.normal(0, 0.01, n)
        out[c] = np.clip(np.round(s * lim), -lim - 1, lim).astype(np.int64)
    return out


test_pcm.__test__ = False


def id3v2_tag(payload: int = 100) -> bytes:
    size = bytes([(payload >> 21) & 0x7F, (payload >> 14) & 0x7F, (payload >> 7) & 0x7F, payload & 0x7F])
    return b"ID3\x04\x00\x00" + size + bytes(payload)


def damaged_variants(seed: int = 7):
    """[(name, stream, PCM of the frames that survive, frames dropped)]: the damage classes the decoders must handle.  The
    expected PCM comes from the encoder's input, not from a decoder."""
    rng = np.random.default_rng(seed)
    pcm = test_pcm(rng, 2, 4096 * 6 + 100, 16)
    meta, frames = encode_parts(pcm, 44100, 16, Options(stereo="mid_side"))
    bs = [4096] * 6 + [100]

    def keep(mask):
        parts = [pcm[:, sum(bs[:k]):sum(bs[:k + 1])] for k in range(len(bs)) if mask[k]]
        return np.concatenate(parts, axis=1)

    def recrc(frame: bytearray) -> bytes:
        frame[-2:] = crc16(bytes(frame[:-2])).to_bytes(2, "big")
        return bytes(frame)

    out = [("truncated_last", meta + b"".join(frames[:-1]) + frames[-1][:-5], keep([1] * 6 + [0]), 1)]
    flipped = bytearray(frames[2])
    flipped[len(flipped) // 2] ^= 0x10
    out.append(("bitflip", meta + b"".join(frames[:2]) + bytes(flipped) + b"".join(frames[3:]), keep([1, 1, 0, 1, 1, 1, 1]), 1))
    # junk between frames: the frame before it reaches to the next header and fails its CRC-16
    out.append(("junk", meta + b"".join(frames[:3]) + b"\x00junk\xff\x12" * 5 + b"".join(frames[3:]), keep([1, 1, 0, 1, 1, 1, 1]), 1))
    out.append(("id3v2", id3v2_tag(300) + meta + b"".join(frames), pcm, 0))
    out.append(("trailing_tag", meta + b"".join(frames) + b"TAG" + bytes(125), pcm, 0))
    # a frame whose CRC-16 holds but whose first subframe has a reserved type: it does not parse and is dropped (the
    # device then lays out and decodes the stream a second time).  Header: 4 bytes, frame number 3 (1 byte), CRC-8.
    bad = bytearray(frames[3])
    bad[6] = 0x04
    out.append(("reserved_subframe", meta + b"".join(frames[:3]) + recrc(bad) + b"".join(frames[4:]), keep([1, 1, 1, 0, 1, 1, 1]), 1))
    # false syncs with a valid CRC-8 inside a payload (verbatim mono 16-bit samples are the payload's bytes): one claims
    # frame 40 (inside the continuity window, but nothing continues it), one the very number expected next
    for name, number in (("false_sync", 0x28), ("false_sync_next", 0x02)):
        mono = test_pcm(rng, 1, 4096 * 4, 16)
        fake = bytes([0xFF, 0xF8, 0xC9, 0x08, number])
        fake += bytes([crc8(fake)])
        words = [int.from_bytes(fake[k:k + 2], "big") for k in (0, 2, 4)]
        mono[0, 5000:5003] = [w - 65536 if w >= 32768 else w for w in words]
        out.append((name, encode(mono, 44100, 16, Options(subframe="verbatim", wasted=False)), mono, 0))
    return out
