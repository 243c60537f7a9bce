"""Cases and oracles of MP3 verification (include/mp3rgain_amd_mp3verify.h), shared by tests/test_mp3_verify_cpu.py and
tests/test_gpu_mp3_verify.py.

The oracle of both CRCs is bit by bit and shares no table with the C code.  The info-tag writer builds an Xing/Info frame
with the 36-byte LAME extension and correct checksums round streams of oracle/mp3_bitstream.py; `damaged` derives the damaged
variants and says, from the definitions alone, which flags and verdict each must read."""
import random
import struct
import sys
from dataclasses import dataclass
from pathlib import Path
from typing import Dict, List, Optional

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "oracle"))
import mp3_bitstream as mb  # noqa: E402

L = 64            # RG_CRC_CHUNK (csrc/rg_crc16.h): bytes one lane hashes
TILE = 256 * L    # bytes one block hashes

FIXTURES = ROOT / "tests" / "golden" / "fixtures"
DENSE = sorted((ROOT / "tests" / "golden" / "mp3").glob("dense_*.mp3"))


# ---- the oracles: bit by bit ------------------------------------------------------------------------------------------------
def crc16_arc(data: bytes) -> int:
    """CRC-16/ARC: polynomial 0x8005 reflected, init 0, no final xor."""
    crc = 0
    for b in data:
        crc ^= b
        for _ in range(8):
            crc = (crc >> 1) ^ 0xA001 if crc & 1 else crc >> 1
    return crc


def crc16_mpeg(data: bytes) -> int:
    """The frame CRC: polynomial 0x8005, MSB first, init 0xFFFF."""
    crc = 0xFFFF
    for b in data:
        for k in range(7, -1, -1):
            top = (crc >> 15) & 1
            crc = (crc << 1) & 0xFFFF
            if top ^ ((b >> k) & 1):
                crc ^= 0x8005
    return crc


def side_bytes(lsf: bool, mono: bool) -> int:
    return (9 if mono else 17) if lsf else (17 if mono else 32)


def frame_crc_ok(frame: bytes) -> bool:
    """`frame`: a protected frame from its first byte; the oracle of rg_mp3_frame_crc_check for a valid header."""
    lsf = ((frame[1] >> 3) & 3) != 3
    mono = (frame[3] >> 6) == 3
    sb = side_bytes(lsf, mono)
    return crc16_mpeg(frame[2:4] + frame[6:6 + sb]) == (frame[4] << 8 | frame[5])


# ---- streams ----------------------------------------------------------------------------------------------------------------
def stream(rate: int, mode: int, n_frames: int, crc: bool, seed: int, bitrate: int) -> List[bytes]:
    """`n_frames` audio frames of an oracle/mp3_bitstream.py stream, one bytes object per frame."""
    rng = random.Random(seed)
    lsf = mb.RATES[rate][0] != 3
    nch = 1 if mode == 3 else 2
    frames = [mb.FrameSpec([[mb.GranuleSpec(mb.random_spectrum(rng, 100, 5)) for _ in range(nch)] for _ in range(1 if lsf else 2)],
                           bitrate, mode=mode, crc=crc) for _ in range(n_frames)]
    data = mb.write_stream(frames, rate, rng)
    fb = (72 if lsf else 144) * bitrate * 1000 // rate
    assert len(data) == fb * n_frames
    return [data[i * fb:(i + 1) * fb] for i in range(n_frames)]


def tag_frame(rate: int, mode: int, bitrate: int, protected: bool, flags: int, n_frames: int, music: bytes, marker: bytes = b"Info",
              encoder: bytes = b"LAME3.100", lavf_rule: bool = False, with_ext: bool = True) -> bytes:
    """An Xing/Info frame for a stream of `n_frames` audio frames whose bytes are `music`, with the LAME extension: music
    length (this frame included), music CRC and tag CRC by LAME's rule, or by libavformat's with `lavf_rule`."""
    ver_bits, rate_idx = mb.RATES[rate]
    lsf = ver_bits != 3
    br_idx = (mb.BITRATES_V2 if lsf else mb.BITRATES_V1).index(bitrate)
    fb = (72 if lsf else 144) * bitrate * 1000 // rate
    sb = side_bytes(lsf, mode == 3)
    head = bytes([0xFF, 0xE0 | (ver_bits << 3) | (1 << 1) | (0 if protected else 1), (br_idx << 4) | (rate_idx << 2), (mode << 6) | 0x04])
    f = bytearray(fb)
    f[0:4] = head
    at = 4 + (2 if protected else 0) + sb
    if protected:
        f[4:6] = struct.pack(">H", crc16_mpeg(bytes(f[2:4]) + bytes(sb)))
    f[at:at + 4] = marker
    f[at + 4:at + 8] = struct.pack(">I", flags)
    p = at + 8
    if flags & 1:
        f[p:p + 4] = struct.pack(">I", n_frames)
        p += 4
    if flags & 2:
        f[p:p + 4] = struct.pack(">I", fb + len(music))
        p += 4
    if flags & 4:
        f[p:p + 100] = bytes(min(255, i * 256 // 100) for i in range(100))
        p += 100
    if flags & 8:
        f[p:p + 4] = struct.pack(">I", 57)
        p += 4
    if not with_ext:
        return bytes(f)
    assert p + 36 <= fb, "the frame is too small for the extension"
    f[p:p + 9] = encoder.ljust(9, b"\0")[:9]
    f[p + 9] = 0x24
    f[p + 28:p + 32] = struct.pack(">I", fb + len(music))
    f[p + 32:p + 34] = struct.pack(">H", crc16_arc(music))
    if lavf_rule:
        assert p + 36 <= 190
        f[p + 34:p + 36] = struct.pack(">H", crc16_arc(bytes(f[:190])))  # (the field is still zero)
    else:
        f[p + 34:p + 36] = struct.pack(">H", crc16_arc(bytes(f[:p + 34])))
    return bytes(f)


def ape_tag(items: Dict[str, str]) -> bytes:
    """An APEv2 tag with header and footer."""
    body = b"".join(struct.pack("<II", len(v.encode()), 0) + k.encode() + b"\0" + v.encode() for k, v in items.items())
    size = len(body) + 32

    def block(flags):
        return b"APETAGEX" + struct.pack("<IIII", 2000, size, len(items), flags) + bytes(8)
    return block(0xA0000000) + body + block(0x80000000)


ID3V1 = b"TAG" + b"title".ljust(30, b"\0") + bytes(94) + b"\xff"
ID3V2 = b"ID3\x04\x00\x00\x00\x00\x00\x22" + b"TIT2\x00\x00\x00\x05\x00\x00\x03abcd" + bytes(19)  # 10 + 34 bytes

F = {"has_info_tag": 1, "has_lame_ext": 2, "tag_crc_match": 4, "music_crc_match": 8, "length_match": 16, "frame_count_match": 32,
     "complete": 64, "frame_crcs_ok": 128, "gain_tag": 256}
ALL_GOOD = 255


@dataclass
class Case:
    name: str
    data: bytes
    flags: int                 # expected
    verdict: str
    audio_frames: int
    protected_frames: int = 0
    frame_crc_failed: int = 0
    music_crc_computed: Optional[int] = None
    info_frame: int = 1
    dropped_frames: int = 0


# (rate, mode, bitrate): MPEG-1 stereo, MPEG-1 mono, MPEG-2 stereo, MPEG-2 mono
KINDS = {"v1_stereo": (44100, 0, 128), "v1_mono": (44100, 3, 96), "v2_stereo": (22050, 1, 64), "v2_mono": (24000, 3, 64)}
N_FRAMES = 12


def clean(kind: str, crc: bool, protected_tag: bool, flags: int, seed: int, **kw):
    rate, mode, br = KINDS[kind]
    frames = stream(rate, mode, N_FRAMES, crc, seed, br)
    music = b"".join(frames)
    tag = tag_frame(rate, mode, br, protected_tag, flags, N_FRAMES, music, **kw)
    return tag, frames


def clean_cases() -> List[Case]:
    """Every kind x protected / unprotected tag frame x flag sets 15, 7, 1, streams with and without frame CRCs, behind an
    ID3v2 tag or not: all read verified."""
    out = []
    seed = 100
    for kind in KINDS:
        for protected_tag in (False, True):
            for flags in (15, 7, 1):
                seed += 1
                crc = (seed % 2) == 0
                lavf = flags == 1 and not protected_tag and kind != "v1_stereo"  # the field lies inside the first 190 bytes
                tag, frames = clean(kind, crc, protected_tag, flags, seed, marker=b"Xing" if flags == 7 else b"Info", lavf_rule=lavf,
                                    encoder=b"Lavc62.11" if lavf else b"LAME3.100")
                head = ID3V2 if seed % 3 == 0 else b""
                out.append(Case(f"{kind}-{'p' if protected_tag else 'u'}-{flags}", head + tag + b"".join(frames), ALL_GOOD, "verified", N_FRAMES,
                                N_FRAMES if crc else 0, 0, crc16_arc(b"".join(frames))))
    return out


def damaged_cases() -> List[Case]:
    out = []
    for k, (kind, protected_tag) in enumerate((("v1_stereo", False), ("v2_mono", True))):
        rate, mode, br = KINDS[kind]
        tag, frames = clean(kind, True, protected_tag, 15, 500 + k)
        music = b"".join(frames)
        whole = tag + music
        fb = len(frames[0])
        sb = side_bytes(mb.RATES[rate][0] != 3, mode == 3)
        sfx = f"-{kind}"

        def flip(data: bytes, at: int, bit: int = 0) -> bytes:
            b = bytearray(data)
            b[at] ^= 1 << bit
            return bytes(b)
        # a flipped audio byte: the last byte of a frame in the middle (main data or its padding; every frame still decodes)
        at = len(tag) + 5 * fb + fb - 1
        bad = flip(whole, at)
        out.append(Case("audio-byte" + sfx, bad, ALL_GOOD & ~F["music_crc_match"], "music CRC mismatch", N_FRAMES, N_FRAMES, 0, crc16_arc(bad[len(tag):])))
        # a flipped side-information bit in a protected frame: the private bits behind main_data_begin, which no decoder reads
        lsf = mb.RATES[rate][0] != 3
        at = len(tag) + 3 * fb + 6 + 1
        bit = 7 if lsf else 6  # MPEG-1: main_data_begin has 9 bits, LSF 8; the bit behind it is private
        bad = flip(whole, at, bit)
        out.append(Case("side-bit" + sfx, bad, ALL_GOOD & ~(F["music_crc_match"] | F["frame_crcs_ok"]), "1 frame CRCs failed", N_FRAMES, N_FRAMES, 1,
                        crc16_arc(bad[len(tag):])))
        # the last frame dropped from the file
        bad = whole[:-fb]
        out.append(Case("last-frame-gone" + sfx, bad, ALL_GOOD & ~(F["music_crc_match"] | F["length_match"] | F["frame_count_match"]), "length mismatch",
                        N_FRAMES - 1, N_FRAMES - 1, 0, crc16_arc(bad[len(tag):])))
        # six bytes cut off: the walk loses the last frame, the CRC runs over what is left
        bad = whole[:-6]
        out.append(Case("six-short" + sfx, bad, ALL_GOOD & ~(F["music_crc_match"] | F["length_match"] | F["frame_count_match"]), "length mismatch",
                        N_FRAMES - 1, N_FRAMES - 1, 0, crc16_arc(bad[len(tag):])))
        # appended tags lie behind the music length: nothing changes
        out.append(Case("id3v1" + sfx, whole + ID3V1, ALL_GOOD, "verified", N_FRAMES, N_FRAMES, 0, crc16_arc(music)))
        out.append(Case("apev2" + sfx, whole + ape_tag({"ARTIST": "nobody"}) + ID3V1, ALL_GOOD, "verified", N_FRAMES, N_FRAMES, 0, crc16_arc(music)))
        # gain applied the way this project's -r does: global_gain bytes rewritten (here: one, together with the frame's CRC
        # word), an MP3GAIN_UNDO item appended
        b = bytearray(whole)
        fr = len(tag) + 2 * fb
        # global_gain of granule 0, channel 0: behind main_data_begin, the private bits, scfsi (MPEG-1), part2_3_length (12) and
        # big_values (9); its lowest bit is flipped
        nch = 1 if mode == 3 else 2
        gbit = ((8 + (1 if nch == 1 else 2)) if lsf else (9 + (5 if nch == 1 else 3) + 4 * nch)) + 12 + 9 + 7
        b[fr + 6 + gbit // 8] ^= 0x80 >> (gbit % 8)
        b[fr + 4:fr + 6] = struct.pack(">H", crc16_mpeg(bytes(b[fr + 2:fr + 4]) + bytes(b[fr + 6:fr + 6 + sb])))
        gained = bytes(b) + ape_tag({"MP3GAIN_UNDO": "+001,+001,N", "MP3GAIN_MINMAX": "149,151"})
        out.append(Case("gain" + sfx, gained, (ALL_GOOD | F["gain_tag"]) & ~F["music_crc_match"], "gain applied, CRC not comparable", N_FRAMES, N_FRAMES, 0,
                        crc16_arc(bytes(b[len(tag):]))))
        # a frame the decoders drop: big_values (the 9 bits in front of global_gain) above 288.  The frame is protected, so its
        # CRC fails as well; dropped frames come first in the verdict
        b = bytearray(whole)
        fr = len(tag) + 7 * fb
        for bit in range(gbit - 7 - 9, gbit - 7):
            b[fr + 6 + bit // 8] |= 0x80 >> (bit % 8)
        out.append(Case("dropped" + sfx, bytes(b), ALL_GOOD & ~(F["music_crc_match"] | F["complete"] | F["frame_crcs_ok"]), "1 frames dropped", N_FRAMES,
                        N_FRAMES, 1, crc16_arc(bytes(b[len(tag):])), dropped_frames=1))
        # an untouched file with the undo tag still verifies
        out.append(Case("gain-tag-only" + sfx, whole + ape_tag({"MP3GAIN_UNDO": "+000,+000,N"}), ALL_GOOD | F["gain_tag"], "verified", N_FRAMES, N_FRAMES,
                        0, crc16_arc(music)))
        # the tag's own CRC
        p = 4 + (2 if protected_tag else 0) + sb + 8 + 4 + 4 + 100 + 4 + 9  # the extension's byte 9 (revision / VBR method)
        bad = flip(whole, p)
        out.append(Case("tag-crc" + sfx, bad, ALL_GOOD & ~F["tag_crc_match"], "info tag CRC mismatch", N_FRAMES, N_FRAMES, 0, crc16_arc(music)))
        # the frames field
        p = 4 + (2 if protected_tag else 0) + sb + 8
        b = bytearray(whole)
        b[p:p + 4] = struct.pack(">I", N_FRAMES + 1)
        ext = 4 + (2 if protected_tag else 0) + sb + 0x78
        b[ext + 34:ext + 36] = struct.pack(">H", crc16_arc(bytes(b[:ext + 34])))
        out.append(Case("frame-count" + sfx, bytes(b), ALL_GOOD & ~F["frame_count_match"], "frame count mismatch", N_FRAMES, N_FRAMES, 0, crc16_arc(music)))
        # no extension: Xing with the frames field only
        tag1 = tag_frame(rate, mode, br, protected_tag, 1, N_FRAMES, music, marker=b"Xing", with_ext=False)
        out.append(Case("no-ext" + sfx, tag1 + music, F["has_info_tag"] | F["frame_count_match"] | F["complete"] | F["frame_crcs_ok"], "no checksum", N_FRAMES,
                        N_FRAMES, 0, 0))
    return out


# ---- ranges for the CRC-16/ARC seam ------------------------------------------------------------------------------------------
LENGTHS = [0, 1, L - 1, L, L + 1, 2 * L, 64 * L - 1, 64 * L + 1, 256 * L - 1, 256 * L + 1, 300 * L + 17]


@dataclass
class Ranges:
    data: np.ndarray
    offsets: List[int]
    lengths: List[int]
    guards: np.ndarray  # bool mask: bytes no range covers


def ranges(lengths: List[int], seed: int) -> Ranges:
    """Ranges of these lengths laid end to end from the buffer's first byte to its last.  Every third range abuts its
    predecessor; in front of the others lie 0 to 7 guard bytes, so that start offsets walk through every residue mod 8."""
    rng = np.random.default_rng(seed)
    offs, pos = [], 0
    for i, n in enumerate(lengths):
        if i % 3:
            pos += (i - pos) % 8
        offs.append(pos)
        pos += n
    data = rng.integers(0, 256, size=pos, dtype=np.uint8)
    guards = np.ones(pos, dtype=bool)
    for o, n in zip(offs, lengths):
        guards[o:o + n] = False
    return Ranges(data, offs, list(lengths), guards)


def expect(r: Ranges) -> List[int]:
    raw = r.data.tobytes()
    return [crc16_arc(raw[o:o + n]) for o, n in zip(r.offsets, r.lengths)]


# ---- synthetic protected frames for the frame-CRC seam ------------------------------------------------------------------------
def protected_frames(n: int, seed: int):
    """`n` protected frame heads (header, CRC word, side information: every side-information size) at arbitrary offsets of one
    buffer, the last one touching the buffer's last byte; a known tenth has one bit flipped in header byte 2 or 3, the side
    information or the CRC word -- flips that keep the header valid and the side information's size.  -> (data, offsets, ok)."""
    rng = random.Random(seed)
    heads = {32: (3, 0), 17: (3, 3), 9: (2, 3)}  # side bytes -> (version bits, mode); 17 is also MPEG-2 stereo (2, 0)
    buf = bytearray()
    offs, ok = [], []
    for i in range(n):
        sb = (9, 17, 32)[i % 3]
        ver, mode = heads[sb] if not (sb == 17 and i % 2) else (2, 0)
        buf += bytes(rng.randrange(256) for _ in range(rng.randrange(0, 5)))
        f = bytearray([0xFF, 0xE0 | (ver << 3) | 2, (rng.randrange(1, 15) << 4) | (rng.randrange(3) << 2) | (rng.randrange(4)),
                       (mode << 6) | rng.randrange(64)])
        side = bytes(rng.randrange(256) for _ in range(sb))
        f += struct.pack(">H", crc16_mpeg(bytes(f[2:4]) + side)) + side
        good = True
        if i % 10 == 3:
            good = False
            where = rng.choice(("h2", "h3", "side", "crc"))
            if where == "h2":
                f[2] ^= 1 << rng.randrange(2)          # padding / private bit: the header stays valid
            elif where == "h3":
                f[3] ^= 1 << rng.randrange(6)          # below the mode bits: the side information keeps its size
            elif where == "side":
                f[6 + rng.randrange(sb)] ^= 1 << rng.randrange(8)
            else:
                f[4 + rng.randrange(2)] ^= 1 << rng.randrange(8)
        offs.append(len(buf))
        ok.append(1 if good else 0)
        buf += f
    return np.frombuffer(bytes(buf), dtype=np.uint8), offs, ok
