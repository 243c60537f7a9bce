"""ctypes binding of include/mp3rgain_amd_mp3verify.h: the info tag of an MPEG Layer III stream, the two CRCs through their
seams, and the verdict of `--verify` for an MP3 file.

Only loads the in-tree shared library; route 0 of the seams and info_tag need no GPU."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import List, Optional

import numpy as np

from . import _capi

HAS_INFO_TAG, HAS_LAME_EXT, TAG_CRC_MATCH, MUSIC_CRC_MATCH, LENGTH_MATCH, FRAME_COUNT_MATCH, COMPLETE, FRAME_CRCS_OK, GAIN_TAG = (
    1, 2, 4, 8, 16, 32, 64, 128, 256)
FLAG_NAMES = ("has_info_tag", "has_lame_ext", "tag_crc_match", "music_crc_match", "length_match", "frame_count_match", "complete",
              "frame_crcs_ok", "gain_tag")


class Mp3TagInfo(C.Structure):
    """rg_mp3_tag_info."""
    _fields_ = [
        ("info_frame", C.c_uint32),
        ("has_lame_ext", C.c_uint32),
        ("tag_frame_offset", C.c_uint64),
        ("tag_frame_bytes", C.c_uint32),
        ("xing_flags", C.c_uint32),
        ("has_frames", C.c_uint32),
        ("xing_frames", C.c_uint32),
        ("xing_bytes", C.c_uint32),
        ("ext_offset", C.c_uint32),
        ("music_length", C.c_uint32),
        ("music_crc", C.c_uint16),
        ("tag_crc", C.c_uint16),
        ("encoder", C.c_char * 9),
        ("reserved", C.c_uint8 * 7),
    ]


class Mp3VerifyRecord(C.Structure):
    """rg_mp3_verify_result."""
    _fields_ = [
        ("status", C.c_int32),
        ("flags", C.c_uint32),
        ("audio_frames", C.c_uint32),
        ("dropped_frames", C.c_uint32),
        ("protected_frames", C.c_uint32),
        ("frame_crc_failed", C.c_uint32),
        ("junk_bytes", C.c_uint32),
        ("xing_frames", C.c_uint32),
        ("music_length", C.c_uint32),
        ("info_frame", C.c_uint32),
        ("audio_bytes", C.c_uint64),
        ("music_crc_stored", C.c_uint16),
        ("music_crc_computed", C.c_uint16),
        ("tag_crc_stored", C.c_uint16),
        ("tag_crc_computed", C.c_uint16),
        ("encoder", C.c_uint8 * 9),
        ("xing_flags", C.c_uint8),
        ("reserved", C.c_uint8 * 6),
    ]


SYMBOLS = [
    ("rg_mp3_info_tag", C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(Mp3TagInfo)]),
    ("rg_mp3_crc_folded_host", C.c_uint16, [C.c_void_p, C.c_size_t]),
    ("rg_mp3_verify_data", C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(Mp3VerifyRecord)]),
    ("rg_mp3_verify", C.c_int, [C.c_void_p, C.POINTER(C.c_char_p), C.c_size_t, C.POINTER(Mp3VerifyRecord)]),
    ("rg_mp3_crc_ranges", C.c_int, [C.c_void_p, C.c_int, C.c_size_t, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64), C.c_void_p, C.c_size_t,
                                    C.POINTER(C.c_uint16)]),
    ("rg_mp3_frame_crc_check", C.c_int, [C.c_void_p, C.c_int, C.c_size_t, C.POINTER(C.c_uint64), C.c_void_p, C.c_size_t, C.POINTER(C.c_uint8)]),
    ("rg_mp3_crc_rate", C.c_int, [C.c_void_p, C.c_size_t, C.c_uint64, C.c_size_t, C.c_uint32, C.c_uint32, C.c_size_t, C.POINTER(C.c_double),
                                  C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_size_t)]),
]


class Mp3VerifyError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"{msg} (status {code})")
        self.code = code


def _lib():
    L = _capi.load()
    if not getattr(L, "_mp3verify_bound", False):
        for name, res, args in SYMBOLS:
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        L._mp3verify_bound = True
    return L


def is_mpeg(data: bytes) -> bool:
    """Whether `--verify` sends a file that starts like this to rg_mp3_verify: a bare MPEG Layer III stream (not RIFF/WAVE, not
    FLAC, also behind an ID3v2 tag, and not an ISO base media file)."""
    from . import flacdec

    if data[:4] == b"RIFF" or data[4:8] == b"ftyp" or flacdec.is_flac(data):
        return False
    info = Mp3TagInfo()
    buf = (C.c_char * max(1, len(data))).from_buffer_copy(data if data else b"\0")
    return _lib().rg_mp3_info_tag(buf, len(data), C.byref(info)) == 0


def info_tag(data: bytes) -> Mp3TagInfo:
    """rg_mp3_info_tag: the tag frame of an MPEG Layer III stream."""
    info = Mp3TagInfo()
    buf = (C.c_char * max(1, len(data))).from_buffer_copy(data if data else b"\0")
    rc = _lib().rg_mp3_info_tag(buf, len(data), C.byref(info))
    if rc != 0:
        raise Mp3VerifyError(rc, "not an MPEG Layer III stream")
    return info


def crc_ranges(ctx, route: int, offsets, lengths, data: np.ndarray) -> List[int]:
    """rg_mp3_crc_ranges: CRC-16/ARC of data[offsets[i] : offsets[i] + lengths[i]]; route 0 = host twin (`ctx` may be None),
    route 1 = the chunk and fold kernels."""
    L = _lib()
    n = len(offsets)
    data = np.ascontiguousarray(data, dtype=np.uint8)
    off = (C.c_uint64 * max(1, n))(*[int(x) for x in offsets])
    ln = (C.c_uint64 * max(1, n))(*[int(x) for x in lengths])
    out = (C.c_uint16 * max(1, n))()
    rc = L.rg_mp3_crc_ranges(ctx, int(route), n, off, ln, data.ctypes.data if data.size else None, data.size, out)
    if rc != 0:
        raise Mp3VerifyError(rc, _capi.load().rg_last_error(ctx).decode())
    return list(out[:n])


def frame_crc_check(ctx, route: int, frame_offsets, data: np.ndarray) -> List[int]:
    """rg_mp3_frame_crc_check: 1 per protected frame whose CRC word matches, else 0."""
    L = _lib()
    n = len(frame_offsets)
    data = np.ascontiguousarray(data, dtype=np.uint8)
    off = (C.c_uint64 * max(1, n))(*[int(x) for x in frame_offsets])
    out = (C.c_uint8 * max(1, n))()
    rc = L.rg_mp3_frame_crc_check(ctx, int(route), n, off, data.ctypes.data if data.size else None, data.size, out)
    if rc != 0:
        raise Mp3VerifyError(rc, _capi.load().rg_last_error(ctx).decode())
    return list(out[:n])


@dataclass
class Mp3VerifyResult:
    """One file of Analyzer.verify_mp3 (rg_mp3_verify_result)."""
    flags: int
    audio_frames: int
    dropped_frames: int
    protected_frames: int
    frame_crc_failed: int
    junk_bytes: int
    xing_frames: int
    music_length: int
    info_frame: int
    audio_bytes: int
    music_crc_stored: int
    music_crc_computed: int
    tag_crc_stored: int
    tag_crc_computed: int
    encoder: str
    xing_flags: int = 0
    error: Optional[Exception] = None  # why there is no verdict; every other field is then zero

    def flag(self, name: str) -> bool:
        return bool(self.flags & (1 << FLAG_NAMES.index(name)))

    @property
    def verdict(self) -> str:
        """The first that applies (include/mp3rgain_amd_mp3verify.h; README: --verify)."""
        f = self.flag
        if self.error is not None:
            return str(self.error)
        if self.dropped_frames:
            return f"{self.dropped_frames} frames dropped"
        if self.frame_crc_failed:
            return f"{self.frame_crc_failed} frame CRCs failed"
        if f("has_lame_ext") and not f("length_match"):
            return "length mismatch"
        if f("has_lame_ext") and not f("music_crc_match"):
            return "gain applied, CRC not comparable" if f("gain_tag") else "music CRC mismatch"
        if f("has_lame_ext") and not f("tag_crc_match"):
            return "info tag CRC mismatch"
        if self.info_frame == 1 and (self.xing_flags & 1) and not f("frame_count_match"):
            return "frame count mismatch"
        if not f("has_lame_ext"):
            return "no checksum"
        return "verified"

    @property
    def failed(self) -> bool:
        return self.verdict not in ("verified", "no checksum", "gain applied, CRC not comparable")

    @property
    def verified(self) -> bool:
        return self.verdict == "verified"

    def as_dict(self) -> dict:
        d = {k: getattr(self, k) for k in ("audio_frames", "dropped_frames", "protected_frames", "frame_crc_failed", "junk_bytes", "xing_frames",
                                           "music_length", "info_frame", "audio_bytes", "music_crc_stored", "music_crc_computed",
                                           "tag_crc_stored", "tag_crc_computed", "encoder", "xing_flags", "flags")}
        d.update({n: self.flag(n) for n in FLAG_NAMES})
        return d


def result_of(r: Mp3VerifyRecord, error=None) -> Mp3VerifyResult:
    enc = bytes(r.encoder).split(b"\0")[0].decode("latin-1")
    return Mp3VerifyResult(int(r.flags), int(r.audio_frames), int(r.dropped_frames), int(r.protected_frames), int(r.frame_crc_failed),
                           int(r.junk_bytes), int(r.xing_frames), int(r.music_length), int(r.info_frame), int(r.audio_bytes),
                           int(r.music_crc_stored), int(r.music_crc_computed), int(r.tag_crc_stored), int(r.tag_crc_computed), enc, int(r.xing_flags), error)


def verify_data(data: bytes) -> Mp3VerifyResult:
    """rg_mp3_verify_data: the host twin of Analyzer.verify_mp3 for one stream in memory (no GPU)."""
    rec = Mp3VerifyRecord()
    buf = (C.c_char * max(1, len(data))).from_buffer_copy(data if data else b"\0")
    rc = _lib().rg_mp3_verify_data(buf, len(data), C.byref(rec))
    return result_of(rec, Mp3VerifyError(rc, "not a bare MPEG Layer III stream") if rc != 0 else None)


def verify_data_raw(data: bytes) -> bytes:
    rec = Mp3VerifyRecord()
    buf = (C.c_char * max(1, len(data))).from_buffer_copy(data if data else b"\0")
    _lib().rg_mp3_verify_data(buf, len(data), C.byref(rec))
    return bytes(rec)


def crc_folded_host(data: bytes) -> int:
    """rg_mp3_crc_folded_host: CRC-16/ARC of `data` by the kernels' arithmetic (chunks, trees, powers of x) run on the host."""
    buf = (C.c_char * max(1, len(data))).from_buffer_copy(data if data else b"\0")
    return int(_lib().rg_mp3_crc_folded_host(buf, len(data)))
