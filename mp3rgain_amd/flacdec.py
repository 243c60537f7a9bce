"""ctypes binding of include/mp3rgain_amd_flac.h: a native FLAC stream -> planar int32 PCM (host decoder).

Host code, no GPU needed.  Only loads the in-tree shared library -- there is no Python decoder behind it."""
from __future__ import annotations

import ctypes as C
from typing import List, Tuple

import numpy as np

from . import _capi

OK, ERR_ARG, ERR_NOT_FLAC, ERR_CAPACITY, ERR_UNSUPPORTED = 0, -1, -2, -3, -4


class FlacInfo(C.Structure):
    _fields_ = [
        ("sample_rate", C.c_uint32),
        ("channels", C.c_uint32),
        ("bits_per_sample", C.c_uint32),
        ("min_block_size", C.c_uint32),
        ("max_block_size", C.c_uint32),
        ("id3v2_bytes", C.c_uint32),
        ("total_samples", C.c_uint64),
        ("metadata_bytes", C.c_uint64),
        ("frames", C.c_uint64),
        ("audio_frames", C.c_uint32),
        ("dropped_frames", C.c_uint32),
    ]

    def as_dict(self):
        return {k: int(getattr(self, k)) for k, _ in self._fields_}


class FlacFrame(C.Structure):
    _fields_ = [
        ("offset", C.c_uint64),
        ("first_sample", C.c_uint64),
        ("length", C.c_uint32),
        ("block_size", C.c_uint32),
        ("channel_assignment", C.c_uint8),
        ("header_length", C.c_uint8),
        ("reserved", C.c_uint16),
        ("reserved2", C.c_uint32),
    ]


class FlacVerifyRecord(C.Structure):
    """rg_flac_verify_result."""
    _fields_ = [
        ("status", C.c_int32),
        ("flags", C.c_uint32),
        ("frames", C.c_uint64),
        ("total_samples", C.c_uint64),
        ("audio_frames", C.c_uint32),
        ("dropped_frames", C.c_uint32),
        ("md5_stream", C.c_uint8 * 16),
        ("md5_decoded", C.c_uint8 * 16),
    ]


VERIFY_HAS_SIGNATURE, VERIFY_MD5_MATCH, VERIFY_LENGTH_MATCH, VERIFY_COMPLETE = 1, 2, 4, 8

SYMBOLS = [
    ("rg_flac_is_flac", C.c_int, [C.c_void_p, C.c_size_t]),
    ("rg_flac_scan", C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(FlacInfo)]),
    ("rg_flac_index_frames", C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(FlacFrame), C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(FlacInfo)]),
    ("rg_flac_decode_s32", C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p), C.c_uint64, C.POINTER(FlacInfo)]),
    ("rg_flac_index_selfcheck", C.c_int, [C.c_void_p, C.c_size_t]),
    ("rg_flac_last_error", C.c_char_p, []),
    ("rg_flac_decode_device", C.c_int, [C.c_void_p, C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p), C.c_uint64, C.POINTER(FlacInfo)]),
    ("rg_flac_stage_device_batch", C.c_int, [C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p), C.POINTER(C.c_size_t), C.POINTER(_capi.TrackDesc),
                                             C.POINTER(FlacInfo), C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t)]),
    ("rg_flac_decode_arena", C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(C.c_uint32), C.POINTER(FlacInfo)]),
    ("rg_flac_stream_md5", C.c_int, [C.c_void_p, C.c_size_t, C.c_void_p]),
    ("rg_flac_md5_s32", C.c_int, [C.POINTER(C.c_void_p), C.c_uint32, C.c_uint64, C.c_uint32, C.c_void_p]),
    ("rg_flac_md5_arena", C.c_int, [C.c_void_p, C.c_int, C.c_size_t, C.POINTER(_capi.TrackDesc), C.POINTER(C.c_uint32), C.c_void_p, C.c_size_t,
                                    C.c_void_p]),
    ("rg_flac_md5_rate", C.c_int, [C.c_void_p, C.c_size_t, C.c_uint64, C.c_uint32, C.c_size_t, C.c_uint32, C.c_uint32, C.POINTER(C.c_double),
                                   C.POINTER(C.c_double), C.POINTER(C.c_size_t)]),
    ("rg_flac_verify", C.c_int, [C.c_void_p, C.POINTER(C.c_char_p), C.c_size_t, C.POINTER(FlacVerifyRecord)]),
]


class FlacError(RuntimeError):
    def __init__(self, code: int, msg: str):
        super().__init__(f"{msg} (status {code})")
        self.code = code


def _lib():
    L = _capi.load()
    if not getattr(L, "_flac_bound", False):
        for name, res, args in SYMBOLS:
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        L._flac_bound = True
    return L


def _buf(data: bytes):
    return (C.c_char * max(1, len(data))).from_buffer_copy(data if data else b"\0")


def is_flac(data: bytes) -> bool:
    return bool(_lib().rg_flac_is_flac(_buf(data), len(data)))


def scan(data: bytes) -> FlacInfo:
    L = _lib()
    info = FlacInfo()
    rc = L.rg_flac_scan(_buf(data), len(data), C.byref(info))
    if rc != OK:
        raise FlacError(rc, L.rg_flac_last_error().decode())
    return info


def index(data: bytes) -> Tuple[List[FlacFrame], FlacInfo]:
    """The frame walk the device route uses: ([rg_flac_frame], info)."""
    L = _lib()
    info = FlacInfo()
    n = C.c_size_t()
    buf = _buf(data)
    rc = L.rg_flac_index_frames(buf, len(data), None, 0, C.byref(n), C.byref(info))
    if rc not in (OK, ERR_CAPACITY):
        raise FlacError(rc, L.rg_flac_last_error().decode())
    frames = (FlacFrame * max(1, n.value))()
    rc = L.rg_flac_index_frames(buf, len(data), frames, n.value, C.byref(n), C.byref(info))
    if rc != OK:
        raise FlacError(rc, L.rg_flac_last_error().decode())
    return list(frames[:n.value]), info


def decode(data: bytes) -> Tuple[int, int, np.ndarray, FlacInfo]:
    """-> (sample rate, bits per sample, int32 [channels][samples], info)."""
    L = _lib()
    _, info = index(data)
    cap = int(info.frames)
    out = np.zeros((int(info.channels), max(1, cap)), dtype=np.int32)
    planes = (C.c_void_p * int(info.channels))(*[out[c].ctypes.data for c in range(int(info.channels))])
    di = FlacInfo()
    rc = L.rg_flac_decode_s32(_buf(data), len(data), planes, cap, C.byref(di))
    if rc != OK:
        raise FlacError(rc, L.rg_flac_last_error().decode())
    return int(di.sample_rate), int(di.bits_per_sample), out[:, :int(di.frames)], di


def decode_arena(data: bytes) -> Tuple[List[np.ndarray], FlacInfo]:
    """rg_flac_decode_arena, the host twin of the device decoder's output stage: the stream decoded through the arena sink
    -> ([plane per channel: int16 (<= 16 bits per sample, << 16 - bps) or int32 (<< 32 - bps)], info)."""
    L = _lib()
    _, info = index(data)
    ch = int(info.channels)
    eb = 2 if info.bits_per_sample <= 16 else 4
    arena = np.zeros(max(1, int(info.frames) * ch * eb), dtype=np.uint8)
    di = FlacInfo()
    got_eb = C.c_uint32()
    rc = L.rg_flac_decode_arena(_buf(data), len(data), arena.ctypes.data, arena.size, C.byref(got_eb), C.byref(di))
    if rc != OK:
        raise FlacError(rc, L.rg_flac_last_error().decode())
    assert got_eb.value == eb
    n = int(di.frames)
    dt = np.int16 if eb == 2 else np.int32
    return [arena[c * n * eb:(c + 1) * n * eb].view(dt) for c in range(ch)], di


def selfcheck(data: bytes) -> int:
    """rg_flac_index_selfcheck: 0 = the index and the decoder agree, 1 = they do not, < 0 = not decodable."""
    return int(_lib().rg_flac_index_selfcheck(_buf(data), len(data)))


def stream_md5(data: bytes):
    """STREAMINFO's MD5 signature (rg_flac_stream_md5): the 16 bytes, or None when the field is all zero (no signature)."""
    L = _lib()
    out = (C.c_uint8 * 16)()
    rc = L.rg_flac_stream_md5(_buf(data), len(data), out)
    if rc < 0:
        raise FlacError(rc, L.rg_flac_last_error().decode())
    return bytes(out) if rc == 1 else None


def md5_planes(planes, bps: int) -> bytes:
    """rg_flac_md5_s32: the signature of right-justified PCM, `planes` = [channels][frames] integers of `bps` bits."""
    L = _lib()
    arr = np.ascontiguousarray(planes, dtype=np.int32)
    if arr.ndim != 2:
        raise ValueError("planes must be [channels][frames]")
    ch, n = arr.shape
    ptrs = (C.c_void_p * max(1, ch))(*[arr[c].ctypes.data for c in range(ch)])
    out = (C.c_uint8 * 16)()
    rc = L.rg_flac_md5_s32(ptrs, ch, n, int(bps), out)
    if rc != OK:
        raise FlacError(rc, f"rg_flac_md5_s32: {ch} channels of {bps} bits per sample")
    return bytes(out)


def md5_arena(ctx, route: int, descs, bps, arena: np.ndarray):
    """rg_flac_md5_arena: the streams `descs` ([TrackDesc], format S16 or S32 planar, left-justified) of `bps` ([int]) in the
    host arena `arena` (uint8) -> [16 digest bytes per stream].  route 0: the host twin (`ctx` may be None), route 1: the kernel."""
    L = _lib()
    n = len(descs)
    arena = np.ascontiguousarray(arena, dtype=np.uint8)
    d = (_capi.TrackDesc * max(1, n))(*descs)
    b = (C.c_uint32 * max(1, n))(*[int(x) for x in bps])
    out = (C.c_uint8 * (16 * max(1, n)))()
    rc = L.rg_flac_md5_arena(ctx, int(route), n, d, b, arena.ctypes.data if arena.size else None, arena.size, out)
    if rc != OK:
        raise FlacError(rc, _capi.load().rg_last_error(ctx).decode())
    raw = bytes(out)
    return [raw[16 * i:16 * i + 16] for i in range(n)]
