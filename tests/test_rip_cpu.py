"""The rip checksums without a GPU (include/mp3rgain_amd_rip.h): the serial host twin (route 0) and the kernels' fold
arithmetic run on the host (route 2) against the Python restatement of the definitions (tests/rip_cases.py: zlib.crc32, numpy
and a plain loop), the CRC-32 algebra of rg_crc32.h against a bit-by-bit CRC, the argument checks, and the rip log reader on
logs the test writes itself.  No tolerance anywhere.  tests/test_gpu_rip.py holds the kernels (route 1) to the same cases."""
import ctypes as C
import sys
import zlib
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import arena_layouts as al  # noqa: E402
import rip_cases as rc  # noqa: E402

from mp3rgain_amd import _capi, riplog  # noqa: E402
from mp3rgain_amd import replaygain as rg  # noqa: E402

RG_ERR_INVALID_ARG, RG_ERR_FORMAT = -1, -9
POLY = 0xEDB88320


def test_record_is_48_bytes(capi):
    assert C.sizeof(_capi.RipRecord) == 48
    assert _capi.RipRecord.crc32.offset == 32 and _capi.RipRecord.arv2.offset == 44 and _capi.RipRecord.null_samples.offset == 16


def test_kernel_shape_is_usable(capi):
    c, t, f = rc.shape()
    assert c >= 1 and t % c == 0 and t > c and f >= 2
    assert max(rc.lengths()) == f * t + t + 1 and max(rc.lengths()) * 4 < 16 << 20  # a few MB at the most


@pytest.mark.parametrize("route", [0, 2], ids=["serial", "folded"])
def test_host_routes_match_the_restatement(capi, route):
    """Every case and every flag combination, field by field, from an arena with loud guards around sample-aligned tracks."""
    cases, wants = rc.cases(), rc.wants()
    arena, descs, guards = al.pack(rc.tracks(cases), al.Layout("guard", "loud", "input", 3))
    descs = list(descs)[:len(cases)]
    assert any(d.offset_bytes % 4 == 2 for d in descs) and guards
    bad = []
    for fl in rc.ALL_FLAGS:
        out = rg.rip_checksums_arena(None, route, descs, [fl] * len(cases), arena)
        for cs, r in zip(cases, out):
            n = len(cs.left)
            assert (r.status, r.frames, r.sample_rate, r.dropped_frames) == (0, n, 44100, 0)
            assert r.flags == _capi.RIP_CD_RATE | _capi.RIP_COMPLETE | (_capi.RIP_CD_FRAMES if n % 588 == 0 else 0)
            if rc.got(r) != wants[(cs.name, fl)]:
                bad.append((cs.name, fl, rc.got(r), wants[(cs.name, fl)]))
    assert not bad, f"{len(bad)} records differ from the restatement: {bad[:4]}"
    # flags = NULL is all 0
    out = rg.rip_checksums_arena(None, route, descs, None, arena)
    assert [rc.got(r) for r in out] == [wants[(cs.name, 0)] for cs in cases]


def test_range_may_be_empty(capi):
    """A first-and-last track shorter than 2 * 2940 frames: `to` < `from`, both sums 0, the CRCs untouched."""
    cs = next(c for c in rc.cases() if c.name == "random_5879")
    w = rc.wants()[(cs.name, rc.FIRST | rc.LAST)]
    assert (w.arv1, w.arv2) == (0, 0) and w.crc32 == rc.wants()[(cs.name, 0)].crc32 != 0
    cs = next(c for c in rc.cases() if c.name == "random_5880")  # one position counts: i = 2940
    w = rc.wants()[(cs.name, rc.FIRST | rc.LAST)]
    v = (int(cs.left[2939]) & 0xFFFF) | ((int(cs.right[2939]) & 0xFFFF) << 16)
    assert w.arv1 == (v * 2940) & 0xFFFFFFFF


# ---- rg_crc32.h ------------------------------------------------------------------------------------------------------------------
def _bitwise_raw(data: bytes, reg: int = 0) -> int:
    """The CRC register bit by bit: reflected, no final XOR."""
    for b in data:
        reg ^= b
        for _ in range(8):
            reg = (reg >> 1) ^ (POLY if reg & 1 else 0)
    return reg


def _algebra(a, b, n):
    prod, power = C.c_uint32(), C.c_uint32()
    assert _capi.load().rg_rip_crc32_algebra(a, b, n, C.byref(prod), C.byref(power)) == 0
    return prod.value, power.value


def test_crc32_product_and_powers_match_a_bitwise_crc(capi):
    """x^(8n) is the register 0x80000000 (x^0) clocked through n zero bytes; a * x^(8n) is the register a clocked the same
    way; the product is commutative and x^0 is its one.  Then zlib's CRC from the raw register: the fix-up of rg_crc32.h."""
    rng = np.random.default_rng(5)
    one = 0x80000000
    for n in (0, 1, 2, 3, 4, 7, 8, 63, 64, 65, 1000, 4097):
        _, power = _algebra(0, 0, n)
        assert power == _bitwise_raw(bytes(n), one), n
        for a in (1, one, 0xFFFFFFFF, int(rng.integers(1, 1 << 32))):
            assert _algebra(a, power, 0)[0] == _bitwise_raw(bytes(n), a) == _algebra(power, a, 0)[0], (a, n)
            assert _algebra(a, one, 0)[0] == a
    # large exponents: x^(8 (m + n)) = x^(8 m) x^(8 n)
    for m, n in ((1 << 20, 12345), ((1 << 33) + 5, (1 << 31) - 1), (4 * ((1 << 32) - 1), 1)):
        assert _algebra(_algebra(0, 0, m)[1], _algebra(0, 0, n)[1], m + n) == (_algebra(0, 0, m + n)[1],) * 2
    for n in (1, 5, 64, 1001):
        msg = rng.integers(0, 256, n, dtype=np.uint8).tobytes()
        raw, (_, power) = _bitwise_raw(msg), _algebra(0, 0, n)
        assert (~(raw ^ _algebra(0xFFFFFFFF, power, 0)[0])) & 0xFFFFFFFF == zlib.crc32(msg)


def test_folded_route_on_crafted_lengths(capi):
    """Route 2 on lengths around every power the fold uses: one chunk more or less than 2^j chunks, tiles, and runs."""
    c, t, f = rc.shape()
    rng = np.random.default_rng(6)
    lens = sorted({c * (1 << j) + d for j in range(0, 9) for d in (-1, 0, 1)} | {t * k + d for k in (2, 3, f - 1, f, f + 1) for d in (-1, 1)})
    tracks = [rc.Track([rng.integers(-3, 4, n, dtype=np.int16), rng.integers(-3, 4, n, dtype=np.int16)], 48000) for n in lens]
    arena, descs, _ = al.pack(tracks, al.Layout("abut", "loud", "reversed"))
    flags = [rc.ALL_FLAGS[k % 4] for k in range(len(lens))]
    out = rg.rip_checksums_arena(None, 2, list(descs)[:len(lens)], flags, arena)
    for tr, fl, r in zip(tracks, flags, out):
        assert rc.got(r) == rc.want(tr.channels[0], tr.channels[1], fl), (len(tr.channels[0]), fl)
        assert not r.flags & _capi.RIP_CD_RATE
    assert rg.rip_checksums_arena(None, 0, list(descs)[:len(lens)], flags, arena)[0].crc32 == out[0].crc32


# ---- arguments --------------------------------------------------------------------------------------------------------------------
def test_argument_errors(capi):
    L = _capi.load()
    arena = np.zeros(64, dtype=np.uint8)
    out = (_capi.RipRecord * 1)()
    d = (_capi.TrackDesc * 1)(_capi.TrackDesc(0, 16, 44100, 2, _capi.FMT_S16_PLANAR))
    for route in (0, 2):
        assert L.rg_rip_checksums_arena(None, route, 1, d, None, arena.ctypes.data, 64, out) == 0
        assert L.rg_rip_checksums_arena(None, route, 1, None, None, arena.ctypes.data, 64, out) == RG_ERR_INVALID_ARG
        assert L.rg_rip_checksums_arena(None, route, 1, d, None, arena.ctypes.data, 64, None) == RG_ERR_INVALID_ARG
        assert L.rg_rip_checksums_arena(None, route, 1, d, None, None, 64, out) == RG_ERR_INVALID_ARG
        assert L.rg_rip_checksums_arena(None, route, 0, None, None, None, 0, None) == 0
        for desc, code, text in ((_capi.TrackDesc(0, 17, 44100, 2, _capi.FMT_S16_PLANAR), RG_ERR_INVALID_ARG, "beyond the arena"),
                                 (_capi.TrackDesc(2, 16, 44100, 2, _capi.FMT_S16_PLANAR), RG_ERR_INVALID_ARG, "beyond the arena"),
                                 (_capi.TrackDesc(66, 0, 44100, 2, _capi.FMT_S16_PLANAR), RG_ERR_INVALID_ARG, "beyond the arena"),
                                 (_capi.TrackDesc(1, 4, 44100, 2, _capi.FMT_S16_PLANAR), RG_ERR_INVALID_ARG, "sample-aligned"),
                                 (_capi.TrackDesc(0, 16, 44100, 1, _capi.FMT_S16_PLANAR), RG_ERR_FORMAT, "1 channel"),
                                 (_capi.TrackDesc(0, 4, 44100, 3, _capi.FMT_S16_PLANAR), RG_ERR_FORMAT, "3 channel"),
                                 (_capi.TrackDesc(0, 8, 44100, 2, _capi.FMT_S32_PLANAR), RG_ERR_FORMAT, "16-bit"),
                                 (_capi.TrackDesc(0, 8, 44100, 2, _capi.FMT_F32_PLANAR), RG_ERR_FORMAT, "16-bit"),
                                 (_capi.TrackDesc(0, 1 << 32, 44100, 2, _capi.FMT_S16_PLANAR), RG_ERR_FORMAT, "2^32")):
            with pytest.raises(rg.ReplayGainError) as e:
                rg.rip_checksums_arena(None, route, [desc], [0], arena)
            assert e.value.code == code and text in str(e.value), (desc.frames, desc.channels, str(e.value))
    assert L.rg_rip_checksums_arena(None, 1, 1, d, None, arena.ctypes.data, 64, out) == RG_ERR_INVALID_ARG  # the kernels need a context
    assert L.rg_rip_checksums_arena(None, 3, 1, d, None, arena.ctypes.data, 64, out) == RG_ERR_INVALID_ARG
    # a track may end at the arena's last byte
    assert rc.got(rg.rip_checksums_arena(None, 0, [_capi.TrackDesc(32, 8, 44100, 2, _capi.FMT_S16_PLANAR)], [0], arena)[0]).null_samples == 16


# ---- the log reader ---------------------------------------------------------------------------------------------------------------
class _Sums:
    crc32, crc32_nonnull, arv1, arv2 = 0x1A2B3C4D, 0x0BADF00D, 0x9F3B1C22, 0x00C0FFEE


def _eac_log(crcs):
    head = "Exact Audio Copy V1.6 from 23. October 2020\r\n\r\nEAC extraction logfile\r\n\r\nUsed drive  : HL-DT-ST\r\n\r\n"
    body = ""
    for k, crc in enumerate(crcs):
        body += (f"Track {k + 1:2d}\r\n\r\n     Filename C:\\rip\\{k + 1:02d} - deadbeef cafebabe.wav\r\n\r\n     Peak level 98.8 %\r\n"
                 f"     Track quality 100.0 %\r\n     Test CRC 11111111\r\n     Copy CRC {crc:08X}\r\n     Copy OK\r\n\r\n")
    return head + body + "No errors occurred\r\n\r\nEnd of status report\r\n"


def _xld_log(tracks):
    out = "X Lossless Decoder version 20210101 (153.1)\n\nXLD extraction logfile\n\nAll Tracks\n    Statistics\n        Read error : 0\n\n"
    for k, (crc, skip, v1, v2) in enumerate(tracks):
        out += (f"Track {k + 1:02d}\n    Filename : /rip/{k + 1:02d}.flac\n    CRC32 hash               : {crc:08X}\n"
                f"    CRC32 hash (skip zero)   : {skip:08X}\n    AccurateRip v1 signature : {v1:08X}\n"
                f"    AccurateRip v2 signature : {v2:08X}\n        ->Accurately ripped (v1+v2, confidence 5/5)\n    Statistics\n        Read error : 0\n\n")
    return out + "No errors occurred\n\nEnd of status report\n"


def test_log_reader_eac_shape_utf16_copy_crc_matches_either_crc():
    s = _Sums()
    text = _eac_log([s.crc32, s.crc32_nonnull, 0x22222222])
    for data in (b"\xff\xfe" + text.encode("utf-16-le"), b"\xfe\xff" + text.encode("utf-16-be"), text.encode("utf-8")):
        tr = riplog.parse(data)
        assert [t.number for t in tr] == [1, 2, 3]
        assert [t.copy_crc for t in tr] == [s.crc32, s.crc32_nonnull, 0x22222222]
        assert all((t.crc32, t.crc32_skip_zero, t.arv1, t.arv2) == (None,) * 4 for t in tr)
        v = [riplog.compare(t, s) for t in tr]
        assert [x.ok for x in v] == [True, True, False] and v[0].text == "match" and v[2].text == "mismatch: Copy CRC"


def test_log_reader_xld_shape_and_missing_section():
    s = _Sums()
    text = _xld_log([(s.crc32, s.crc32_nonnull, s.arv1, s.arv2), (s.crc32, s.crc32, s.arv1, s.arv2 ^ 1)])
    tr = riplog.parse(text.encode("utf-8"))
    assert len(tr) == 2 and (tr[0].crc32, tr[0].crc32_skip_zero, tr[0].arv1, tr[0].arv2) == (s.crc32, s.crc32_nonnull, s.arv1, s.arv2)
    assert tr[0].copy_crc is None and riplog.compare(tr[0], s).ok
    v = riplog.compare(tr[1], s)
    assert not v.ok and v.text == "mismatch: CRC32 hash (skip zero), AccurateRip v2"
    # a section lost: one section for two files is the caller's to notice; a log without sections gives none
    assert len(riplog.parse(_xld_log([(1, 2, 3, 4)]).encode())) == 1 and riplog.parse(b"no tracks here\nTrack quality 100 %\n") == []
    # bytes that are not UTF-8 are replaced, not fatal; a section without values compares as nothing
    tr = riplog.parse(b"Track 7\n    Filename : \xff\xfe\xfd.flac\n")
    assert len(tr) == 1 and tr[0].number == 7 and riplog.compare(tr[0], s).text == "nothing to compare"
