"""The host side of the FLAC MD5 feature (include/mp3rgain_amd_flac.h): rg_flac_md5_s32, rg_flac_stream_md5 and route 0 of
rg_flac_md5_arena -- the host twin that shares its code with the device kernel (csrc/rg_md5.h) -- against hashlib.md5 over
NumPy-packed bytes (tests/flac_md5_cases.py), which shares nothing with the code under test.  No tolerance anywhere."""
import hashlib
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import flac_md5_cases as mc  # noqa: E402
import flacenc  # noqa: E402

from mp3rgain_amd import _capi, flacdec  # noqa: E402

GOLD = Path(__file__).resolve().parent / "golden" / "flac"


@pytest.fixture(scope="module")
def matrix(capi):
    return mc.matrix()


def test_oracle_packing():
    """The packing itself, on values whose bytes are known."""
    assert mc.pack([[1, -2]], 16) == b"\x01\x00\xfe\xff"
    assert mc.pack([[1], [-2]], 12) == b"\x01\x00\xfe\xff"             # two channels, one frame
    assert mc.pack([[-8, 7]], 4) == b"\xf8\x07"
    assert mc.pack([[-(1 << 23), 0x123456]], 24) == b"\x00\x00\x80\x56\x34\x12"
    assert mc.pack([[-1]], 17) == b"\xff\xff\xff"
    assert mc.md5(np.zeros((2, 0), dtype=np.int32), 16) == hashlib.md5(b"").digest()


def test_matrix_covers_the_padding_cases(matrix):
    lengths = {len(mc.pack(s.pcm, s.bps)) for s in matrix}
    assert {n % 64 for n in lengths} >= set(mc.RESIDUES)
    assert {0, 64} <= lengths and any(n > 64 and n % 64 == 0 for n in lengths)
    assert {s.bps for s in matrix} == set(mc.BPS) and {s.pcm.shape[0] for s in matrix} == set(mc.CHANNELS)
    for s in matrix:
        if s.pcm.size >= 3:
            assert {-(1 << (s.bps - 1)), (1 << (s.bps - 1)) - 1, -1} <= set(s.pcm.reshape(-1).tolist()), s.name


def test_md5_s32_matches_hashlib(matrix):
    for s in matrix:
        assert flacdec.md5_planes(s.pcm, s.bps) == mc.md5(s.pcm, s.bps), s.name


def test_md5_s32_rejects_what_it_does_not_hash(capi):
    z = np.zeros((1, 4), dtype=np.int32)
    for bps in (3, 25, 32):
        with pytest.raises(flacdec.FlacError):
            flacdec.md5_planes(z, bps)
    with pytest.raises(flacdec.FlacError):
        flacdec.md5_planes(np.zeros((9, 4), dtype=np.int32), 16)


def _with_signature(stream: bytes, sig: bytes, at: int = 0) -> bytes:
    """`stream` with `sig` in STREAMINFO's MD5 field: bytes 26..42 behind "fLaC" (which is at `at`)."""
    assert stream[at:at + 4] == b"fLaC" and len(sig) == 16
    return stream[:at + 26] + sig + stream[at + 42:]


def test_stream_md5(capi):
    rng = np.random.default_rng(3)
    pcm = flacenc.test_pcm(rng, 2, 1000, 16)
    stream = flacenc.encode(pcm, 44100, 16)
    assert stream[26:42] == bytes(16)
    assert flacdec.stream_md5(stream) is None
    gold = (GOLD / "s16_stereo_44k_alt.flac").read_bytes()
    assert flacdec.stream_md5(gold) is None
    sig = mc.md5(pcm, 16)
    assert flacdec.stream_md5(_with_signature(stream, sig)) == sig
    tag = flacenc.id3v2_tag()
    assert flacdec.stream_md5(tag + _with_signature(stream, sig)) == sig
    assert flacdec.stream_md5(tag + stream) is None
    one = bytes(15) + b"\x01"  # a signature whose only set bit is in its last byte is a signature
    assert flacdec.stream_md5(_with_signature(stream, one)) == one
    assert flacdec.scan(_with_signature(stream, sig)).as_dict() == flacdec.scan(stream).as_dict()
    with pytest.raises(flacdec.FlacError) as ei:
        flacdec.stream_md5(b"RIFF" + bytes(60))
    assert ei.value.code == flacdec.ERR_NOT_FLAC


@pytest.mark.parametrize("stereo", ["independent", "left_side", "right_side", "mid_side", "alternate"])
def test_encode_decode_md5_stereo(capi, stereo):
    rng = np.random.default_rng(5)
    pcm = flacenc.test_pcm(rng, 2, 3 * 1152 + 77, 16)
    stream = flacenc.encode(pcm, 44100, 16, flacenc.Options(block_size=1152, stereo=stereo))
    _, bps, got, info = flacdec.decode(stream)
    assert info.dropped_frames == 0 and bps == 16
    assert flacdec.md5_planes(got, bps) == mc.md5(pcm, 16)


def test_encode_decode_md5_six_channels(capi):
    rng = np.random.default_rng(6)
    pcm = flacenc.test_pcm(rng, 6, 2 * 576 + 5, 24)
    stream = flacenc.encode(pcm, 48000, 24, flacenc.Options(block_size=576))
    _, bps, got, info = flacdec.decode(stream)
    assert info.dropped_frames == 0 and bps == 24
    assert flacdec.md5_planes(got, bps) == mc.md5(pcm, 24)


def _descs(a):
    return [_capi.TrackDesc(off, frames, 44100, ch, fmt) for off, frames, ch, fmt in a.descs]


def test_arena_route0_matches_hashlib(matrix):
    """The host twin reading the arena's left-justified form, in the layout the kernel test uses: sample-aligned offsets,
    guards in the gaps, abutting streams, byte 0 and the last byte in use."""
    streams = mc.gpu_streams()
    a = mc.arena(streams)
    assert a.descs[0][0] == 0 and a.descs[-1][0] + len(mc.planes_bytes(streams[-1])) == a.bytes.size
    assert any(off % 4 == 2 and frames % 2 == 1 and ch > 1 for off, frames, ch, fmt in a.descs if fmt == mc.FMT_S16)
    ends = {off + len(mc.planes_bytes(s)) for (off, *_), s in zip(a.descs, streams) if s.pcm.size}
    assert any(off in ends for off, frames, *_ in a.descs[1:] if frames), "no two streams abut"
    bps = [s.bps for s in streams]
    got = flacdec.md5_arena(None, 0, _descs(a), bps, a.bytes)
    for s, g in zip(streams, got):
        assert g == mc.md5(s.pcm, s.bps), s.name
    other = a.bytes.copy()
    other[a.guards] ^= 0xA5
    assert a.guards.any() and flacdec.md5_arena(None, 0, _descs(a), bps, other) == got


def test_arena_refuses_streams_outside_it(capi):
    arena = np.zeros(64, dtype=np.uint8)
    ok = _capi.TrackDesc(0, 8, 44100, 2, mc.FMT_S32)  # 8 frames * 2 channels * 4 bytes: exactly the arena
    assert flacdec.md5_arena(None, 0, [ok], [24], arena) == [hashlib.md5(bytes(48)).digest()]
    for bad, bps in ((_capi.TrackDesc(0, 9, 44100, 2, mc.FMT_S32), 24),        # one frame too many
                     (_capi.TrackDesc(4, 8, 44100, 2, mc.FMT_S32), 24),        # pushed past the end
                     (_capi.TrackDesc(2, 1, 44100, 1, mc.FMT_S32), 24),        # not sample-aligned
                     (_capi.TrackDesc(1, 1, 44100, 1, mc.FMT_S16), 16),
                     (_capi.TrackDesc(0, 1, 44100, 1, mc.FMT_S16), 17),        # 17 bits do not fit a 16-bit element
                     (_capi.TrackDesc(0, 1, 44100, 1, 0), 16),                 # float planes
                     (_capi.TrackDesc(0, 1 << 62, 44100, 8, mc.FMT_S32), 24),  # frames * channels * 4 wraps
                     (_capi.TrackDesc(1 << 40, 0, 44100, 1, mc.FMT_S16), 16)):
        with pytest.raises(flacdec.FlacError):
            flacdec.md5_arena(None, 0, [bad], [bps], arena)
