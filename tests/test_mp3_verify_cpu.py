"""The host side of MP3 verification (include/mp3rgain_amd_mp3verify.h): the info-tag parser, the host twin of both CRCs
(route 0 of the seams), the kernels' fold arithmetic run on the host, and the record rg_mp3_verify_data fills -- against a
bit-by-bit Python CRC (tests/mp3_verify_cases.py) that shares no table with the C code, and against the recorded numbers of
the reference's fixtures (tests/golden/mp3_verify_expected.json).  No tolerance anywhere."""
import json
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import mp3_verify_cases as vc  # noqa: E402

from mp3rgain_amd import mp3dec, mp3verify as mv  # noqa: E402

EXPECTED = json.loads((Path(__file__).resolve().parent / "golden" / "mp3_verify_expected.json").read_text())


def test_oracle_check_values():
    assert vc.crc16_arc(b"123456789") == 0xBB3D and vc.crc16_arc(b"") == 0
    assert vc.crc16_mpeg(b"123456789") == 0xAEE7  # CRC-16/CMS: poly 0x8005, init 0xFFFF, not reflected
    assert vc.crc16_arc(bytes(5) + b"123456789") == 0xBB3D  # leading zeros leave it unchanged


@pytest.mark.parametrize("name", ["test_joint_stereo.mp3", "test_vbr.mp3", "test_mono.mp3", "test_stereo.mp3"])
def test_fixture_reads_what_was_recorded(capi, name):
    want = EXPECTED[name]
    data = (vc.FIXTURES / name).read_bytes()
    t = mv.info_tag(data)
    r = mv.verify_data(data)
    assert r.error is None and t.info_frame == 1 and t.has_lame_ext == 1
    assert t.tag_frame_offset == want["id3v2_bytes"] == 44 and r.xing_frames == want["xing_frames"] == 40
    assert r.music_length == want["music_length"] and r.encoder.startswith("Lavc")
    assert r.music_crc_stored == int(want["music_crc_stored"], 16) and r.music_crc_computed == int(want["music_crc_computed"], 16)
    # the oracle over the same range
    end = min(len(data), 44 + r.music_length)
    assert r.music_crc_computed == vc.crc16_arc(data[44 + t.tag_frame_bytes:end]) and r.audio_bytes == end - 44 - t.tag_frame_bytes
    assert r.verdict == want["verdict"] and r.dropped_frames == 0 and r.flag("complete") and r.flag("frame_crcs_ok")
    if name == "test_stereo.mp3":
        assert len(data) == want["file_bytes"] == 17173 and 44 + r.music_length == len(data) + 6
        assert not r.flag("length_match") and not r.flag("music_crc_match") and r.music_crc_computed == 0x5B8F
        assert r.failed and not r.verified
        return
    assert r.verified and r.flags == vc.ALL_GOOD and r.audio_frames == want["audio_frames"] == 40
    assert r.tag_crc_stored == int(want["tag_crc_stored"], 16) == r.tag_crc_computed == int(want["tag_crc_190"], 16)
    frame = bytearray(data[44:44 + 190])
    field = t.ext_offset + 34
    if field < 190:
        frame[field:field + 2] = b"\0\0"
    assert len(frame) == 190 and vc.crc16_arc(bytes(frame)) == int(want["tag_crc_190"], 16)
    if name == "test_mono.mp3":  # libavformat's rule only: LAME's gives another value
        assert field == 175 and vc.crc16_arc(data[44:44 + field]) == int(want["tag_crc_lame_rule"], 16) != r.tag_crc_stored
        assert r.flag("tag_crc_match")


@pytest.mark.parametrize("path", vc.DENSE, ids=lambda p: p.stem)
def test_dense_goldens_carry_no_checksum(capi, path):
    data = path.read_bytes()
    r = mv.verify_data(data)
    _, info = mp3dec.decode(data)
    assert r.verdict == "no checksum" and not r.failed and r.flag("complete") and r.info_frame == 0
    assert r.flags == vc.F["complete"] | vc.F["frame_crcs_ok"] and r.audio_frames == info.audio_frames + info.skipped_frames
    assert r.dropped_frames == info.skipped_frames == 0


def test_host_twin_of_the_music_crc(capi):
    """Route 0 over every length the chunking cares about and start offsets of every residue mod 8."""
    lengths = vc.LENGTHS + [vc.L - 1, vc.L + 1, 3, 2 * vc.L, 7, 5, 1, 2, 6, 9, 11, 13]
    r = vc.ranges(lengths, 7)
    assert {o % 8 for o in r.offsets} == set(range(8)) and r.offsets[0] == 0 and r.offsets[-1] + r.lengths[-1] == r.data.size
    assert mv.crc_ranges(None, 0, r.offsets, r.lengths, r.data) == vc.expect(r)
    with pytest.raises(mv.Mp3VerifyError):
        mv.crc_ranges(None, 0, [r.data.size - 3], [4], r.data)
    with pytest.raises(mv.Mp3VerifyError):
        mv.crc_ranges(None, 0, [r.data.size + 1], [0], r.data)
    assert mv.crc_ranges(None, 0, [r.data.size], [0], r.data) == [0]


def test_fold_arithmetic_equals_the_serial_crc(capi):
    """Chunked and combined equals serial: the kernels' arithmetic (csrc/rg_crc16.h: rg_crc16_mul, rg_crc16_x8n, the trees) on
    the host, at the lengths where a chunk, a tile or a run of tiles begins, and one long enough for runs of two tiles."""
    rng = np.random.default_rng(3)
    for n in vc.LENGTHS + [vc.TILE, vc.TILE + 1, 2 * vc.TILE - 1, 256 * vc.TILE + 1, 257 * vc.TILE + 77]:
        data = rng.integers(0, 256, size=n, dtype=np.uint8)
        want = mv.crc_ranges(None, 0, [0], [n], data)[0]
        if n <= 300 * vc.L + 17:
            assert want == vc.crc16_arc(data.tobytes())
        assert mv.crc_folded_host(data.tobytes()) == want, n


def test_host_twin_of_the_frame_crc(capi):
    data, offs, ok = vc.protected_frames(300, 11)
    assert offs[-1] + 6 + 32 >= data.size - 1 and sum(ok) == 270
    assert mv.frame_crc_check(None, 0, offs, data) == ok
    # the oracle agrees with the construction
    raw = data.tobytes()
    assert [int(vc.frame_crc_ok(raw[o:o + 40])) for o in offs] == ok
    # an unprotected frame, an invalid header and side information beyond the buffer are failures, not faults
    f = bytearray(raw[offs[0]:offs[0] + 40])
    f[1] |= 1
    assert mv.frame_crc_check(None, 0, [0], np.frombuffer(bytes(f), dtype=np.uint8)) == [0]
    f[1] &= 0xFE
    f[2] |= 0xF0
    assert mv.frame_crc_check(None, 0, [0], np.frombuffer(bytes(f), dtype=np.uint8)) == [0]
    assert mv.frame_crc_check(None, 0, [offs[-1]], data[:offs[-1] + 8]) == [0]
    with pytest.raises(mv.Mp3VerifyError):
        mv.frame_crc_check(None, 0, [data.size - 5], data)


def test_a_stream_of_the_writer_carries_the_frame_crc_the_oracle_computes(capi):
    """oracle/mp3_bitstream.py writes the CRC word; both the Python oracle and the library read it as correct."""
    frames = vc.stream(44100, 1, 6, True, 5, 128)
    raw = b"".join(frames)
    offs = [i * len(frames[0]) for i in range(6)]
    assert all(vc.frame_crc_ok(f) for f in frames)
    assert mv.frame_crc_check(None, 0, offs, np.frombuffer(raw, dtype=np.uint8)) == [1] * 6


def _check(c: vc.Case):
    r = mv.verify_data(c.data)
    assert r.error is None, c.name
    assert (hex(r.flags), r.verdict) == (hex(c.flags), c.verdict), c.name
    assert (r.audio_frames, r.protected_frames, r.frame_crc_failed, r.dropped_frames) == (c.audio_frames, c.protected_frames, c.frame_crc_failed, c.dropped_frames), c.name
    assert r.music_crc_computed == c.music_crc_computed, c.name
    _, info = mp3dec.decode(c.data)
    assert r.dropped_frames == info.skipped_frames, c.name


def test_written_info_tags_verify(capi):
    """Flag sets 15, 7 and 1; MPEG-1 / MPEG-2, stereo / mono; protected and unprotected tag frames; LAME's and libavformat's
    tag-CRC rule; streams with and without frame CRCs."""
    cases = vc.clean_cases()
    assert len(cases) == 24 and any(c.protected_frames for c in cases) and any(not c.protected_frames for c in cases)
    for c in cases:
        _check(c)
        t = mv.info_tag(c.data)
        assert t.has_lame_ext and t.xing_frames == vc.N_FRAMES and t.encoder[:4] in (b"LAME", b"Lavc")


def test_damage_reads_as_the_definitions_say(capi):
    cases = vc.damaged_cases()
    assert {c.verdict for c in cases} >= {"music CRC mismatch", "1 frames dropped", "1 frame CRCs failed", "length mismatch", "gain applied, CRC not comparable",
                                          "info tag CRC mismatch", "frame count mismatch", "no checksum", "verified"}
    for c in cases:
        _check(c)
        r = mv.verify_data(c.data)
        assert r.failed == (c.verdict not in ("verified", "no checksum", "gain applied, CRC not comparable")), c.name


def test_an_extension_of_another_encoder_does_not_count(capi):
    tag, frames = vc.clean("v1_stereo", False, False, 15, 9, encoder=b"GOGO3.13 ")
    r = mv.verify_data(tag + b"".join(frames))
    assert r.verdict == "no checksum" and r.flag("has_info_tag") and not r.flag("has_lame_ext") and r.flag("frame_count_match")


def test_a_vbri_frame_is_named_by_its_own_marker(capi):
    """A header frame with "VBRI" at byte 36 reads info_frame = 2 and no fields; where the side information ends at byte 36 the
    same four bytes "Info" there read info_frame = 1.  Either way no checksum, and the frame is not counted as audio."""
    for kind, marker, want in (("v1_mono", b"VBRI", 2), ("v2_stereo", b"VBRI", 2), ("v1_stereo", b"Info", 1)):
        tag, frames = vc.clean(kind, False, False, 0, 11, marker=bytes(4), with_ext=False)
        tag = tag[:36] + marker + tag[40:]
        data = tag + b"".join(frames)
        t = mv.info_tag(data)
        assert (t.info_frame, t.has_lame_ext, t.has_frames, t.tag_frame_bytes) == (want, 0, 0, len(tag)), kind
        r = mv.verify_data(data)
        assert (r.info_frame, r.verdict, r.audio_frames) == (want, "no checksum", vc.N_FRAMES) and r.flag("has_info_tag") and r.flag("complete"), kind


def test_what_is_not_a_bare_mpeg_stream_is_refused(capi):
    import flacenc
    from wavutil import test_signal, wav_bytes

    wav = wav_bytes(test_signal("s16", 44100, 2000, 2, 1), 44100, "s16")
    pcm = np.zeros((1, 64), dtype=np.int32)
    for blob in (wav, flacenc.encode(pcm, 44100, 16), b"\0\0\0\x18ftypM4A " + bytes(64), bytes(4096), b""):
        r = mv.verify_data(bytes(blob))
        assert r.error is not None and r.error.code == -9 and r.flags == 0
        assert mv.verify_data_raw(bytes(blob))[4:] == bytes(68)
