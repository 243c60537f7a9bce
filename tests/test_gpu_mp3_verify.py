"""MP3 verification on the GPU (include/mp3rgain_amd_mp3verify.h): the CRC-16/ARC chunk and fold kernels and the frame-CRC
kernel through their seams (route 1) on bytes of the test's own choosing, rg_mp3_verify on files, its equality across decode
routes and groups, and `--verify` of the command line on a mixed list.  The oracle is the bit-by-bit Python CRC of
tests/mp3_verify_cases.py; no tolerance anywhere.  tests/test_mp3_verify_cpu.py proves the same cases on the host twin."""
import io
import json
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import flac_md5_cases as mc  # noqa: E402
import flacenc  # noqa: E402
import mp3_verify_cases as vc  # noqa: E402
import wavutil  # noqa: E402

from mp3rgain_amd import mp3dec, mp3verify as mv  # noqa: E402

pytestmark = pytest.mark.gpu

RG_ERR_INVALID_ARG, RG_ERR_IO, RG_ERR_FORMAT = -1, -8, -9
CASES = Path(__file__).resolve().parent / "golden" / "mp3_cases"
REC = 72  # sizeof(rg_mp3_verify_result)


@pytest.fixture()
def an(_ctx):
    _ctx.set_tuning(6, 3)
    _ctx.set_tuning(13, 0)
    _ctx.set_decoder_command(None)
    yield _ctx
    _ctx.set_tuning(6, 3)
    _ctx.set_tuning(13, 0)


def crc16_arc_many(data: np.ndarray, offsets, lengths):
    """The bit-by-bit CRC-16/ARC of many ranges at once: the ranges right-aligned in one matrix (leading zeros leave the CRC
    unchanged), one byte column at a time, eight shift-and-xor steps per byte.  No table."""
    n, width = len(offsets), max(lengths) if lengths else 0
    m = np.zeros((n, width), dtype=np.uint16)
    for i, (o, k) in enumerate(zip(offsets, lengths)):
        m[i, width - k:] = data[o:o + k]
    crc = np.zeros(n, dtype=np.uint16)
    for col in range(width):
        crc ^= m[:, col]
        for _ in range(8):
            crc = (crc >> 1) ^ (np.uint16(0xA001) * (crc & 1))
    return [int(x) for x in crc]


# ---- the kernels, through the seams -------------------------------------------------------------------------------------------
def test_chunk_and_fold_kernels_match_the_bitwise_crc(an):
    """One launch of about 300 ranges: every length at which a chunk or a tile begins or ends, one of a few hundred chunks,
    random lengths up to 40 000 (up to three tiles), offsets that are only byte-aligned, abutting ranges, the buffer's first
    and last byte in use, guard bytes between ranges.  Rewriting the guards changes nothing; the host twin gives the same."""
    rng = np.random.default_rng(31)
    lengths = vc.LENGTHS + [int(x) for x in rng.integers(0, 40001, size=289)] + [vc.TILE, 2 * vc.TILE + 1]
    rng.shuffle(lengths)
    r = vc.ranges(lengths, 32)
    assert len(lengths) >= 300 and r.offsets[0] == 0 and r.offsets[-1] + r.lengths[-1] == r.data.size
    assert {o % 8 for o in r.offsets} == set(range(8)) and {o % 16 for o in r.offsets} == set(range(16))
    assert any(a + n == b and n for a, n, b in zip(r.offsets, r.lengths, r.offsets[1:])) and r.guards.sum() > 300
    want = crc16_arc_many(r.data, r.offsets, r.lengths)
    assert want[:3] == [vc.crc16_arc(r.data[o:o + n].tobytes()) for o, n in zip(r.offsets[:3], r.lengths[:3])]
    got = an.mp3_crc_ranges(1, r.offsets, r.lengths, r.data)
    bad = [(o, n) for o, n, g, w in zip(r.offsets, r.lengths, got, want) if g != w]
    assert not bad, f"{len(bad)} of {len(want)} CRCs differ from the bitwise CRC: {bad[:8]}"
    other = r.data.copy()
    other[r.guards] ^= 0x5A
    assert an.mp3_crc_ranges(1, r.offsets, r.lengths, other) == got
    assert an.mp3_crc_ranges(0, r.offsets, r.lengths, r.data) == got


def test_fold_kernel_folds_runs_of_tiles(an):
    """More than 256 tiles in one range: each lane of the fold kernel folds a run of two tile CRCs.  The range of 257 tiles is
    held to a serial byte-table CRC whose table the test builds from the bitwise CRC (the bitwise one itself would take a minute
    over 4 MB), the one-tile range to the bitwise CRC; for the other two the reference is the host twin, which
    tests/test_mp3_verify_cpu.py holds to the bitwise CRC at this size."""
    rng = np.random.default_rng(33)
    data = rng.integers(0, 256, size=300 * vc.TILE + 12345, dtype=np.uint8)
    offs, lens = [0, 3, data.size - vc.TILE, 5], [data.size, 257 * vc.TILE + 1, vc.TILE, 256 * vc.TILE]
    got = an.mp3_crc_ranges(1, offs, lens, data)
    table = [vc.crc16_arc(bytes([b])) for b in range(256)]
    crc = 0
    for b in data[offs[1]:offs[1] + lens[1]].tobytes():
        crc = (crc >> 8) ^ table[(crc ^ b) & 0xFF]
    assert got[1] == crc and got[2] == vc.crc16_arc(data[offs[2]:].tobytes())
    assert got == an.mp3_crc_ranges(0, offs, lens, data)


def test_launcher_refuses_ranges_and_frames_outside_the_buffer(an):
    import mp3rgain_amd as rg

    data = np.arange(100, dtype=np.uint8)
    for offs, lens in (([0, 90], [100, 11]), ([101], [0]), ([50], [2 ** 63])):
        with pytest.raises(rg.ReplayGainError) as e:
            an.mp3_crc_ranges(1, offs, lens, data)
        assert e.value.code == RG_ERR_INVALID_ARG
    with pytest.raises(rg.ReplayGainError) as e:
        an.mp3_frame_crc_check(1, [0, 95], data)
    assert e.value.code == RG_ERR_INVALID_ARG
    assert an.mp3_crc_ranges(1, [0, 100, 99], [100, 0, 1], data) == [vc.crc16_arc(data.tobytes()), 0, vc.crc16_arc(b"\x63")]
    assert an.mp3_crc_ranges(1, [], [], data) == []


def test_frame_crc_kernel_reports_exactly_the_damaged_frames(an):
    """About 2000 synthetic protected frames of every side-information size at arbitrary offsets, the last one touching the
    buffer's last byte; a known tenth has one bit flipped in header byte 2 or 3, the side information or the CRC word."""
    data, offs, ok = vc.protected_frames(2000, 41)
    assert ok.count(0) == 200 and {o % 4 for o in offs} == {0, 1, 2, 3}
    raw = data.tobytes()
    assert offs[-1] + 6 + vc.side_bytes(((raw[offs[-1] + 1] >> 3) & 3) != 3, (raw[offs[-1] + 3] >> 6) == 3) == data.size
    assert [int(vc.frame_crc_ok(raw[o:o + 40])) for o in offs] == ok
    got = an.mp3_frame_crc_check(1, offs, data)
    assert got == ok, [i for i, (g, w) in enumerate(zip(got, ok)) if g != w][:8]
    assert an.mp3_frame_crc_check(0, offs, data) == ok
    # side information that would reach beyond the buffer is a failure, not a read
    assert an.mp3_frame_crc_check(1, [offs[-1]], data[:offs[-1] + 8]) == [0]


# ---- rg_mp3_verify on files ---------------------------------------------------------------------------------------------------
def _write(tmp_path, name, data):
    p = tmp_path / name
    p.write_bytes(data)
    return p


@pytest.fixture()
def files(tmp_path):
    """(path, expected host-twin record or status) of the fixtures, the dense goldens, two damaged goldens, the written and the
    damaged cases, and a WAV, a FLAC and a missing path among them."""
    out = []
    for p in sorted(vc.FIXTURES.glob("*.mp3")) + vc.DENSE + sorted(CASES.glob("*.mp3")):
        out.append((p, p.read_bytes()))
    out.append((_write(tmp_path, "a.wav", wavutil.wav_bytes(wavutil.test_signal("s16", 44100, 3000, 2, seed=1), 44100, "s16")), RG_ERR_FORMAT))
    cases = vc.clean_cases()[::3] + vc.damaged_cases()
    for k, c in enumerate(cases):
        out.append((_write(tmp_path, f"{k:02d}-{c.name}.mp3", c.data), c.data))
        if k == 5:
            out.append((tmp_path / "missing.mp3", RG_ERR_IO))
        if k == 9:
            out.append((_write(tmp_path, "a.flac", flacenc.encode(np.zeros((2, 1200), dtype=np.int32), 44100, 16)), RG_ERR_FORMAT))
    return out, cases


def test_verify_files_equal_the_host_twin_and_the_definitions(an, files):
    listed, cases = files
    paths = [p for p, _ in listed]
    raw = an.verify_mp3_raw(paths)
    res = an.verify_mp3(paths)
    assert len(raw) == REC * len(paths)
    by_name = {}
    for i, ((p, what), r) in enumerate(zip(listed, res)):
        rec = raw[REC * i:REC * (i + 1)]
        if isinstance(what, int):
            assert r.error is not None and r.error.code == what and str(p) in str(r.error), p
            assert rec[4:] == bytes(REC - 4) and r.failed
            continue
        assert r.error is None, (p, r.error)
        assert rec == mv.verify_data_raw(what), p  # the host twin's record, byte for byte
        _, info = mp3dec.decode(what)
        assert r.dropped_frames == info.skipped_frames and r.audio_frames == info.audio_frames + info.skipped_frames, p
        by_name[p.name] = r
    assert by_name["test_stereo.mp3"].verdict == "length mismatch" and by_name["test_stereo.mp3"].music_crc_computed == 0x5B8F
    for name in ("test_joint_stereo.mp3", "test_vbr.mp3", "test_mono.mp3"):
        assert by_name[name].verified and by_name[name].flags == vc.ALL_GOOD
    for p in vc.DENSE:
        assert by_name[p.name].verdict == "no checksum" and by_name[p.name].flag("complete")
    for p in CASES.glob("*.mp3"):
        assert by_name[p.name].verdict == "1 frames dropped"
    for k, c in enumerate(cases):
        r = by_name[f"{k:02d}-{c.name}.mp3"]
        assert (hex(r.flags), r.verdict, r.dropped_frames, r.frame_crc_failed) == (hex(c.flags), c.verdict, c.dropped_frames, c.frame_crc_failed), c.name
        assert r.music_crc_computed == c.music_crc_computed, c.name
    assert an.verify_mp3([]) == []


def test_verify_is_the_same_across_routes_and_groups(an, files):
    """The rg_mp3_verify_result array, byte for byte, for every value of tuning key 6 (3: the loader pipeline and the kernels;
    2, 1: split decode and the kernels; 0: the host decoder and the host twin) and with key 13 forcing groups of two files.
    A decoder command is set and must not be run."""
    listed, _ = files
    paths = [p for p, _ in listed]
    want = an.verify_mp3_raw(paths)
    an.set_decoder_command("false {}")
    try:
        for key6 in (2, 1, 0, 3):
            an.set_tuning(6, key6)
            assert an.verify_mp3_raw(paths) == want, f"tuning key 6 = {key6}"
        an.set_tuning(13, 24 * 12000)  # 12 000 file bytes per group: the written cases go two by two, larger files alone
        for key6 in (3, 0):
            an.set_tuning(6, key6)
            assert an.verify_mp3_raw(paths) == want, f"groups of two, tuning key 6 = {key6}"
    finally:
        an.set_decoder_command(None)


def test_analysis_is_untouched_by_a_verify_call(an, files):
    """The loader keeps MPEG bytes only while rg_mp3_verify runs: an analysis after it gives what one before it gave."""
    p = vc.FIXTURES / "test_joint_stereo.mp3"
    before = an.analyze_track_file(p)
    assert an.verify_mp3([p])[0].verified
    after = an.analyze_track_file(p)
    assert (before.loudness_db, before.peak) == (after.loudness_db, after.peak)


# ---- the command line ---------------------------------------------------------------------------------------------------------
def test_cli_verify_on_a_mixed_list(an, tmp_path):
    from mp3rgain_amd import cli

    pcm = flacenc.test_pcm(np.random.default_rng(5), 2, 2000, 16)
    flac = _write(tmp_path, "plain.flac", flacenc.encode(pcm, 44100, 16))
    good = vc.FIXTURES / "test_mono.mp3"
    short = vc.FIXTURES / "test_stereo.mp3"
    bare = vc.DENSE[0]
    gained = _write(tmp_path, "gained.mp3", next(c.data for c in vc.damaged_cases() if c.name.startswith("gain-v1")))

    def run(*args):
        out, err = io.StringIO(), io.StringIO()
        rc = cli.main([str(a) for a in args], out, err)
        return rc, out.getvalue(), err.getvalue()

    rc, out, err = run("--verify", good, flac, short, bare, gained, tmp_path / "missing.mp3")
    assert rc == 1
    assert "test_mono.mp3 - verified" in out and "plain.flac - no signature" in out and "test_stereo.mp3 - length mismatch" in out
    assert f"{bare.name} - no checksum" in out and "gained.mp3 - gain applied, CRC not comparable" in out
    assert "missing.mp3 - Failed to open" in err
    rc, out, _ = run("--verify", good, flac, bare, gained)
    assert rc == 0
    # TSV has no header: an MP3 row says "mp3" in its third field, where a FLAC row (as without MP3 files) has its frame count
    rc, out, _ = run("--verify", "-o", "tsv", good, flac, short)
    assert rc == 1 and out.splitlines() == ["test_mono.mp3\tverified\tmp3\t40\t40\t0\t0\tff67\tff67",
                                            f"plain.flac\tno signature\t2000\t2000\t0\t{'00' * 16}\t{mc.md5(pcm, 16).hex()}",
                                            "test_stereo.mp3\tlength mismatch\tmp3\t39\t40\t0\t0\tbcfe\t5b8f"]
    rc, out, _ = run("--verify", "-o", "tsv", flac, good)
    assert rc == 0 and [line.split("\t")[2] for line in out.splitlines()] == ["2000", "mp3"]
    rc, out, _ = run("--verify", "-o", "json", good, flac, short)
    assert rc == 1
    d = json.loads(out)
    g, f, s = d["files"]
    fields = {"status", "flags", "audio_frames", "dropped_frames", "protected_frames", "frame_crc_failed", "junk_bytes", "xing_frames", "music_length",
              "audio_bytes", "music_crc_stored", "music_crc_computed", "tag_crc_stored", "tag_crc_computed", "encoder"} | set(mv.FLAG_NAMES)
    assert fields <= set(g) and fields <= set(s) and "md5_decoded" in f and "music_length" not in f
    assert (g["verdict"], g["verified"], g["music_crc_computed"], g["tag_crc_stored"], g["encoder"]) == ("verified", True, 0xFF67, 0x2BC4, "Lavc62.11")
    assert (s["verdict"], s["verified"], s["length_match"], s["music_crc_match"], s["music_crc_computed"]) == ("length mismatch", False, False, False, 0x5B8F)
    assert d["summary"] == {"total_files": 3, "successful": 2, "failed": 1}
