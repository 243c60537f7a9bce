"""FLAC verification on the GPU (include/mp3rgain_amd_flac.h): the MD5 kernel through its seam (rg_flac_md5_arena, route 1) on
PCM of the test's own choosing, rg_flac_verify on files, its equality across decoder routes and groups, and `--verify` of the
command line.  The oracle is hashlib.md5 over NumPy-packed bytes (tests/flac_md5_cases.py); no tolerance anywhere.
tests/test_flac_md5_cpu.py proves the same cases on the host twin."""
import hashlib
import io
import json
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import flac_md5_cases as mc  # noqa: E402
import flacenc  # noqa: E402
from wavutil import test_signal, wav_bytes  # noqa: E402

from mp3rgain_amd import _capi, flacdec  # noqa: E402

pytestmark = pytest.mark.gpu

GOLD = Path(__file__).resolve().parent / "golden" / "flac"
EXPECTED = json.loads((GOLD / "expected.json").read_text())
RG_ERR_IO, RG_ERR_FORMAT = -8, -9


@pytest.fixture()
def an(_ctx):
    _ctx.set_tuning(14, 1)
    _ctx.set_tuning(13, 0)
    _ctx.set_decoder_command(None)
    yield _ctx
    _ctx.set_tuning(14, 1)
    _ctx.set_tuning(13, 0)


# ---- the kernel, through the seam ---------------------------------------------------------------------------------------------
def test_kernel_matches_hashlib_on_a_ragged_arena(an):
    """One launch over the whole matrix and the long streams (three waves and more, the last one ragged), lengths 0 to 5000
    frames in shuffled order, offsets that are only sample-aligned, abutting streams, byte 0 and the last byte in use, guards
    in the gaps.  Rewriting the guards changes nothing, and the host twin gives the same bytes."""
    streams = mc.gpu_streams()
    a = mc.arena(streams)
    n = len(streams)
    assert n >= 130 and n % 64 != 0
    frames = [s.pcm.shape[1] for s in streams]
    assert min(frames) == 0 and max(frames) == 5000
    assert a.descs[0][0] == 0 and a.descs[-1][0] + len(mc.planes_bytes(streams[-1])) == a.bytes.size
    assert any(off % 4 == 2 and f % 2 == 1 and ch > 1 for off, f, ch, fmt in a.descs if fmt == mc.FMT_S16)
    descs = [_capi.TrackDesc(off, f, 44100, ch, fmt) for off, f, ch, fmt in a.descs]
    bps = [s.bps for s in streams]
    got = an.flac_md5_arena(1, descs, bps, a.bytes)
    bad = [s.name for s, g in zip(streams, got) if g != mc.md5(s.pcm, s.bps)]
    assert not bad, f"{len(bad)} of {n} digests differ from hashlib: {bad[:8]}"
    other = a.bytes.copy()
    other[a.guards] ^= 0xA5
    assert a.guards.sum() > n and an.flac_md5_arena(1, descs, bps, other) == got
    assert an.flac_md5_arena(0, descs, bps, a.bytes) == got


def test_kernel_refuses_a_stream_outside_the_arena(an):
    """The launcher checks every record against the arena: nothing is launched for a descriptor that reaches beyond it."""
    import mp3rgain_amd as rg

    arena = np.zeros(64, dtype=np.uint8)
    with pytest.raises(rg.ReplayGainError):
        an.flac_md5_arena(1, [_capi.TrackDesc(0, 9, 44100, 2, mc.FMT_S32)], [24], arena)
    with pytest.raises(rg.ReplayGainError):
        an.flac_md5_arena(1, [_capi.TrackDesc(2, 1, 44100, 1, mc.FMT_S32)], [24], arena)
    assert an.flac_md5_arena(1, [_capi.TrackDesc(0, 8, 44100, 2, mc.FMT_S32)], [24], arena) == [hashlib.md5(bytes(48)).digest()]


# ---- rg_flac_verify on files --------------------------------------------------------------------------------------------------
def _signed(stream: bytes, sig: bytes, total=None) -> bytes:
    """`stream` (no ID3v2 tag) with `sig` in STREAMINFO's MD5 field, and STREAMINFO's total_samples replaced if given."""
    at = stream.index(b"fLaC")
    b = bytearray(stream)
    b[at + 26:at + 42] = sig
    if total is not None:
        b[at + 21] = (b[at + 21] & 0xF0) | ((total >> 32) & 0x0F)
        b[at + 22:at + 26] = (total & 0xFFFFFFFF).to_bytes(4, "big")
    return bytes(b)


@pytest.fixture(scope="module")
def intact():
    rng = np.random.default_rng(21)
    pcm = flacenc.test_pcm(rng, 2, 3 * 1152 + 77, 16)
    return pcm, flacenc.encode(pcm, 44100, 16, flacenc.Options(block_size=1152, stereo="mid_side")), mc.md5(pcm, 16)


def _write(tmp_path, name, data):
    p = tmp_path / name
    p.write_bytes(data)
    return p


def test_verify_signatures_and_length(an, tmp_path, intact):
    pcm, stream, sig = intact
    wrong = bytes([sig[0] ^ 1]) + sig[1:]
    gold = "s24_stereo_96k_ms_rice2"
    files = [_write(tmp_path, "good.flac", _signed(stream, sig)),
             _write(tmp_path, "wrong.flac", _signed(stream, wrong)),
             GOLD / f"{gold}.flac",
             _write(tmp_path, "long.flac", _signed(stream, sig, total=pcm.shape[1] + 1)),
             _write(tmp_path, "tagged.flac", flacenc.id3v2_tag(300) + _signed(stream, sig))]
    good, bad, unsigned, longer, tagged = an.verify_flac(files)
    for r in (good, tagged):
        assert r.error is None and r.verified, r
        assert (r.has_signature, r.md5_match, r.length_match, r.complete) == (True, True, True, True)
        assert (r.frames, r.total_samples, r.audio_frames, r.dropped_frames) == (pcm.shape[1], pcm.shape[1], 4, 0)
        assert r.md5_stream == sig == r.md5_decoded
    assert bad.error is None and not bad.verified
    assert (bad.has_signature, bad.md5_match, bad.length_match, bad.complete) == (True, False, True, True)
    assert bad.md5_stream == wrong and bad.md5_decoded == sig
    # a committed file without a signature: the digest is that of the PCM whose sha256 expected.json records
    e = EXPECTED[gold]
    _, bps, want, _ = flacdec.decode((GOLD / f"{gold}.flac").read_bytes())
    assert hashlib.sha256(np.ascontiguousarray(want.astype("<i4")).tobytes()).hexdigest() == e["sha256"]
    assert unsigned.error is None and not unsigned.verified
    assert (unsigned.has_signature, unsigned.md5_match, unsigned.length_match, unsigned.complete) == (False, False, True, True)
    assert unsigned.md5_stream == bytes(16) and unsigned.md5_decoded == mc.md5(want, bps)
    assert (unsigned.frames, unsigned.dropped_frames) == (e["samples"], 0)
    assert longer.error is None and not longer.verified
    assert (longer.has_signature, longer.md5_match, longer.length_match, longer.complete) == (True, True, False, True)
    assert (longer.frames, longer.total_samples) == (pcm.shape[1], pcm.shape[1] + 1)


def test_verify_damaged_streams(an, tmp_path):
    """Every damaged variant carries the signature of the intact input.  A stream that loses a frame shows COMPLETE and
    MD5_MATCH off, dropped_frames as the host decoder reports it, and the digest of what survived; the others verify."""
    variants = flacenc.damaged_variants()
    whole = {}  # the intact input of a variant: the stereo stream's (the first six variants), or its own
    files, want = [], []
    for name, data, kept, dropped in variants:
        _, _, host, hi = flacdec.decode(data)
        assert int(hi.dropped_frames) == dropped and np.array_equal(host, kept), name
        full = kept if dropped == 0 else None
        if full is not None and kept.shape[0] == 2:
            whole[2] = kept
        files.append((name, data, kept, dropped, full))
    lost = 0
    paths = []
    for name, data, kept, dropped, full in files:
        source = full if full is not None else whole[2]
        at = data.index(b"fLaC")
        paths.append(_write(tmp_path, f"{name}.flac", data[:at] + _signed(data[at:], mc.md5(source, 16))))
        want.append((name, kept, dropped, mc.md5(source, 16)))
    res = an.verify_flac(paths)
    for (name, kept, dropped, sig), r in zip(want, res):
        assert r.error is None and r.has_signature and r.md5_stream == sig, name
        assert r.dropped_frames == dropped and r.frames == kept.shape[1], name
        assert r.md5_decoded == mc.md5(kept, 16), name
        assert r.complete == (dropped == 0) and r.md5_match == (dropped == 0) and r.verified == (dropped == 0), name
        lost += dropped > 0
    assert lost == 4 and len(res) == len(variants) == 8


def test_verify_failing_files_fail_alone(an, tmp_path, intact):
    pcm, stream, sig = intact
    good = _write(tmp_path, "good.flac", _signed(stream, sig))
    wav = _write(tmp_path, "a.wav", wav_bytes(test_signal("s16", 44100, 5000, 2, seed=1), 44100, "s16"))
    missing = tmp_path / "missing.flac"
    rng = np.random.default_rng(22)
    wide = _write(tmp_path, "wide.flac", flacenc.encode(flacenc.test_pcm(rng, 2, 2000, 32), 44100, 32, flacenc.Options(subframe="verbatim", wasted=False)))
    an.set_decoder_command("false {}")  # a decoder command is set and must not be run
    try:
        res = an.verify_flac([good, wav, good, missing, wide, good])
    finally:
        an.set_decoder_command(None)
    for r in (res[0], res[2], res[5]):
        assert r.error is None and r.verified and r.md5_decoded == sig
    for r, code, text in ((res[1], RG_ERR_FORMAT, "Not a native FLAC stream"), (res[3], RG_ERR_IO, "Failed to open"),
                          (res[4], RG_ERR_FORMAT, "FLAC of 32 bits per sample")):
        assert r.error is not None and r.error.code == code and text in str(r.error), r
        assert not r.verified and not (r.has_signature or r.md5_match or r.length_match or r.complete)
        assert (r.frames, r.total_samples, r.audio_frames, r.dropped_frames) == (0, 0, 0, 0)
        assert r.md5_stream == bytes(16) == r.md5_decoded
    assert str(wav) in str(res[1].error) and str(missing) in str(res[3].error) and str(wide) in str(res[4].error)
    assert an.verify_flac([]) == []


def test_verify_is_the_same_across_routes_and_groups(an, tmp_path, intact):
    """The rg_flac_verify_result array, byte for byte: device decoder and kernel, host decoder and host twin, and the list
    taken in several groups."""
    pcm, stream, sig = intact
    rng = np.random.default_rng(23)
    files = [_write(tmp_path, "good.flac", _signed(stream, sig)), GOLD / "s16_6ch_48k.flac", GOLD / "damaged_bitflip.flac",
             tmp_path / "missing.flac", GOLD / "s12_stereo_16k_ls.flac", GOLD / "s20_stereo_88k_rs.flac", GOLD / "damaged_truncated_last.flac"]
    for k, (bps, ch, n) in enumerate(((8, 1, 0), (24, 3, 1001), (16, 2, 4097))):
        p = flacenc.test_pcm(rng, ch, n, bps)
        files.append(_write(tmp_path, f"extra{k}.flac", _signed(flacenc.encode(p, 48000, bps, flacenc.Options(block_size=576)), mc.md5(p, bps))))
    device = an.verify_flac_raw(files)
    assert len(device) == 64 * len(files)
    res = an.verify_flac(files)
    assert [r.verified for r in res] == [True, False, False, False, False, False, False, True, True, True]
    assert res[2].dropped_frames == 1 and res[6].dropped_frames == 1 and res[3].error.code == RG_ERR_IO
    an.set_tuning(14, 0)
    host = an.verify_flac_raw(files)
    an.set_tuning(14, 1)
    assert host == device
    an.set_tuning(13, 24 * 30000)  # a few files per group
    assert an.verify_flac_raw(files) == device
    an.set_tuning(14, 0)
    assert an.verify_flac_raw(files) == device


# ---- the command line ---------------------------------------------------------------------------------------------------------
def test_cli_verify(an, tmp_path, intact):
    from mp3rgain_amd import cli

    pcm, stream, sig = intact
    good = _write(tmp_path, "good.flac", _signed(stream, sig))
    wrong = _write(tmp_path, "wrong.flac", _signed(stream, bytes(15) + b"\x01"))
    unsigned = _write(tmp_path, "unsigned.flac", stream)

    def run(*args):
        out, err = io.StringIO(), io.StringIO()
        rc = cli.main([str(a) for a in args], out, err)
        return rc, out.getvalue(), err.getvalue()

    rc, out, _ = run("--verify", "-o", "json", good, wrong, unsigned)
    assert rc == 1
    d = json.loads(out)
    g, w, u = d["files"]
    for f in (g, w, u):
        assert {"file", "status", "verified", "has_signature", "md5_match", "length_match", "complete", "frames", "total_samples",
                "dropped_frames", "md5_stream", "md5_decoded"} <= set(f)
        assert f["status"] == "success" and f["frames"] == f["total_samples"] == pcm.shape[1] and f["dropped_frames"] == 0
        assert f["md5_decoded"] == sig.hex() and f["length_match"] is True and f["complete"] is True
    assert (g["verified"], g["has_signature"], g["md5_match"], g["md5_stream"]) == (True, True, True, sig.hex())
    assert (w["verified"], w["has_signature"], w["md5_match"], w["md5_stream"]) == (False, True, False, "00" * 15 + "01")
    assert (u["verified"], u["has_signature"], u["md5_match"], u["md5_stream"]) == (False, False, False, "00" * 16)
    assert d["summary"] == {"total_files": 3, "successful": 2, "failed": 1}
    rc, out, _ = run("--verify", "-o", "json", good, unsigned)
    assert rc == 0 and [f["verified"] for f in json.loads(out)["files"]] == [True, False]
    rc, out, err = run("--verify", good, wrong, unsigned, tmp_path / "missing.flac")
    assert rc == 1
    assert "good.flac - verified" in out and "wrong.flac - MD5 mismatch" in out and "unsigned.flac - no signature" in out
    assert "missing.flac - Failed to open" in err
    rc, out, _ = run("--verify", "-o", "tsv", good, wrong)
    assert rc == 1 and out.splitlines() == [f"good.flac\tverified\t{pcm.shape[1]}\t{pcm.shape[1]}\t0\t{sig.hex()}\t{sig.hex()}",
                                            f"wrong.flac\tMD5 mismatch\t{pcm.shape[1]}\t{pcm.shape[1]}\t0\t{'00' * 15}01\t{sig.hex()}"]
