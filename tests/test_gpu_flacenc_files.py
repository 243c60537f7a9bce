"""rg_flac_encode_files (include/mp3rgain_amd_flacenc.h): sub-second generated WAV files of every integer kind and FLAC files at
16 and 24 bits through the file call.  The oracle is the serial host twin (rg_flac_encode_arena route 0, which
tests/test_flacenc_cpu.py holds to its input) on the PCM the files were written from: the frames of every output are the
twin's, byte for byte, and the output decodes to that PCM.  Verify on and off, both FLAC decoder routes and a group size that
splits the list give the same files; a FLAC source's metadata comes through; each failure fails alone between good files and
leaves nothing behind."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import flacenc  # noqa: E402
import flacenc_cases as fc  # noqa: E402
import wavutil  # noqa: E402
from wavutil import wav_bytes  # noqa: E402

from mp3rgain_amd import _capi, flacdec  # noqa: E402
from mp3rgain_amd import replaygain as rgmod  # noqa: E402

pytestmark = pytest.mark.gpu

GOLD = Path(__file__).resolve().parent / "golden"
RG_ERR_STATE, RG_ERR_IO, RG_ERR_FORMAT = -6, -8, -9


@pytest.fixture()
def an(_ctx):
    _ctx.set_tuning(14, 1)
    _ctx.set_tuning(13, 0)
    _ctx.set_decoder_command(None)
    yield _ctx
    _ctx.set_tuning(14, 1)
    _ctx.set_tuning(13, 0)


def _write(tmp, name, data):
    p = tmp / name
    p.write_bytes(data)
    return p


def _blocks(stream):
    """[(type, body)] of a FLAC stream's metadata."""
    at, out = 4, []
    while True:
        last, t, n = stream[at] & 0x80, stream[at] & 0x7F, int.from_bytes(stream[at + 1:at + 4], "big")
        out.append((t, stream[at + 4:at + 4 + n]))
        at += 4 + n
        if last:
            return out


def _with_metadata(stream):
    """A FLAC stream with a SEEKTABLE, a VORBIS_COMMENT, an APPLICATION, a PICTURE and a PADDING block behind STREAMINFO."""
    blocks = _blocks(stream)
    vc = (4, (5).to_bytes(4, "little") + b"tests" + (1).to_bytes(4, "little") + (9).to_bytes(4, "little") + b"TITLE=one")
    extra = [(3, bytes(18)), (2, b"apps" + bytes(range(40))), vc, (6, bytes(range(200, 256)) * 3), (1, bytes(64)), (2, b"app2" + b"\x01\x02")]
    allb = [blocks[0]] + extra
    meta = b"fLaC" + b"".join(bytes([(0x80 if k == len(allb) - 1 else 0) | t]) + len(b).to_bytes(3, "big") + b for k, (t, b) in enumerate(allb))
    audio_at = 4 + sum(4 + len(b) for _, b in blocks)
    return meta + stream[audio_at:], [b for b in extra if b[0] not in (1, 3)]


@pytest.fixture(scope="module")
def library(tmp_path_factory):
    """[(path, Case of the PCM the file holds, blocks expected behind STREAMINFO or None)]"""
    tmp = tmp_path_factory.mktemp("flacenc")
    rng = np.random.default_rng(91)
    out = []
    for k, (kind, nch, bps) in enumerate((("u8", 2, 8), ("s16", 2, 16), ("s24", 6, 24), ("s16", 1, 16), ("s24", 2, 24))):
        n = 9000 + 1000 * k + 7
        chans = wavutil.test_signal(kind, 48000, n, nch, 190 + k)
        pcm = np.stack([np.asarray(c, dtype=np.int64) - (128 if kind == "u8" else 0) for c in chans])
        out.append((_write(tmp, f"{k}_{kind}_{nch}.wav", wav_bytes(chans, 48000, kind)), fc.Case(f"wav_{kind}_{nch}", pcm, bps, 48000), None))
    for name, bps in (("plain16", 16), ("plain24", 24)):
        pcm = flacenc.test_pcm(rng, 2, 3 * 1152 + 301, bps)
        stream, kept = _with_metadata(flacenc.encode(pcm, 44100, bps, flacenc.Options(block_size=1152, extra_metadata=False)))
        out.append((_write(tmp, f"{name}.flac", stream), fc.Case(f"flac_{name}", pcm, bps, 44100), kept))
    return out


def _twin_frames(cases, block=None, lpc=None):
    import arena_layouts as al
    arena, descs, _ = al.pack([fc.track_of(c) for c in cases], al.Layout("guard", "loud", "input", 2))
    streams, recs, _ = rgmod.flac_encode_arena(None, 0, list(descs)[:len(cases)], [c.bps for c in cases], arena, block, lpc)
    return [s[int(r.metadata_bytes):] for s, r in zip(streams, recs)]


def _encode(an, library, tmp, tag, **kw):
    outs = [tmp / f"{tag}_{k}.flac" for k in range(len(library))]
    recs = an.encode_flac([p for p, _, _ in library], outs, **kw)
    return outs, recs


def test_files_are_the_twins_frames_and_decode_to_their_source(an, library, tmp_path):
    want = _twin_frames([c for _, c, _ in library])
    outs, recs = _encode(an, library, tmp_path, "v")
    for (src, c, kept), dst, r, frames in zip(library, outs, recs, want):
        assert r.error is None and r.written and r.verified and r.complete and r.dropped_frames == 0, (c.name, r.error)
        data = dst.read_bytes()
        assert not dst.with_name(dst.name + ".part").exists()
        assert len(data) == r.stream_bytes and data[r.metadata_bytes:] == frames, c.name
        rate, bps, pcm, info = flacdec.decode(data)
        assert (rate, bps) == (c.rate, c.bps) and np.array_equal(pcm, c.pcm) and info.dropped_frames == 0, c.name
        assert flacdec.stream_md5(data) == flacdec.md5_planes(c.pcm, c.bps) == r.md5_pcm == r.md5_decoded, c.name
        got = _blocks(data)
        assert got[0][0] == 0 and [(t, bytes(b)) for t, b in got[1:]] == ([(t, bytes(b)) for t, b in kept] if kept is not None else [(4, got[1][1])]), c.name
        assert kept is not None or b"mp3rgain_amd" in got[1][1]
    # without the verify, with the host FLAC decoder and in groups of a file or two: the same files
    first = [p.read_bytes() for p in outs]
    outs2, recs2 = _encode(an, library, tmp_path, "n", verify=False)
    assert [p.read_bytes() for p in outs2] == first and not any(r.verified for r in recs2) and all(r.md5_decoded == bytes(16) for r in recs2)
    an.set_tuning(14, 0)
    an.set_tuning(13, 1 << 18)
    outs3, recs3 = _encode(an, library, tmp_path, "g")
    assert [p.read_bytes() for p in outs3] == first and all(r.verified for r in recs3)
    # other options reach the kernels
    want = _twin_frames([c for _, c, _ in library], 512, 12)
    outs4, recs4 = _encode(an, library, tmp_path, "o", block_size=512, max_lpc_order=12)
    assert [p.read_bytes()[r.metadata_bytes:] for p, r in zip(outs4, recs4)] == want and all(r.block_size == 512 for r in recs4)


def test_each_failure_fails_alone(an, library, tmp_path):
    good = [library[1], library[5]]
    f32 = _write(tmp_path, "float.wav", wav_bytes(wavutil.test_signal("f32", 44100, 3000, 2, 7), 44100, "f32"))
    s32 = _write(tmp_path, "s32.wav", wav_bytes(wavutil.test_signal("s32", 44100, 3000, 2, 8), 44100, "s32"))
    mp3 = GOLD / "mp3" / "v1_44k_ms_mixed.mp3"
    missing = tmp_path / "missing.wav"
    name, damaged, kept_pcm, dropped = next(v for v in flacenc.damaged_variants() if v[0] == "bitflip")
    dmg = _write(tmp_path, "damaged.flac", damaged)
    exists = tmp_path / "exists.flac"
    exists.write_bytes(b"mine")
    files = [good[0][0], mp3, f32, missing, good[1][0], good[0][0], good[1][0], dmg, s32]
    outs = [tmp_path / f"out_{k}.flac" for k in range(len(files))]
    outs[5] = exists
    outs[6] = good[1][0]  # the output is the input
    before = good[1][0].read_bytes()
    recs = an.encode_flac(files, outs)
    codes = [r.error.code if r.error is not None else 0 for r in recs]
    assert codes == [0, RG_ERR_FORMAT, RG_ERR_FORMAT, RG_ERR_IO, 0, RG_ERR_IO, RG_ERR_IO, 0, RG_ERR_FORMAT], [str(r.error) for r in recs]
    assert "MPEG" in str(recs[1].error) and "float" in str(recs[2].error) and "exists" in str(recs[5].error) and "is the input" in str(recs[6].error)
    assert exists.read_bytes() == b"mine" and good[1][0].read_bytes() == before
    for k in (1, 2, 3, 8):
        assert not outs[k].exists() and not recs[k].written
    assert sorted(p.name for p in tmp_path.glob("*.part")) == []
    for k, (src, c, _) in ((0, good[0]), (4, good[1])):
        assert np.array_equal(flacdec.decode(outs[k].read_bytes())[2], c.pcm)
    # the source with a dropped frame is encoded from what decoded
    r = recs[7]
    assert r.dropped_frames == dropped and not r.complete and r.verified and r.written
    assert np.array_equal(flacdec.decode(outs[7].read_bytes())[2], kept_pcm)
    # the same list again: every output of the first run now exists
    again = an.encode_flac(files, outs)
    assert all(r.error is not None for r in again)
