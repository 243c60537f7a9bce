"""rg_compare on files (include/mp3rgain_amd_compare.h): a few generated files of some seconds -- a WAV and a FLAC of the same
samples, one with 588 frames cut from its head; a copy behind 3 s + 17 frames of lead-in; a -3 dB re-dithered copy; another
recording; a file at another sample rate; a file that is not there -- through the fingerprint hint and through given hints.  The
oracle is the serial host twin (rg_compare_arena route 0, which tests/test_compare_cpu.py holds to the restatement) on the PCM
the files were written from with the lag the file route found as its hint, byte for byte.  Both FLAC decoder routes give the same
bytes, and a group size that splits the list is refused."""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import arena_layouts as al  # noqa: E402
import compare_cases as cc  # noqa: E402
import flacenc  # noqa: E402
from wavutil import wav_bytes  # noqa: E402

from mp3rgain_amd import _capi  # noqa: E402
from mp3rgain_amd import replaygain as rgmod  # noqa: E402

pytestmark = pytest.mark.gpu

RG_ERR_IO, RG_ERR_REFUSED = -8, -10
N, RATE, LEAD = 180000, 44100, 3 * 44100 + 17


@pytest.fixture()
def an(_ctx):
    _ctx.set_tuning(14, 1)
    _ctx.set_tuning(13, 0)
    _ctx.set_decoder_command(None)
    yield _ctx
    _ctx.set_tuning(14, 1)
    _ctx.set_tuning(13, 0)


def _music(rng, n):
    """Two channels of low-passed noise with a slow swell: something a fingerprint can hold on to."""
    out = []
    for _ in range(2):
        x = np.cumsum(rng.standard_normal(n + 64))
        x = x[64:] - np.convolve(x, np.ones(64) / 64.0, "valid")[:n]  # the drift taken out
        x *= 1.0 + 0.5 * np.sin(np.arange(n) / 9000.0)
        out.append(np.rint(x / np.abs(x).max() * 20000.0).astype(np.int16))
    return out


@pytest.fixture(scope="module")
def library(tmp_path_factory):
    """{name: (path, Tr of the planes the arena holds)}."""
    tmp = tmp_path_factory.mktemp("compare")
    rng = np.random.default_rng(91)
    x = _music(rng, N)
    lib = {}

    def wav(name, chans, rate=RATE):
        p = tmp / f"{name}.wav"
        p.write_bytes(wav_bytes(chans, rate, "s16"))
        lib[name] = (p, cc.Tr(name, [np.ascontiguousarray(c) for c in chans], rate))

    wav("ref", x)
    cut = [c[588:].copy() for c in x]
    p = tmp / "cut.flac"
    p.write_bytes(flacenc.encode(np.array([c.astype(np.int32) for c in cut]), RATE, 16, flacenc.Options(block_size=4096)))
    lib["cut"] = (p, cc.Tr("cut", cut, RATE))
    wav("lead", [np.concatenate([np.zeros(LEAD, np.int16), c]) for c in x])
    wav("gain", [np.rint(c * 10 ** (-3.0 / 20) + rng.triangular(-1, 0, 1, size=N)).astype(np.int16) for c in x])
    wav("other", _music(rng, N))
    wav("r48", x, 48000)
    lib["missing"] = (tmp / "missing.wav", None)
    return lib


def _twin(lib, names, pairs, lags, **opts):
    """Route 0 on the planes the files were written from, the file route's lags as hints and nothing to search."""
    trs = [lib[n][1] for n in names]
    arena, descs, _ = al.pack(trs, al.Layout("abut", "loud", "input"))
    return rgmod.compare_arena(None, 0, list(descs)[:len(trs)], [(a, b, h) for (a, b), h in zip(pairs, lags)], arena, radius=0, **opts)


def test_copies_through_the_fingerprint_hint(an, library):
    names = ["cut", "ref", "lead", "gain", "other", "r48"]
    files = [library[n][0] for n in names]
    pairs = [(0, 1), (1, 2), (1, 3), (1, 4), (1, 5), (3, 1), (2, 1), (1, 0)]
    got = an.compare(files, pairs)
    assert all(r.error is None for r in got)
    cut, lead, gain, other, r48, back, lead_ref, ref_cut = got
    # the FLAC whose head was cut against the WAV: identical, 588 frames on
    assert "identical" in cut.verdicts and (cut.lag, cut.a_head, cut.b_head, cut.a_tail, cut.b_tail, cut.overlap) == (588, 0, 588, 0, 0, N - 588)
    assert cut.reading == "identical samples, starts 588 samples later" and cut.hint % 512 == 0 and abs(cut.hint - 588) <= 512 and cut.format_a == cut.format_b == _capi.FMT_S16_PLANAR
    assert "identical" in lead.verdicts and (lead.lag, lead.b_head, lead.overlap) == (LEAD, LEAD, N) and lead.hint % 512 == 0 and abs(lead.hint - LEAD) <= 512
    assert gain.verdicts == ["same master"] and abs(gain.gain_db - 3.0) < 0.01 and 0.05 < gain.residual_lsb2 < 0.4 and gain.lag == 0
    assert back.verdicts == ["same master"] and abs(back.gain_db + 3.0) < 0.01 and back.reading.startswith("same master  (gain -3.00 dB, residual 0.")
    assert other.verdicts[0] == "unrelated" and other.lock < 0.1 and other.reading.startswith("not the same recording")
    assert r48.verdicts == ["different sample rate"] and r48.overlap == 0
    # the longer file as the reference copy: the match probes with b, and the sign of its lag turns round
    assert "identical" in lead_ref.verdicts and (lead_ref.lag, lead_ref.a_head, lead_ref.b_head, lead_ref.overlap) == (-LEAD, LEAD, 0, N)
    assert lead_ref.hint % 512 == 0 and abs(lead_ref.hint + LEAD) <= 512 and lead_ref.reading == f"identical samples, starts {LEAD} samples earlier"
    assert "identical" in ref_cut.verdicts and (ref_cut.lag, ref_cut.a_head, ref_cut.b_head, ref_cut.overlap) == (-588, 588, 0, N - 588)
    # the moments at the lag that was found are the serial twin's, byte for byte behind the pick
    twin = _twin(library, names, pairs[:4], [r.lag for r in got[:4]])
    for r, w in zip(got[:4], twin):
        for f in ("overlap", "a_head", "a_tail", "b_head", "b_tail", "blocks", "differing_blocks", "equal", "first_diff", "max_diff", "aa", "bb", "ab", "polarity",
                  "gain_db", "null_db", "null_unity_db", "residual_lsb2", "worst_block", "worst_block_db", "gain_min_db", "gain_max_db"):
            assert getattr(r, f) == getattr(w, f), (r.a, r.b, f)


def test_given_hints_both_decoder_routes_and_a_missing_file(an, library):
    names = ["cut", "ref", "missing", "lead", "gain"]
    files = [library[n][0] for n in names]
    pairs = [(0, 1), (1, 2), (1, 3), (2, 4), (1, 4)]
    hints = [580, 0, LEAD - 1000, 0, 3]
    raw = an.compare_raw(files, pairs, hints, blocks_per_pair=8, segment_frames=16384)
    REC = C.sizeof(_capi.CompareRecord)
    recs = [_capi.CompareRecord.from_buffer_copy(raw[0][REC * k:REC * k + REC]) for k in range(len(pairs))]
    assert [r.status for r in recs] == [0, RG_ERR_IO, 0, RG_ERR_IO, 0]
    assert bytes(recs[1])[4:] == bytes(REC - 4)  # a failing file's pairs: zero apart from the status
    assert [r.lag for r in (recs[0], recs[2], recs[4])] == [588, LEAD, 0] and [r.hint for r in (recs[0], recs[2], recs[4])] == [580, LEAD - 1000, 3]
    assert recs[0].flags & _capi.CMP_IDENTICAL and recs[2].flags & _capi.CMP_IDENTICAL and recs[4].flags & _capi.CMP_SAME_MASTER
    # the serial twin on the planes, the same hints and options: the same bytes (the indices are the call's)
    live = ["cut", "ref", "lead", "gain"]
    trs = [library[n][1] for n in live]
    arena, descs, _ = al.pack(trs, al.Layout("abut", "loud", "input"))
    twin, t_blocks, t_rows = rgmod.compare_arena(None, 0, list(descs)[:4], [(0, 1, 580), (1, 2, LEAD - 1000), (1, 3, 3)], arena, blocks_per_pair=8, lag_sums=True,
                                                     segment_frames=16384)
    for r, w, (a, b) in zip((recs[0], recs[2], recs[4]), twin, ((0, 1), (1, 3), (1, 4))):
        w.a, w.b = a, b
        assert bytes(r) == bytes(w), cc.differences(cc.got(r), cc.got(w))
    rows = np.frombuffer(raw[2], np.int64).reshape(len(pairs), -1)
    assert rows[[0, 2, 4]].tobytes() == t_rows.tobytes() and not rows[[1, 3]].any()
    BLK = C.sizeof(_capi.CompareBlock)
    for k, per in zip((0, 2, 4), t_blocks):
        assert raw[1][8 * BLK * k:8 * BLK * k + BLK * len(per)] == b"".join(bytes(b) for b in per)
    got = an.compare(files, pairs, hints, segment_frames=16384)
    assert got[1].error is not None and got[1].error.code == RG_ERR_IO and "missing.wav" in str(got[1].error) and got[0].error is None
    # the host FLAC decoder gives the same bytes
    an.set_tuning(14, 0)
    assert an.compare_raw(files, pairs, hints, blocks_per_pair=8, segment_frames=16384) == raw
    # a group size that splits the list: refused as a whole, with a text that says so
    an.set_tuning(13, 1 << 18)
    with pytest.raises(rgmod.ReplayGainError) as e:
        an.compare(files, pairs, hints)
    assert e.value.code == RG_ERR_REFUSED and "groups" in str(e.value) and "together" in str(e.value)


def test_the_projects_128_kbps_stream_differs(an, tmp_path):
    """An MPEG Layer III file against the WAV it was coded from: the float planes the device decoder leaves in the arena against
    16-bit planes, through the staged MPEG route; the serial twin on the host decoder's PCM gives the same bytes."""
    sys.path.insert(0, str(Path(__file__).resolve().parent.parent / "oracle"))
    import mp3_encoder as E

    from mp3rgain_amd import mp3dec

    n = 26000
    x = _music(np.random.default_rng(5), n)
    (tmp_path / "ref.wav").write_bytes(wav_bytes(x, RATE, "s16"))
    stream = E.encode(np.stack(x) / 32768.0, RATE, 128, seed=3)
    (tmp_path / "coded.mp3").write_bytes(stream)
    files = [tmp_path / "ref.wav", tmp_path / "coded.mp3"]
    raw = an.compare_raw(files, [(0, 1)], [1000], blocks_per_pair=2)
    r = _capi.CompareRecord.from_buffer_copy(raw[0])
    c = rgmod.compare_from_record(r)
    assert (r.status, r.dropped_a, r.dropped_b, r.format_a, r.format_b) == (0, 0, 0, _capi.FMT_S16_PLANAR, _capi.FMT_F32_PLANAR)
    assert c.verdicts[0] == "differs" and c.lag == 1057 and c.lock > 0.95 and -40.0 < c.null_db < -10.0 and abs(c.gain_db) < 0.5
    assert c.first_diff < 50 and c.reading.startswith("same recording, differs  (null -") and "first difference at 0:00.0" in c.reading
    dec, info = mp3dec.decode(stream)
    trs = [cc.Tr("ref", x, RATE), cc.Tr("coded", [np.ascontiguousarray(dec[0]), np.ascontiguousarray(dec[1])], RATE)]
    arena, descs, _ = al.pack(trs, al.Layout("abut", "loud", "input"))
    twin, t_blocks, t_rows = rgmod.compare_arena(None, 0, list(descs)[:2], [(0, 1, 1000)], arena, blocks_per_pair=2, lag_sums=True)
    assert raw[0] == bytes(twin[0]) and raw[2] == t_rows.tobytes() and raw[1][:48 * len(t_blocks[0])] == b"".join(bytes(b) for b in t_blocks[0])


def test_a_pair_that_cannot_be_measured_has_its_own_text(an, tmp_path):
    """Two healthy WAV files at 400 kHz: the block length would come from the sample rate and is beyond the limit, so the pair
    gets RG_ERR_FORMAT with a text of its own; the files' texts stay empty and another pair of the call is measured."""
    x = np.arange(-300, 300, dtype=np.int16)
    for name, rate in (("a.wav", 400000), ("b.wav", 400000), ("c.wav", 44100), ("d.wav", 44100)):
        (tmp_path / name).write_bytes(wav_bytes([x, x], rate, "s16"))
    files = [tmp_path / n for n in ("a.wav", "b.wav", "c.wav", "d.wav")]
    got = an.compare(files, [(0, 1), (2, 3)], hints=0, radius=4)
    assert got[0].error is not None and got[0].error.code == -9 and "a block of 400000 frames" in str(got[0].error) and "a.wav against" in str(got[0].error)
    assert got[1].error is None and got[1].verdicts == ["identical"]
    assert [an._lib.rg_tracks_error(an._ctx, i) for i in range(4)] == [b""] * 4 and an._lib.rg_compare_error(an._ctx, 1) == b""
    assert got[0].overlap == 0 and got[0].flags == 0
