"""rg_dynamic_range on files (include/mp3rgain_amd_dr.h): generated WAV files of every kind the library reads, FLAC at 16 and 24
bits, an MP3 from the goldens, a missing path, a non-audio file and a 9-channel WAV among them.  The oracle is the serial host
twin (rg_dr_arena route 0, which tests/test_dr_cpu.py holds to the restatement) on the PCM the files were written from, byte for
byte, and the restatement itself (tests/dr_cases.py); for the MP3, the twin on the PCM the device decoder returns.  Both FLAC
decoder routes and a group size that splits the list give the same bytes."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import arena_layouts as al  # noqa: E402
import dr_cases as dc  # noqa: E402
import flacenc  # noqa: E402
import wavutil  # noqa: E402
from wavutil import planar_for_oracle, wav_bytes  # noqa: E402

from mp3rgain_amd import _capi  # noqa: E402
from mp3rgain_amd import replaygain as rgmod  # noqa: E402

pytestmark = pytest.mark.gpu

GOLD = Path(__file__).resolve().parent / "golden"
RG_ERR_IO, RG_ERR_FORMAT = -8, -9
REC = 64 + 8 * 64
OPTS = ((None, None), (1000, None), (777, 500))  # (block_frames, top_permille): the defaults make every file one short block


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


@pytest.fixture(scope="module")
def library(tmp_path_factory):
    """[(path, Tr of the planes the arena holds)]: WAV of every kind in mono, stereo and 5.1, and two FLAC files."""
    tmp = tmp_path_factory.mktemp("dr")
    rng = np.random.default_rng(71)
    out = []
    for k, (kind, nch) in enumerate((("u8", 1), ("s16", 2), ("s24", 6), ("s32", 2), ("f32", 1), ("f32", 6), ("s16", 6), ("u8", 2), ("s24", 1))):
        n = 9000 + 1000 * k + 7
        chans = wavutil.test_signal(kind, 48000, n, nch, 80 + k)
        if kind == "f32":
            chans[0][300] = np.float32(1.5)
            chans[0][301] = np.float32(np.nan)
        out.append((_write(tmp, f"{k}_{kind}_{nch}.wav", wav_bytes(chans, 48000, kind)), dc.Tr(f"wav_{kind}_{nch}", planar_for_oracle(chans, kind), 48000)))
    for name, bps in (("plain16", 16), ("plain24", 24)):
        n = 3 * 1152 + 301
        pcm = flacenc.test_pcm(rng, 2, n, bps)
        dt, w = (np.int16, 16) if bps <= 16 else (np.int32, 32)
        planes = [(pcm[ch].astype(np.int64) << (w - bps)).astype(dt) for ch in range(2)]
        out.append((_write(tmp, f"{name}.flac", flacenc.encode(pcm, 44100, bps, flacenc.Options(block_size=1152))), dc.Tr(f"flac_{name}", planes, 44100)))
    return out


def _records(raw, n):
    assert len(raw) == REC * n
    return [_capi.DrRecord.from_buffer_copy(raw[REC * k:REC * k + REC]) for k in range(n)]


def _twin(trs, opts):
    arena, descs, _ = al.pack(trs, al.Layout("abut", "loud", "input"))
    return rgmod.dr_arena(None, 0, list(descs)[:len(trs)], arena, *opts)


@pytest.mark.parametrize("opts", OPTS, ids=lambda o: f"{o[0]}-{o[1]}")
def test_files_match_the_host_twin_on_both_decoder_routes_and_in_groups(an, library, opts):
    files, trs = [p for p, _ in library], [tr for _, tr in library]
    raw = an.dynamic_range_raw(files, *opts)
    recs = _records(raw, len(files))
    for r, w, tr in zip(recs, _twin(trs, opts), trs):
        assert r.status == 0, (tr.name, r.status)
        assert bytes(r) == bytes(w), (tr.name, dc.differences(dc.got(r), dc.got(w)))
        assert not dc.differences(dc.got(r), dc.want_track(tr, *opts)), tr.name
    by_name = {tr.name: r for r, tr in zip(recs, trs)}
    assert by_name["wav_f32_1"].flags & _capi.DR_NONFINITE and by_name["wav_f32_1"].ch[0].nonfinite == 1
    assert bool(by_name["wav_s24_6"].flags & _capi.DR_SHORT) == (opts[0] is None) and by_name["wav_s24_6"].channels == 6
    an.set_tuning(14, 0)
    assert an.dynamic_range_raw(files, *opts) == raw
    an.set_tuning(13, 1 << 18)  # a file or two per group
    assert an.dynamic_range_raw(files, *opts) == raw
    an.set_tuning(14, 1)
    assert an.dynamic_range_raw(files, *opts) == raw


def test_the_python_records_and_the_options(an, library):
    files = [p for p, tr in library if tr.name in ("wav_s16_2", "flac_plain24")]
    res = an.dynamic_range(files, 1000)
    raw = _records(an.dynamic_range_raw(files, 1000), 2)
    for d, r in zip(res, raw):
        assert d.error is None and d.complete and not d.short and (d.dr, d.dr_mean, d.peak_db, d.rms_db, d.block_frames) == (r.dr, r.dr_mean, r.peak_db, r.rms_db, 1000)
        assert [c.top_ms for c in d.channels] == [r.ch[c].top_ms for c in range(2)] and d.channels[0].blocks == -(-d.frames // 1000)
    assert rgmod.album_dr(res) == round((res[0].dr + res[1].dr) / 2)
    for bad in ((None, 0), (None, 1001), (dc.MAX_BLOCK + 1, None)):
        with pytest.raises(rgmod.ReplayGainError) as e:
            an.dynamic_range(files, *bad)
        assert e.value.code == -1


def test_an_mp3_file_matches_the_host_twin_on_the_device_decoders_pcm(an):
    f = GOLD / "mp3" / "v1_44k_ms_mixed.mp3"
    pcm, info = an.decode_mp3_device(f.read_bytes())
    tr = rgmod.PcmTrack([np.ascontiguousarray(ch) for ch in pcm], int(info.sample_rate))
    arena, descs = rgmod.pack_tracks([tr])
    for opts in ((None, None), (4000, None)):
        want = rgmod.dr_arena(None, 0, list(descs)[:1], arena, *opts)[0]
        got = _capi.DrRecord.from_buffer_copy(an.dynamic_range_raw([f], *opts))
        assert bytes(got) == bytes(want), dc.differences(dc.got(got), dc.got(want))
        assert (got.format, got.channels, got.frames) == (_capi.FMT_F32_PLANAR, pcm.shape[0], pcm.shape[1]) and got.flags & _capi.DR_COMPLETE


def test_failing_files_fail_alone(an, tmp_path, library):
    rng = np.random.default_rng(72)
    nine = _write(tmp_path, "nine.wav", wav_bytes([rng.integers(-100, 100, 500) for _ in range(9)], 48000, "s16"))
    text = _write(tmp_path, "notes.txt", b"not audio at all\n" * 40)
    missing = tmp_path / "missing.flac"
    good = [library[1], library[9], library[4]]
    files = [good[0][0], missing, good[1][0], nine, good[2][0], text]
    an.set_decoder_command("false {}")  # a decoder command is set and must not be run
    try:
        res = an.dynamic_range(files, 1000)
        raw = an.dynamic_range_raw(files, 1000)
    finally:
        an.set_decoder_command(None)
    recs = _records(raw, len(files))
    for r, w in zip([recs[k] for k in (0, 2, 4)], _twin([tr for _, tr in good], (1000, None))):
        assert bytes(r) == bytes(w)
    for k, code, needle in ((1, RG_ERR_IO, "Failed to open"), (3, RG_ERR_FORMAT, "9 channels"), (5, None, "")):
        r = res[k]
        assert r.error is not None and (code is None or r.error.code == code) and needle in str(r.error) and str(files[k]) in str(r.error), (k, str(r.error))
        assert (r.frames, r.flags, r.channels, r.dr, r.dr_mean) == (0, 0, [], 0, 0.0)
        assert recs[k].status == r.error.code and raw[REC * k + 4:REC * k + REC] == bytes(REC - 4)  # zero apart from `status`
    assert an.dynamic_range([]) == []
