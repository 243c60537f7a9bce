"""rg_spectrum on files (include/mp3rgain_amd_spectrum.h): WAV (16-bit, 24-bit, float) and FLAC (16- and 24-bit) files of the
verdict signals of tests/spectrum_cases.py, an MP3 from the goldens, a missing path and a junk file among them.  The oracle is
the seam (rg_spectrum_arena, route 2) on the PCM the files were written from, which the other tests hold to the restatement.
Both FLAC decoder routes and a group size that splits the list give the same bytes."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import arena_layouts as al  # noqa: E402
import flacenc  # noqa: E402
import spectrum_cases as sc  # noqa: E402
from wavutil import wav_bytes  # noqa: E402

from mp3rgain_amd import _capi  # noqa: E402
from mp3rgain_amd import replaygain as rgmod  # noqa: E402

pytestmark = pytest.mark.gpu

GOLD = Path(__file__).resolve().parent / "golden"
RG_ERR_IO, RG_ERR_FORMAT = -8, -9
REC = 40 + 8 * 32
BL, UP, COMPLETE = _capi.SPEC_BANDLIMITED, _capi.SPEC_UPSAMPLED, _capi.SPEC_COMPLETE


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
    """[(path, Tr of the planes the arena holds)]: the verdict signals as stereo files, the second channel at half the level."""
    tmp = tmp_path_factory.mktemp("spectrum")
    out = []
    for name, kind in (("white", "wav-s16"), ("white-16k", "wav-s16"), ("white-16k", "flac-16"), ("pink-up96k", "wav-s24"), ("pink-up96k", "flac-24"),
                       ("pink-96k", "flac-24"), ("white-16k-f32", "wav-f32"), ("pink", "flac-16")):
        x, row = sc.verdict_signal(name)
        rate = row[1]
        chans = [x, 0.5 * x]
        if kind == "wav-f32":
            planes = [c.astype(np.float32) for c in chans]
            data = wav_bytes(planes, rate, "f32")
        elif kind.endswith("16"):
            planes = [sc.as_s16(c) for c in chans]
            data = wav_bytes(planes, rate, "s16") if kind.startswith("wav") else flacenc.encode(np.stack(planes).astype(np.int64), rate, 16)
        else:
            planes = [sc.as_s24(c) for c in chans]
            ints = [p >> 8 for p in planes]
            data = wav_bytes(ints, rate, "s24") if kind.startswith("wav") else flacenc.encode(np.stack(ints).astype(np.int64), rate, 24)
        ext = "wav" if kind.startswith("wav") else "flac"
        out.append((_write(tmp, f"{len(out)}_{name}_{kind}.{ext}", data), sc.Tr(f"{name}/{kind}", tuple(planes), rate)))
    return out


def _records(raw, n):
    return [_capi.SpectrumRecord.from_buffer_copy(raw[REC * k:REC * k + REC]) for k in range(n)]


def _seam(library):
    tracks = [tr for _, tr in library]
    arena, descs, _ = al.pack(tracks, al.Layout("guard", "loud", "input", 1))
    recs, e = rgmod.spectrum_arena(None, 2, list(descs)[:len(tracks)], arena)
    return b"".join(bytes(r) for r in recs), e.tobytes()


def test_files_match_the_seam_on_both_decoder_routes_and_in_groups(an, library):
    files = [p for p, _ in library]
    raw, bands = an.spectrum_raw(files)
    assert len(raw) == REC * len(files) and len(bands) == len(files) * 8 * 256 * 8
    want_raw, want_bands = _seam(library)
    assert raw == want_raw and bands == want_bands
    by_name = {tr.name: r for r, (_, tr) in zip(_records(raw, len(files)), library)}
    for name in ("white-16k/wav-s16", "white-16k/flac-16"):
        r = by_name[name]
        assert r.flags == BL | COMPLETE and abs(r.cutoff_hz - 16200.0) <= 172.3 and all(abs(c.cutoff_hz - 16200.0) <= 172.3 for c in r.ch[:2]), name
    for name in ("white/wav-s16", "pink/flac-16", "pink-96k/flac-24"):
        r = by_name[name]
        assert r.flags == COMPLETE and (r.cutoff_hz, r.ch[0].edge_db) == (r.sample_rate / 2.0, 0.0), name
    for name in ("pink-up96k/wav-s24", "pink-up96k/flac-24"):
        r = by_name[name]
        assert r.flags == BL | UP | COMPLETE and 21900.0 <= r.cutoff_hz <= 22800.0, name
    assert by_name["white-16k-f32/wav-f32"].flags == BL | COMPLETE
    an.set_tuning(14, 0)
    assert an.spectrum_raw(files) == (raw, bands)
    an.set_tuning(13, 1 << 20)  # a file or two per group
    assert an.spectrum_raw(files) == (raw, bands)
    an.set_tuning(14, 1)
    assert an.spectrum_raw(files) == (raw, bands)
    # the Python results say the same
    res = an.spectrum(files, bands=True)
    r = res[[tr.name for _, tr in library].index("pink-up96k/flac-24")]
    assert r.error is None and r.upsampled and r.bandlimited and r.complete and r.verdicts == ["bandlimited", "upsampled"]
    assert r.words == f"96 kHz file with nothing above {r.cutoff_hz / 1000:.1f} kHz"
    lv = r.channels[0].levels_db
    assert len(lv) == 256 and max(lv) == 0.0 and lv[255] < -60.0
    assert an.spectrum(files)[0].channels[0].bands is None and an.spectrum(files)[0].words == "no cutoff below Nyquist"


def test_options_reach_the_verdict(an, library):
    files = [p for p, tr in library if tr.name == "white-16k/wav-s16"]
    assert an.spectrum(files, edge_db=200.0)[0].verdicts == ["ok"]
    assert an.spectrum(files, min_cutoff_hz=20000.0)[0].verdicts == ["ok"]
    assert an.spectrum(files, edge_db=20.0, min_cutoff_hz=1000.0)[0].bandlimited
    with pytest.raises(rgmod.ReplayGainError) as e:
        an.spectrum(files, edge_db=0.0)
    assert e.value.code == -1


def test_an_mp3_file_matches_the_seam_on_the_device_decoders_pcm(an):
    f = GOLD / "mp3" / "v1_44k_ms_mixed.mp3"
    pcm, info = an.decode_mp3_device(f.read_bytes())
    tr = rgmod.PcmTrack([np.ascontiguousarray(ch) for ch in pcm], int(info.sample_rate))
    arena, descs = rgmod.pack_tracks([tr])
    want, want_e = rgmod.spectrum_arena(None, 2, list(descs)[:1], arena)
    raw, bands = an.spectrum_raw([f])
    got = _capi.SpectrumRecord.from_buffer_copy(raw)
    assert raw == bytes(want[0]) and bands == want_e.tobytes()
    assert (got.format, got.channels, got.frames) == (_capi.FMT_F32_PLANAR, pcm.shape[0], pcm.shape[1]) and got.flags & COMPLETE
    assert got.ch[0].analysed_frames == sc.frames_of(pcm.shape[1]) > 0


def test_failing_files_fail_alone(an, tmp_path, library):
    missing = tmp_path / "missing.flac"
    junk = _write(tmp_path, "junk.flac", bytes(range(256)) * 40)
    rng = np.random.default_rng(52)
    nine = _write(tmp_path, "nine.wav", wav_bytes([rng.integers(-100, 100, 500) for _ in range(9)], 48000, "s16"))
    good = [library[1], library[4]]
    files = [good[0][0], missing, good[1][0], nine, junk]
    an.set_decoder_command("false {}")  # a decoder command is set and must not be run
    try:
        res = an.spectrum(files, bands=True)
        raw, bands = an.spectrum_raw(files)
    finally:
        an.set_decoder_command(None)
    want_raw, want_bands = _seam(good)
    assert raw[:REC] + raw[2 * REC:3 * REC] == want_raw
    nb = 8 * 256 * 8
    assert bands[:nb] + bands[2 * nb:3 * nb] == want_bands
    for k, code, text in ((1, RG_ERR_IO, "Failed to open"), (3, RG_ERR_FORMAT, "9 channels"), (4, RG_ERR_FORMAT, "")):
        r = res[k]
        assert r.error is not None and r.error.code == code and text in str(r.error) and str(files[k]) in str(r.error), (k, str(r.error))
        assert (r.frames, r.flags, r.channels, r.cutoff_hz) == (0, 0, [], 0.0)
        assert _records(raw, 5)[k].status == code and raw[REC * k + 4:REC * k + REC] == bytes(REC - 4)  # zero apart from `status`
        assert bands[nb * k:nb * k + nb] == bytes(nb)
    assert an.spectrum([]) == []
