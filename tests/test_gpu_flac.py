"""FLAC on the device (mp3rgain_amd/csrc/rg_flacdev.hip) and through the file route: the device PCM equals the host
decoder's bit for bit, and every result for a FLAC file equals the result for a RIFF/WAVE file of the same PCM (and the
CPU oracle on it): track, album, peak, the error of a broken file, both routes of tuning key 14, the node route."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import flacenc as fe  # noqa: E402
from test_flacdec import MATRIX, _pcm, damaged_variants  # noqa: E402
from wavutil import wav_bytes  # noqa: E402

pytestmark = pytest.mark.gpu
O = fe.Options


@pytest.fixture()
def an(_ctx):
    _ctx.set_kernel(0)
    _ctx.set_tuning(1, 0)
    _ctx.set_tuning(2, 0)
    _ctx.set_tuning(14, 1)
    _ctx.set_tuning(10, 0)
    _ctx.set_decoder_command(None)
    yield _ctx
    _ctx.set_tuning(14, 1)
    _ctx.set_tuning(10, 0)


def _wav_of(pcm, rate, bps):
    """The RIFF/WAVE twin: <= 16 bits as s16 (<< 16 - bps), 17-24 bits as s24 (<< 24 - bps)."""
    if bps <= 16:
        return wav_bytes([c << (16 - bps) for c in pcm], rate, "s16", extensible=len(pcm) > 2)
    return wav_bytes([c << (24 - bps) for c in pcm], rate, "s24", extensible=len(pcm) > 2)


def _planar(pcm, bps):
    if bps <= 16:
        return [(c << (16 - bps)).astype(np.int16) for c in pcm]
    return [(c.astype(np.int64) << (32 - bps)).astype(np.int32) for c in pcm]


@pytest.mark.parametrize("name,opt,ch,bps,rate,n", MATRIX, ids=[m[0] for m in MATRIX])
def test_device_pcm_matrix(an, name, opt, ch, bps, rate, n):
    from mp3rgain_amd import flacdec

    data = fe.encode(_pcm(name, ch, bps, n), rate, bps, opt)
    host = flacdec.decode(data)[2]
    dev, info = an.decode_flac_device(data)
    assert np.array_equal(dev, host) and info.dropped_frames == 0


def test_device_pcm_damaged_and_fuzzed(an):
    from mp3rgain_amd import flacdec

    for name, data, want, dropped in damaged_variants():
        dev, info = an.decode_flac_device(data)
        assert np.array_equal(dev, want) and info.dropped_frames == dropped, name
    rng = np.random.default_rng(0xBEEF)
    base = fe.encode(fe.test_pcm(rng, 2, 30000, 16), 44100, 16, O(block_size=1152, stereo="alternate", subframe="auto"))
    for k in range(300):
        b = bytearray(base)
        for _ in range(int(rng.integers(1, 4))):
            at = int(rng.integers(0, len(b)))
            if k % 2:
                b[at] ^= 1 << int(rng.integers(8))
            else:
                del b[at:at + int(rng.integers(1, 40))]
        b = bytes(b)
        try:
            _, _, host, hi = flacdec.decode(b)
        except flacdec.FlacError:
            continue
        dev, di = an.decode_flac_device(b)
        assert np.array_equal(dev, host) and di.dropped_frames == hi.dropped_frames, k


RATES = [96000, 88200, 64000, 48000, 44100, 32000, 24000, 22050, 16000, 12000, 11025, 8000]


@pytest.mark.parametrize("route", [1, 0])
@pytest.mark.parametrize("rate,ch,bps", [(r, 2, 16) for r in RATES] + [(44100, 1, 8), (48000, 2, 12), (44100, 2, 20), (96000, 2, 24), (48000, 6, 16)])
def test_track_equals_wav(an, oracle, tmp_path, route, rate, ch, bps):
    import mp3rgain_amd as rg

    an.set_tuning(14, route)
    pcm = fe.test_pcm(np.random.default_rng(rate + ch + bps), ch, rate * 2 + 333, bps)
    f = tmp_path / "t.flac"
    w = tmp_path / "t.wav"
    f.write_bytes(fe.encode(pcm, rate, bps, O(stereo="alternate")))
    w.write_bytes(_wav_of(pcm, rate, bps))
    a, b = an.analyze_track_file(f), an.analyze_track_file(w)
    assert (a.loudness_db, a.gain_db, a.peak, a.windows, a.sample_rate, a.flags) == (b.loudness_db, b.gain_db, b.peak, b.windows, b.sample_rate, b.flags)
    assert a.file_type == rg.AudioFileType.Mp3
    pl = _planar(pcm, bps)
    want, _ = oracle.analyze_pcm(pl[0], pl[1] if ch > 1 else None, rate)
    if ch <= 2:
        assert a.loudness_db == want["loudness_db"] and a.peak == want["peak"]
    pk, pw = an.find_peak_amplitude_file(f), an.find_peak_amplitude_file(w)
    assert (pk.peak, pk.peak_pcm, pk.sample_rate) == (pw.peak, pw.peak_pcm, pw.sample_rate)
    assert pk.peak == oracle.find_peak(pl, pl[0].dtype)  # every channel, the 6-channel file included


def test_unsupported_rate_and_broken_file(an, tmp_path):
    import mp3rgain_amd as rg

    good = tmp_path / "good.flac"
    good.write_bytes(fe.encode(fe.test_pcm(np.random.default_rng(1), 2, 50000, 16), 44100, 16))
    hi = tmp_path / "hi.flac"
    hi.write_bytes(fe.encode(fe.test_pcm(np.random.default_rng(2), 2, 20000, 16), 192000, 16))
    broken = tmp_path / "broken.flac"
    broken.write_bytes(b"fLaC" + bytes(40))
    res = an.analyze_track_files([good, broken, hi, good])
    assert isinstance(res[1], rg.ReplayGainError) and "Failed to probe format" in str(res[1])
    assert isinstance(res[2], rg.ReplayGainError) and "Unsupported sample rate: 192000" in str(res[2])
    assert res[0].loudness_db == res[3].loudness_db == an.analyze_track_file(good).loudness_db
    deep = tmp_path / "deep.flac"
    deep.write_bytes(fe.encode(fe.test_pcm(np.random.default_rng(3), 1, 3000, 28), 44100, 28, O(subframe="verbatim")))
    with pytest.raises(rg.ReplayGainError, match="Failed to create decoder"):
        an.analyze_track_file(deep)


@pytest.mark.parametrize("parts", [1, 2])
def test_mixed_album_equals_fold(an, oracle, tmp_path, parts):
    from mp3rgain_amd import mp3dec

    an.set_tuning(10, parts)
    files, hists, peaks = [], [], []
    rng = np.random.default_rng(parts)
    for i, (rate, bps) in enumerate([(44100, 16), (44100, 24), (44100, 16)]):
        pcm = fe.test_pcm(rng, 2, 44100 * 3 + 17 * i, bps)
        f = tmp_path / f"a{i}.flac"
        f.write_bytes(fe.encode(pcm, rate, bps, O(stereo="mid_side")))
        files.append(f)
        pl = _planar(pcm, bps)
        _, h = oracle.analyze_pcm(pl[0], pl[1], rate)
        hists.append(h)
        peaks.append(oracle.analyze_pcm(pl[0], pl[1], rate)[0]["peak"])
    mp3 = Path(__file__).parent / "golden" / "mp3" / "v1_44k_ms_mixed.mp3"
    files.append(mp3)
    pcm3, info3 = mp3dec.decode(mp3.read_bytes())
    want3, h3 = oracle.analyze_pcm(pcm3[0], pcm3[1] if info3.channels == 2 else None, info3.sample_rate)
    hists.append(h3)
    peaks.append(want3["peak"])
    wav = tmp_path / "w.wav"
    wpcm = fe.test_pcm(rng, 2, 44100 * 2, 16)
    wav.write_bytes(_wav_of(wpcm, 44100, 16))
    files.append(wav)
    _, hw = oracle.analyze_pcm(wpcm[0].astype(np.int16), wpcm[1].astype(np.int16), 44100)
    hists.append(hw)
    peaks.append(oracle.analyze_pcm(wpcm[0].astype(np.int16), wpcm[1].astype(np.int16), 44100)[0]["peak"])
    album = an.analyze_album_files(files)
    ref, _ = oracle.album_from_hists(hists, peaks)
    assert album.album_loudness_db == ref["album_loudness_db"] and album.album_gain_db == ref["album_gain_db"]
    assert album.album_peak == max(peaks)
    assert [t.peak for t in album.tracks] == peaks


def test_node_route(an, tmp_path):
    import mp3rgain_amd as rg

    files = []
    for i in range(3):
        f = tmp_path / f"n{i}.flac"
        f.write_bytes(fe.encode(fe.test_pcm(np.random.default_rng(10 + i), 2, 44100 * 2, 16), 44100, 16))
        files.append(f)
    want = an.analyze_album_files(files)
    with rg.Node([0]) as node:
        got = node.analyze_album_files(files)
    assert got.album_loudness_db == want.album_loudness_db and got.album_peak == want.album_peak
    assert [t.loudness_db for t in got.tracks] == [t.loudness_db for t in want.tracks]


def test_full_album_256(an, tmp_path):
    """256 tracks of 30 s, 44.1 kHz, 16-bit stereo: 16 distinct tracks, each behind 16 paths, against the WAV twins."""
    flacs, wavs = [], []
    rng = np.random.default_rng(0x256)
    for k in range(16):
        pcm = fe.test_pcm(rng, 2, 44100 * 30 + k, 16)
        f = tmp_path / f"src{k}.flac"
        f.write_bytes(fe.encode(pcm, 44100, 16, O(stereo="mid_side", subframe="auto", partition_order=4)))
        w = tmp_path / f"src{k}.wav"
        w.write_bytes(_wav_of(pcm, 44100, 16))
        for j in range(16):
            (tmp_path / f"t{k}_{j}.flac").symlink_to(f)
            (tmp_path / f"t{k}_{j}.wav").symlink_to(w)
            flacs.append(tmp_path / f"t{k}_{j}.flac")
            wavs.append(tmp_path / f"t{k}_{j}.wav")
    a, b = an.analyze_album_files(flacs), an.analyze_album_files(wavs)
    assert (a.album_loudness_db, a.album_gain_db, a.album_peak) == (b.album_loudness_db, b.album_gain_db, b.album_peak)
    assert [(t.loudness_db, t.peak, t.windows) for t in a.tracks] == [(t.loudness_db, t.peak, t.windows) for t in b.tracks]


def test_key14_values(an):
    import mp3rgain_amd as rg

    for bad in (-1, 2):
        with pytest.raises(rg.ReplayGainError):
            an.set_tuning(14, bad)
