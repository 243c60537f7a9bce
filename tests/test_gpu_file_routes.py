"""What the per-file calls share (csrc/rg_files.h: LoadOpts, for_each_group, FileGroup): a call leaves the context as it found
it -- the decoder command and the track index are a call's options, not state -- and a failing file keeps its place, its code
and its own text however the list is cut into groups (tuning key 13).  Inputs of a few thousand samples; nothing here needs
a measured number."""
import dataclasses
import io
import os
import struct
import sys
import wave
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import flac_md5_cases as fm  # noqa: E402
import flacenc  # noqa: E402
from wavutil import test_signal, wav_bytes  # noqa: E402

from mp3rgain_amd import _capi, flacdec, mp3dec  # noqa: E402

test_signal.__test__ = False
pytestmark = pytest.mark.gpu

GOLD = Path(__file__).resolve().parent / "golden" / "mp3"
RG_ERR_IO, RG_ERR_FORMAT = -8, -9
SMALL_GROUPS = 24 * 30000  # key 13: 30000 bytes of files per group -- one or two of the files here


@pytest.fixture()
def an(_ctx):
    def defaults():
        _ctx.set_kernel(0)
        for key in (1, 2, 13):
            _ctx.set_tuning(key, 0)
        _ctx.set_tuning(6, 3)
        _ctx.set_tuning(14, 1)
        _ctx.set_channel_mode_r128("pair")
        _ctx.set_decoder_command(None)

    defaults()
    yield _ctx
    defaults()


def _write(tmp_path, name, data):
    p = tmp_path / name
    p.write_bytes(data)
    return p


def _bits(x):
    """A result, or the error in its place, as something == compares bit for bit (NaN included)."""
    if isinstance(x, Exception):
        return (x.code, str(x))
    if dataclasses.is_dataclass(x):
        return tuple(_bits(getattr(x, f.name)) for f in dataclasses.fields(x))
    return x.hex() if isinstance(x, float) else x


def _wav_params(data):
    with wave.open(io.BytesIO(data)) as w:
        return w.getnchannels(), 8 * w.getsampwidth(), w.getframerate(), w.getnframes()


def _flac(rng, n, channels=2, bps=16):
    pcm = flacenc.test_pcm(rng, channels, n, bps)
    data = flacenc.encode(pcm, 44100, bps, flacenc.Options(block_size=576))
    _, _, got, info = flacdec.decode(data)
    assert np.array_equal(got, pcm) and int(info.dropped_frames) == 0  # a good one decodes, to what went in
    return data, fm.md5(pcm, bps)


def _wav(seed, n, nch=2, rate=44100):
    data = wav_bytes(test_signal("s16", rate, n, nch, seed=seed), rate, "s16")
    assert _wav_params(data) == (nch, 16, rate, n)
    return data


@pytest.mark.parametrize("key6", [3, 0], ids=["loader-pipeline", "host-loaders"])
def test_a_call_leaves_the_context_as_it_found_it(an, tmp_path, key6):
    """Both places a call's options reach: the loader pipeline (tuning key 6 = 3) and the host loaders of load_many (0)."""
    import mp3rgain_amd as rg

    an.set_tuning(6, key6)
    rng = np.random.default_rng(41)
    # the stand-in of test_decoder_command_and_file_type: a WAV stream behind a 4-byte prefix that the decoder command strips
    standin = _write(tmp_path, "x.flac", b"JUNK" + _wav(5, 4000))
    flac, flac_md5 = _flac(rng, 3000)
    good_flac = _write(tmp_path, "good.flac", flac)
    mp3 = GOLD / "v1_44k_ms_mixed.mp3"
    ok_wav = _write(tmp_path, "ok.wav", _wav(6, 5000))
    files = [good_flac, standin, mp3]
    an.set_decoder_command("tail -c +5 {}")
    try:
        first = an.analyze_track_file(standin)
        assert first.sample_rate == 44100 and first.windows > 0

        v = an.verify_flac(files)
        assert v[0].error is None and v[0].md5_decoded == flac_md5 and [r.error.code for r in v[1:]] == [RG_ERR_FORMAT] * 2
        assert _bits(an.analyze_track_file(standin)) == _bits(first)

        m = an.verify_mp3(files)
        assert m[2].error is None and [r.error.code for r in m[:2]] == [RG_ERR_FORMAT] * 2
        assert _bits(an.analyze_track_file(standin)) == _bits(first)

        # had the command been run, its output would be a WAV stream this route accepts: it was withheld
        r = an.rip_checksums(files, disc=False)
        raw = an.rip_checksums_raw(files, disc=False)
        assert r[0].error is None and r[0].frames == 3000 and r[2].error.code == RG_ERR_FORMAT
        assert r[1].error.code == RG_ERR_FORMAT and "Failed to probe format" in str(r[1].error) and str(standin) in str(r[1].error)
        assert (r[1].crc32, r[1].crc32_nonnull, r[1].arv1, r[1].arv2, r[1].frames, r[1].null_samples) == (0,) * 6
        assert _capi.RipRecord.from_buffer_copy(raw[48:96]).status == RG_ERR_FORMAT and raw[52:96] == bytes(44)
        assert _bits(an.analyze_track_file(standin)) == _bits(first)

        # a call's track index is that call's alone
        res = an.analyze_track_files([ok_wav, standin], track_index=0)
        assert [isinstance(x, rg.ReplayGainResult) for x in res] == [True, True] and _bits(res[1]) == _bits(first)
        assert an.verify_mp3(files)[2].error is None
        with pytest.raises(rg.ReplayGainError, match=r"Track index 1 out of range \(file has 1 audio track\(s\)\)"):
            an.analyze_track_file(ok_wav, 1)
        assert _bits(an.analyze_track_file(ok_wav)) == _bits(res[0])
    finally:
        an.set_decoder_command(None)


@pytest.fixture(scope="module")
def shelf(tmp_path_factory):
    """The files of the group tests, each checked here, on the CPU, to be what its name says."""
    tmp = tmp_path_factory.mktemp("shelf")
    rng = np.random.default_rng(42)
    s = {"missing": tmp / "missing.flac", "mp3": [GOLD / "v1_44k_ms_mixed.mp3", GOLD / "v1_44k_intensity_ms_short.mp3"]}
    assert not s["missing"].exists()
    for f in s["mp3"]:
        pcm, info = mp3dec.decode(f.read_bytes())
        assert info.sample_rate == 44100 and pcm.shape[1] > 1152 and f.stat().st_size < 30000
    flacs = [_flac(rng, n) for n in (3000, 2 * 1152 + 77, 4001, 3500, 2941, 3333)]
    s["flac"] = [_write(tmp, f"{k}.flac", data) for k, (data, _) in enumerate(flacs)]
    s["flac_md5"] = {s["flac"][k]: md5 for k, (_, md5) in enumerate(flacs)}
    s["wav"] = [_write(tmp, f"{k}.wav", _wav(50 + k, n)) for k, n in enumerate((4000, 3001, 5003))]
    junk = bytes(rng.integers(0, 128, 3000, dtype=np.uint8))  # no byte 0xFF: no MPEG sync word, and no container's magic
    assert junk[:4] not in (b"RIFF", b"fLaC", b"OggS", b"ID3\x04") and b"ftyp" not in junk[:12]
    s["junk"] = _write(tmp, "junk.bin", junk)
    # refused by the two analysis routes: a RIFF/WAVE stream whose header gives no sample rate
    zero = bytearray(_wav(60, 3000))
    at = zero.index(b"fmt ") + 12
    zero[at:at + 4] = struct.pack("<I", 0)
    assert _wav_params(bytes(zero)) == (2, 16, 0, 3000)
    s["zero_rate"] = _write(tmp, "zero_rate.wav", bytes(zero))
    return s


def _groups(files, budget=SMALL_GROUPS):
    """file_groups (csrc/rg_files.hip) on the CPU: 24 bytes of PCM estimated per byte of file, a group closed before the file
    that would take it over the budget, a missing file counting nothing."""
    groups, est = [[]], 0
    for i, f in enumerate(files):
        sz = 24 * (os.path.getsize(f) if os.path.exists(f) else 0)
        if groups[-1] and est + sz > budget:
            groups.append([])
            est = 0
        groups[-1].append(i)
        est += sz
    return groups


def _cut_into_groups(files):
    """The small budget really cuts this list: the failing files (0, 4, 8) lie in three groups, file 4 neither in the first
    group nor first in its own (so `first` and `i` both count), and without the budget the list is one group."""
    groups = _groups(files)
    of = {i: k for k, g in enumerate(groups) for i in g}
    assert len(groups) >= 3 and len({of[0], of[4], of[8]}) == 3 and of[4] > 0 and groups[of[4]][0] < 4, groups
    assert len(_groups(files, 1 << 40)) == 1


def _both_groupings(an, call):
    an.set_tuning(13, 0)
    whole = call()
    an.set_tuning(13, SMALL_GROUPS)
    cut = call()
    an.set_tuning(13, 0)
    return whole, cut


def _check_results(files, failing, whole, cut):
    """Per-file results or errors of one call under both groupings; `failing`: {position: code}."""
    assert len(whole) == len(cut) == len(files)
    for i, f in enumerate(files):
        assert _bits(whole[i]) == _bits(cut[i]), (i, whole[i], cut[i])
        if i in failing:
            assert isinstance(cut[i], Exception) and cut[i].code == failing[i] and str(f) in str(cut[i]), (i, cut[i])
        else:
            assert not isinstance(cut[i], Exception), (i, cut[i])


def _check_records(files, failing, size, whole, cut, raw_whole, raw_cut):
    """The same for a call whose status lives in its records; the raw records byte for byte, and zero where a file failed."""
    assert raw_whole == raw_cut and len(raw_cut) == size * len(files)
    for i, f in enumerate(files):
        assert (whole[i].error is None) == (cut[i].error is None) == (i not in failing), (i, cut[i].error)
        if i in failing:
            assert _bits(whole[i].error) == _bits(cut[i].error) and cut[i].error.code == failing[i] and str(f) in str(cut[i].error), (i, cut[i].error)
            assert struct.unpack_from("<i", raw_cut, size * i)[0] == failing[i] and raw_cut[size * i + 4:size * (i + 1)] == bytes(size - 4)


@pytest.mark.parametrize("r128", [False, True], ids=["replaygain", "r128"])
def test_failing_files_keep_their_place_across_groups_in_the_analysis_calls(an, shelf, r128):
    fl, wv, mp3 = shelf["flac"], shelf["wav"], shelf["mp3"]
    files = [shelf["missing"], fl[0], mp3[0], wv[0], shelf["zero_rate"], fl[1], mp3[1], wv[1], shelf["junk"]]
    failing = {0: RG_ERR_IO, 4: RG_ERR_FORMAT, 8: RG_ERR_FORMAT}
    _cut_into_groups(files)
    if r128:
        whole, cut = _both_groupings(an, lambda: an.analyze_track_files_r128(files, true_peak=True, dynamics=True))
    else:
        whole, cut = _both_groupings(an, lambda: an.analyze_track_files(files))
    _check_results(files, failing, whole, cut)
    assert "Failed to open" in str(cut[0]) and all("Failed to probe format" in str(cut[i]) for i in (4, 8))
    assert [cut[i].sample_rate for i in range(9) if i not in failing] == [44100] * 6


def test_failing_files_keep_their_place_across_groups_in_flac_verify(an, shelf):
    fl = shelf["flac"]
    files = [shelf["junk"], fl[0], fl[1], fl[2], shelf["mp3"][0], fl[3], fl[4], fl[5], shelf["missing"]]
    failing = {0: RG_ERR_FORMAT, 4: RG_ERR_FORMAT, 8: RG_ERR_IO}
    _cut_into_groups(files)
    whole, cut = _both_groupings(an, lambda: an.verify_flac(files))
    raw_whole, raw_cut = _both_groupings(an, lambda: an.verify_flac_raw(files))
    _check_records(files, failing, len(raw_cut) // len(files), whole, cut, raw_whole, raw_cut)
    assert "Not a native FLAC stream" in str(cut[4].error)  # an MPEG stream: refused after it was staged with the others
    assert all(cut[i].md5_decoded == shelf["flac_md5"][files[i]] and cut[i].complete for i in range(9) if i not in failing)


def test_failing_files_keep_their_place_across_groups_in_rip_checksums(an, shelf):
    fl, wv = shelf["flac"], shelf["wav"]
    files = [shelf["missing"], fl[0], wv[0], fl[1], shelf["mp3"][0], wv[1], fl[2], wv[2], shelf["junk"]]
    failing = {0: RG_ERR_IO, 4: RG_ERR_FORMAT, 8: RG_ERR_FORMAT}
    _cut_into_groups(files)
    flags = [0, _capi.RIP_FIRST_TRACK, 0, 0, 0, 0, 0, _capi.RIP_LAST_TRACK, 0]  # they travel with their files, or the sums change
    whole, cut = _both_groupings(an, lambda: an.rip_checksums(files, flags=flags))
    raw_whole, raw_cut = _both_groupings(an, lambda: an.rip_checksums_raw(files, flags=flags))
    _check_records(files, failing, 48, whole, cut, raw_whole, raw_cut)
    assert "an MPEG stream" in str(cut[4].error)  # refused after it was staged with the others
    assert all(cut[i].frames >= 2 * 1152 + 77 and cut[i].complete for i in range(9) if i not in failing)
