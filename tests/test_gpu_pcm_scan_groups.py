"""The route the four PCM scans share on files (rg_pcm_stats, rg_spectrum, rg_dynamic_range, rg_ancestry; the group driver in
mp3rgain_amd/csrc/rg_file_verify.hip): one call per scan over the same six small files, two of which the scan reads clean,
one with a dropped frame, and three that fail each in its own way.  Per file the status, the whole error text, the dropped
frames, that a failed file's record holds nothing but its status, and that a good file's record is the scan's host twin (route 0
of its seam) on the same PCM."""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import flacenc  # noqa: E402
import wavutil  # noqa: E402

from mp3rgain_amd import _capi  # noqa: E402
from mp3rgain_amd import replaygain as rgmod  # noqa: E402

pytestmark = pytest.mark.gpu

GOLD = Path(__file__).resolve().parent / "golden"
RG_ERR_IO, RG_ERR_FORMAT = -8, -9
ANC_OPTS = (2, 3)  # segments, granules: the host twin walks every alignment of every segment

# scan -> (the call on files -> (parsed results, the records' bytes), its record, its host twin on (descs, arena) -> records,
#          the noun of its refusals, its COMPLETE flag)
SCANS = {
    "stats": (lambda an, f: (an.pcm_stats(f), an.pcm_stats_raw(f)), _capi.PcmStatsRecord,
              lambda d, a: rgmod.pcm_stats_arena(None, 0, d, None, a), "PCM stats", _capi.STATS_COMPLETE),
    # (the spectrum's route 0 is the definition in float64, which f32 kernels meet within a tolerance, not bit for bit: its twin
    # for bytes is route 2, the kernels' arithmetic on the host, as in tests/test_gpu_spectrum_files.py; route 0 is held below
    # in what it defines exactly)
    "spectrum": (lambda an, f: (an.spectrum(f), an.spectrum_raw(f)[0]), _capi.SpectrumRecord,
                 lambda d, a: rgmod.spectrum_arena(None, 2, d, a, bands=False)[0], "spectrum", _capi.SPEC_COMPLETE),
    "dr": (lambda an, f: (an.dynamic_range(f), an.dynamic_range_raw(f)), _capi.DrRecord,
           lambda d, a: rgmod.dr_arena(None, 0, d, a), "dynamic range", _capi.DR_COMPLETE),
    "ancestry": (lambda an, f: (an.ancestry(f, *ANC_OPTS), an.ancestry_raw(f, *ANC_OPTS)), _capi.AncestryRecord,
                 lambda d, a: rgmod.ancestry_arena(None, 0, d, a, *ANC_OPTS, counts=False)[0], "ancestry scan", _capi.ANC_COMPLETE),
}


@pytest.fixture()
def an(_ctx):
    _ctx.set_tuning(14, 1)
    _ctx.set_tuning(13, 0)
    _ctx.set_decoder_command(None)
    return _ctx


def _f64_wav(frames):
    """a 2-channel WAV of 64-bit floats: a sample kind the staging does not lay out"""
    import struct

    body = np.zeros(2 * frames, "<f8").tobytes()
    fmt = struct.pack("<HHIIHH", 3, 2, 44100, 44100 * 16, 16, 64)
    chunks = b"fmt " + struct.pack("<I", len(fmt)) + fmt + b"data" + struct.pack("<I", len(body)) + body
    return b"RIFF" + struct.pack("<I", 4 + len(chunks)) + b"WAVE" + chunks


@pytest.fixture(scope="module")
def six(tmp_path_factory):
    """The files, and for those a scan reads: file index -> (planes as the arena holds them, sample rate, frames dropped); the
    MP3's planes are the device decoder's and come in the test."""
    tmp = tmp_path_factory.mktemp("pcm_scan_groups")

    def write(name, data):
        (tmp / name).write_bytes(data)
        return tmp / name

    good = wavutil.test_signal("s16", 44100, 4000, 2, 5)
    name, stream, kept, dropped = next(v for v in flacenc.damaged_variants() if v[0] == "bitflip")
    assert dropped == 1
    mp3 = min((GOLD / "mp3").glob("*.mp3"), key=lambda p: (p.stat().st_size, p.name))
    files = [write("good.wav", wavutil.wav_bytes(good, 44100, "s16")),
             tmp / "missing.wav",
             write("nine.wav", wavutil.wav_bytes([np.arange(8) + c for c in range(9)], 44100, "s16")),
             write("doubles.wav", _f64_wav(8)),
             write("bitflip.flac", stream),
             mp3]
    pcm = {0: (wavutil.planar_for_oracle(good, "s16"), 44100, 0), 4: ([kept[c].astype(np.int16) for c in range(2)], 44100, 1)}
    return files, pcm


@pytest.mark.parametrize("scan", SCANS)
def test_six_files_one_call(an, six, scan):
    call, record, twin, noun, complete = SCANS[scan]
    files, pcm = six
    decoded, info = an.decode_mp3_device(files[5].read_bytes())  # the smallest golden stream: the device decoder takes it
    pcm = dict(pcm)
    pcm[5] = ([np.ascontiguousarray(ch) for ch in decoded], int(info.sample_rate), 0)
    res, raw = call(an, files)
    size = C.sizeof(record)
    assert len(res) == 6 and len(raw) == 6 * size
    recs = [record.from_buffer_copy(raw[size * k:size * (k + 1)]) for k in range(6)]
    # the three that fail, each alone: the status, the whole text, and nothing else in the record
    refused = {1: (RG_ERR_IO, f"Failed to open: {files[1]}"),
               2: (RG_ERR_FORMAT, f"No {noun} (9 channels, more than 8): {files[2]}"),
               3: (RG_ERR_FORMAT, f"No {noun} (64-bit float, not 8, 16, 24 or 32-bit integer or 32-bit float PCM): {files[3]}")}
    for k, (code, text) in refused.items():
        assert res[k].error is not None and (res[k].error.code, str(res[k].error)) == (code, text), (k, str(res[k].error))
        assert recs[k].status == code and raw[size * k + 4:size * (k + 1)] == bytes(size - 4), k
        assert res[k].dropped_frames == 0
    # the three the scan reads: the host twin's record on the same PCM, but for the frames the route dropped
    keys = sorted(pcm)
    tracks = [rgmod.PcmTrack(pcm[k][0], pcm[k][1]) for k in keys]
    arena, descs = rgmod.pack_tracks(tracks)
    for k, want in zip(keys, twin(list(descs)[:len(keys)], arena)):
        dropped = pcm[k][2]
        assert res[k].error is None and recs[k].status == 0, (k, str(res[k].error))
        assert res[k].dropped_frames == recs[k].dropped_frames == dropped, (k, recs[k].dropped_frames)
        assert (recs[k].frames, recs[k].channels, recs[k].sample_rate) == (len(pcm[k][0][0]), len(pcm[k][0]), pcm[k][1]), k
        assert want.status == 0 and want.dropped_frames == 0 and want.flags & complete
        want.dropped_frames = dropped
        if dropped:
            want.flags &= ~complete
        assert bytes(recs[k]) == bytes(want), (k, recs[k].flags, want.flags)
    if scan == "spectrum":  # route 0: the frames it analysed and skipped, and every flag that is not a verdict on the energies
        exact = _capi.SPEC_SHORT | _capi.SPEC_NONFINITE | _capi.SPEC_COMPLETE
        for k, want in zip(keys, rgmod.spectrum_arena(None, 0, list(descs)[:len(keys)], arena, bands=False)[0]):
            r = recs[k]
            assert (r.frames, r.channels, r.format, r.flags & exact) == (want.frames, want.channels, want.format, (want.flags & exact) & ~(complete if pcm[k][2] else 0))
            assert [(c.analysed_frames, c.skipped_frames) for c in r.ch[:r.channels]] == [(c.analysed_frames, c.skipped_frames) for c in want.ch[:r.channels]]
