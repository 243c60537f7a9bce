"""The HIP MP3 decoder (rg_mp3dev.hip) against the float64 reference decoder (oracle/mp3_refdec.py), by itself.

tests/test_gpu_mp3.py asserts device PCM == host PCM on the golden streams.  Here, on the streams generated at test
time (tools/mp3_refdec_check.py: every rate row and channel mode, long window-switching sequences, global_gain 60-255,
quantised values up to 8000 -- beyond the kernels' LDS table of x^(4/3) and into its computed path) and on one encode per
MPEG version, every route of tuning key 6
  * equals mp3dec.decode bit for bit, and
  * meets the bar of tests/test_mp3_refdec.py against the float64 reference directly: rms and max of the error within
    4 float32 floors of the operation, per stream and per 576-sample block, floors computed live.
Then the file-level entry point on three generated files, one per MPEG version: loudness, peak and every histogram bin
are the CPU oracle's on the host decoder's PCM.  One process, one context; a failing step is not repeated."""
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
for _p in (ROOT, ROOT / "oracle", ROOT / "tools", ROOT / "tests"):
    if str(_p) not in sys.path:
        sys.path.insert(0, str(_p))

import mp3_refdec_check as C  # noqa: E402
from mp3rgain_amd import mp3dec  # noqa: E402

pytestmark = pytest.mark.gpu
DEFAULT_ROUTE = 3
INPUTS = [(k, n) for k, n in C.input_names() if k != "golden"]


@pytest.mark.parametrize("kind,name", INPUTS, ids=[n for _, n in INPUTS])
def test_device_decoder_equals_the_host_and_is_within_the_float32_floor(_ctx, kind, name):
    data, st = C.load_input(kind, name)
    r64, r32 = C.references(kind, name)
    want, wi = mp3dec.decode(data)
    try:
        for route in (1, 2, 3):
            _ctx.set_tuning(6, route)
            got, gi = _ctx.decode_mp3_device(data)
            assert (gi.frames, gi.channels, gi.sample_rate, gi.audio_frames, gi.skipped_frames) == (wi.frames, wi.channels, wi.sample_rate, wi.audio_frames, wi.skipped_frames)
            assert got.shape == want.shape == r64.shape
            m = C.measure(got, r64, r32)
            print(f"{name} route {route}: peak {m['peak']:.3g}; in floors: stream rms {m['stream_rms']:.2f} max {m['stream_max']:.2f}, "
                  f"block rms {m['block_rms']:.2f} max {m['block_max']:.2f}")
            assert not m["bad"], (route, m["bad"], C.name_stage(st, got, r64))
            if not np.array_equal(got, want):
                d = np.abs(got.astype(np.float64) - want.astype(np.float64))
                bad = np.argwhere(d > 0)
                raise AssertionError(f"route {route}: {len(bad)} of {got.size} samples differ from the host decoder's, max {d.max():.3g} "
                                     f"(peak {np.abs(want).max():.3g}), first at {bad[0]}")
    finally:
        _ctx.set_tuning(6, DEFAULT_ROUTE)


@pytest.mark.parametrize("name", ["gen_44100_stereo_usual_s1", "gen_22050_joint_is_usual_s1", "gen_12000_mono_usual_s1"])
def test_generated_files_through_the_file_level_entry_point(_ctx, oracle, tmp_path, name):
    import mp3rgain_amd as rg

    data, st = C.load_input("generated", name)
    f = tmp_path / f"{name}.mp3"
    f.write_bytes(data)
    pcm, info = mp3dec.decode(data)
    want, want_hist = oracle.analyze_pcm(pcm[0], pcm[1] if pcm.shape[0] == 2 else None, info.sample_rate)
    assert int(want_hist.sum()) > 0, "the file must carry at least one counted window"
    _ctx.set_kernel(0)
    try:
        for route in (1, 2, 3):
            _ctx.set_tuning(6, route)
            got = _ctx.analyze_track_file(f)
            assert (got.loudness_db, got.peak, got.sample_rate, got.windows) == (want["loudness_db"], want["peak"], info.sample_rate, int(want_hist.sum())), route
            dev, _ = _ctx.decode_mp3_device(data)
            res, hist = _ctx.analyze_tracks([rg.PcmTrack([dev[c] for c in range(dev.shape[0])], info.sample_rate)], return_histograms=True)
            assert np.array_equal(hist[0], want_hist), route
            assert (res[0].loudness_db, res[0].peak) == (want["loudness_db"], want["peak"])
    finally:
        _ctx.set_tuning(6, DEFAULT_ROUTE)
