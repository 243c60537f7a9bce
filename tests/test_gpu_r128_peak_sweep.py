"""EBU R 128 on the GPU: sample peak, true peak and the non-finite flag with the frame that decides them swept over every
position (tests/sweep_cases.py; the method is described in tests/test_gpu_peak_sweep.py).

The loudness kernel carries a frame's magnitude over 32-frame tiles (whole-piece and element-wise branches on the loader and
the consumer side), over lanes of S hops that start early to warm the filter up, and over the last run, which reads on through
the partial hop; the true-peak kernel works in tiles of 1024 frames, each with 48 / F frames of history, sixteen to a
workgroup.  The sample peak must be the marker's normalised magnitude bit for bit; the true peak is held to tests/r128ref.py
on that very track within the TP_TOL tests/test_gpu_r128.py derives.  A track whose position is odd carries a doublet, so its
true peak (about 1.25 x the marker) is an interpolated output between two samples, not a copy of one."""
import math
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import sweep_cases as sc  # noqa: E402
from test_gpu_r128 import TP_TOL  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture()
def an(_ctx):
    """The set-up of tests/test_gpu_r128.py."""
    _ctx.set_kernel(0)
    for key in (1, 2, 4, 10, 13):
        _ctx.set_tuning(key, 0)
    _ctx.set_tuning(14, 1)
    _ctx.set_tuning_r128(1, 0)
    _ctx.set_decoder_command(None)
    yield _ctx
    _ctx.set_tuning_r128(1, 0)
    _ctx.set_tuning(13, 0)


def _check(name, positions, res, want_peak, want_tp, rate):
    peaks = np.array([r.sample_peak for r in res])
    bad = np.flatnonzero(peaks != want_peak)
    assert bad.size == 0, (f"{name}: {bad.size} of {len(res)} sample peaks wrong, first at positions {positions[bad[:12]].tolist()}: "
                           f"got {peaks[bad[:12]].tolist()} want {want_peak[bad[:12]].tolist()}")
    tp = np.array([r.true_peak for r in res])
    err = np.abs(tp - want_tp) / want_tp
    print(f"{name}: {len(res)} positions, worst true-peak error {float(err.max()):.2e} relative (bar {TP_TOL:.0e})")
    bad = np.flatnonzero(~(err <= TP_TOL))
    assert bad.size == 0, (f"{name}: {bad.size} of {len(res)} true peaks off, first at positions {positions[bad[:12]].tolist()}: "
                           f"got {tp[bad[:12]].tolist()} want {want_tp[bad[:12]].tolist()}")
    assert all(r.flags == 0 and r.sample_rate == rate for r in res), name


def _sweep(an, sw, fmt, S, rot):
    import mp3rgain_amd as rg

    an.set_tuning_r128(1, S)
    chans, m = sw.tracks(fmt, rot)
    res = an.analyze_tracks_r128([rg.PcmTrack(ch, sw.rate) for ch in chans], true_peak=True)
    _check(f"{sw.name} {fmt} S{S}", sw.positions, res, sc.expected_peaks(m), sw.true_peak_refs(rot), sw.rate)


@pytest.mark.parametrize("S", [0, 1, 2, 5], ids=lambda s: f"S{s}")
@pytest.mark.parametrize("fmt", sc.FORMATS)
def test_peaks_at_every_position(an, fmt, S):
    """Four hops and 45 frames, stereo, every position: single markers at even positions, doublets at odd ones."""
    _sweep(an, sc.r128_exhaustive(), fmt, S, rot=7)


@pytest.mark.parametrize("S", [5, 7, 64], ids=lambda s: f"S{s}")
@pytest.mark.parametrize("fmt", sc.FORMATS)
def test_peaks_around_every_hop_boundary(an, fmt, S):
    """Forty hops and 333 frames: lanes of 5 and 7 hops and one lane for the whole track; the marker on both sides of every
    hop boundary and a tile and a piece away, and in the first and last 40 frames."""
    _sweep(an, sc.r128_structured(), fmt, S, rot=101)


@pytest.mark.parametrize("rate", sc.TP_RATES)
def test_true_peak_around_every_tile_boundary(an, rate):
    """17 tiles of 1024 frames and 100 frames, mono, the marker within 16 frames of every tile boundary (the sixteenth is the
    workgroup's): the outputs that peak there read history from the tile before.  The formats cycle with the tile, so one call
    mixes all three."""
    import mp3rgain_amd as rg

    sw = sc.tp_structured(rate)
    by_fmt = {fmt: np.flatnonzero([sc.tp_format_of(p) == fmt for p in sw.positions]) for fmt in sc.FORMATS}
    assert sorted(int(i) for idx in by_fmt.values() for i in idx) == list(range(len(sw)))
    tracks, order, m_all = [], [], []
    for fmt, idx in by_fmt.items():
        chans, m = sw.tracks(fmt, 0, pick=idx)
        tracks += [rg.PcmTrack(ch, rate) for ch in chans]
        order += [int(i) for i in idx]
        m_all += [int(v) for v in m]
    order = np.array(order)
    res = an.analyze_tracks_r128(tracks, true_peak=True)
    _check(sw.name, sw.positions[order], res, sc.expected_peaks(m_all), sw.true_peak_refs(0)[order], rate)


@pytest.mark.parametrize("S", [0, 1, 2], ids=lambda s: f"S{s}")
def test_nan_at_every_position(an, S):
    """f32, a NaN in every frame in turn, channel p % 2: the track is flagged, loudness and gain are NaN, the sample peak is
    the finite maximum, and the true peak drops exactly the interpolator outputs the NaN touches."""
    import mp3rgain_amd as rg

    sw = sc.r128_exhaustive()
    an.set_tuning_r128(1, S)
    res = an.analyze_tracks_r128([rg.PcmTrack(ch, sw.rate) for ch in sc.r128_nonfinite_tracks()], true_peak=True)
    want_sp, want_tp = sc.r128_nonfinite_refs()
    bad = [p for p, r in enumerate(res) if not (r.flags == 1 and math.isnan(r.loudness_lufs) and math.isnan(r.gain_db))]
    assert not bad, f"S{S}: {len(bad)} of {len(res)} tracks not flagged or not NaN, first at positions {bad[:12]}"
    sp = np.array([r.sample_peak for r in res])
    bad = np.flatnonzero(sp != want_sp)
    assert bad.size == 0, f"S{S}: sample peaks wrong at positions {bad[:12].tolist()}: got {sp[bad[:12]].tolist()} want {want_sp[bad[:12]].tolist()}"
    tp = np.array([r.true_peak for r in res])
    err = np.abs(tp - want_tp) / want_tp
    print(f"nan S{S}: worst true-peak error {float(np.nanmax(err)):.2e} relative (bar {TP_TOL:.0e})")
    bad = np.flatnonzero(~(err <= TP_TOL))
    assert bad.size == 0, f"S{S}: true peaks off at positions {bad[:12].tolist()}: got {tp[bad[:12]].tolist()} want {want_tp[bad[:12]].tolist()}"
