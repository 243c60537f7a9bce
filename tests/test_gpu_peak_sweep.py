"""ReplayGain 1.0 on the GPU: the peak and the non-finite flag with the one frame that decides them swept over every position.

A sum notices a dropped or doubled frame; a maximum or an "any" flag observes only the frame that holds the extreme, and in the
differential tests (tests/test_gpu_parity.py, tests/test_gpu_scale.py) that frame lies wherever the noise put it.  Here one
batch is a whole sweep (tests/sweep_cases.py): hundreds or thousands of short tracks, identical but for one marker sample of at
least 0.9 of full scale over a background of at most 2^-7, track i carrying it at position p_i.  The expected peak is the marker's
normalised magnitude, bit for bit, and needs nothing from the code under test; every track's marker has its own magnitude, so a
peak credited to a neighbouring track shows as well.  tests/test_peak_sweep_cpu.py holds the inputs to their preconditions.

No histogram bin is asserted on a marker track: a loud impulse in a quiet track is the signal class the transient-moment kernels
flag as imprecise when they are forced (docs/HISTORY.md, section 4).  The non-finite sweep, over plain noise, asserts every bin."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import sweep_cases as sc  # noqa: E402

pytestmark = pytest.mark.gpu


def _run(an, sw, fmt, rot, album=False):
    import mp3rgain_amd as rg

    chans, m = sw.tracks(fmt, rot)
    tracks = [rg.PcmTrack(ch, sw.rate) for ch in chans]
    if album:
        res = an.analyze_album(tracks)
        got, album_peak = res.tracks, res.album_peak
    else:
        got, album_peak = an.analyze_tracks(tracks), None
    want = sc.expected_peaks(m)
    peaks = np.array([g.peak for g in got])
    bad = np.flatnonzero(peaks != want)
    assert bad.size == 0, (f"{sw.name} {fmt}: {bad.size} of {len(sw)} peaks wrong, first at positions {sw.positions[bad[:12]].tolist()}: "
                           f"got {peaks[bad[:12]].tolist()} want {want[bad[:12]].tolist()}")
    windows = np.array([g.windows for g in got])
    bad = np.flatnonzero(windows != sc.windows_of(sw.rate, sw.frames))
    assert bad.size == 0, f"{sw.name} {fmt}: windows {windows[bad[:12]].tolist()} at positions {sw.positions[bad[:12]].tolist()}"
    assert not any(g.flags & 1 for g in got) and all(g.sample_rate == sw.rate for g in got)
    return album_peak, want


EXHAUSTIVE = [(rate, nch, fmt) for rate in sc.RG1_RATES for nch in (2, 1) for fmt in sc.rg1_exhaustive(rate, nch).formats]


@pytest.mark.parametrize("rate,nch,fmt", EXHAUSTIVE, ids=[f"{r}-{n}ch-{f}" for r, n, f in EXHAUSTIVE])
def test_peak_at_every_position(analyzer, rate, nch, fmt):
    """Two windows and 37 frames, the marker in every frame: every piece, tile and turn residue, both window ends, the three
    moment modes of the first window, the partial window's scalar tail; W = 400 (servo form) and W = 1102 (classic form)."""
    sw = sc.rg1_exhaustive(rate, nch)
    _run(analyzer, sw, fmt, rot=sc.FORMATS.index(fmt) * (len(sw) // 3) + nch)


@pytest.mark.parametrize("nch", [2, 1], ids=["s16-stereo", "f32-mono"])
def test_peak_around_every_window_boundary(analyzer, nch):
    """77 windows and 5 frames: with 37 windows per lane, two full lanes, a ragged third (whose row re-reads the track's first
    window) and a partial window; the marker on both sides of every window boundary and a tile, a turn and a piece away."""
    sw = sc.rg1_structured(nch)
    _run(analyzer, sw, sw.formats[0], rot=len(sw) // 2)


@pytest.mark.parametrize("fmt", sc.FORMATS)
def test_album_peak_over_the_sweep(analyzer, fmt):
    sw = sc.rg1_exhaustive(8000, 2)
    album_peak, want = _run(analyzer, sw, fmt, rot=sc.FORMATS.index(fmt) * 200 + 11, album=True)
    assert album_peak == float(want.max()) == 1.0


@pytest.mark.parametrize("fmt", sc.FORMATS)
def test_find_peak_amplitude_at_every_sample(_ctx, oracle, fmt):
    """Three channels of 700 frames, the marker at every sample of the planar block (rg_find_peak_pcm scans all channels; no
    kernel choice or tuning reaches that scan, so it runs once and not once per column)."""
    import mp3rgain_amd as rg

    total = sc.FIND_PEAK_FRAMES * sc.FIND_PEAK_CHANNELS
    bad = []
    for index in range(total):
        chans, m = sc.find_peak_track(index, fmt)
        pk = _ctx.find_peak_amplitude(rg.PcmTrack(chans, 8000))
        want = oracle.find_peak(chans, sc.NP_TYPE[fmt])
        if not (pk.peak == want == abs(m) / 32768.0 and pk.peak_pcm == want * 32768.0):
            bad.append((index, pk.peak, want, m))
    assert not bad, f"{len(bad)} of {total} wrong, first {bad[:8]}"


# ---- the non-finite flag ------------------------------------------------------------------------------------------------------
_NONFINITE = {}


def _nonfinite_set(oracle, what):
    """(tracks, clean track, the oracle's results for every track and the clean one): the oracle runs once per `what`."""
    if what not in _NONFINITE:
        tracks, clean = sc.nonfinite_tracks(oracle, what)
        hist = np.zeros((len(tracks), oracle.HIST), dtype=np.uint8)  # at most three windows in a bin
        res = []
        for i, (l, r) in enumerate(tracks):
            w, wh = oracle.analyze_pcm(l, r, sc.NONFINITE_RATE)
            res.append(w)
            hist[i] = wh
        _NONFINITE[what] = (tracks, clean, res, hist, oracle.analyze_pcm(clean[0], clean[1], sc.NONFINITE_RATE))
    return _NONFINITE[what]


def _same_peak(a, b):
    return a == b or (np.isinf(a) and np.isinf(b))


def _nonfinite_sweep(an, oracle, what):
    import mp3rgain_amd as rg

    tracks, clean, want, want_hist, (cw, cwh) = _nonfinite_set(oracle, what)
    n = len(tracks)
    assert n == sc.NONFINITE_FRAMES and int(want_hist[:, 2000].sum()) > n  # the poisoned windows are in the NaN bin
    poisoned = [rg.PcmTrack(ch, sc.NONFINITE_RATE) for ch in tracks]
    clean_track = rg.PcmTrack(clean, sc.NONFINITE_RATE)
    # first call: every track poisoned; second call: every other one clean, on the same buffers, so a flag, a first-bad
    # record or a NaN bin that outlives its batch shows
    for second in (False, True):
        batch = [clean_track if second and i % 2 == 0 else poisoned[i] for i in range(n)]
        got, h = an.analyze_tracks(batch, return_histograms=True)
        bad = []
        for i in range(n):
            if second and i % 2 == 0:
                ok = np.array_equal(h[i], cwh) and got[i].loudness_db == cw["loudness_db"] and got[i].peak == cw["peak"] and not got[i].flags & 1
            else:
                ok = (np.array_equal(h[i], want_hist[i]) and got[i].loudness_db == want[i]["loudness_db"] and got[i].flags & 1
                      and _same_peak(got[i].peak, want[i]["peak"]))
            if not ok:
                bad.append(i)
        assert not bad, (f"{what}, call {1 + second}: {len(bad)} of {n} positions wrong, first {bad[:12]}; position {bad[0]}: flags "
                         f"{got[bad[0]].flags} peak {got[bad[0]].peak} bins {np.flatnonzero(h[bad[0]]).tolist()} "
                         f"want peak {want[bad[0]]['peak']} bins {np.flatnonzero(want_hist[bad[0]]).tolist()}")


@pytest.mark.parametrize("what", list(sc.NONFINITE_KINDS))
def test_non_finite_sample_at_every_position(analyzer, oracle, what):
    """tests/test_gpu_parity.py places a NaN or an Inf at eight hand-picked positions; this is all 837 of a track of two
    windows and 37 frames, in channel p % 2: identical histogram (the NaN bin from the poisoned window on, the dropped window
    of an Inf in a window's last frame), equal loudness and peak, the flag set."""
    _nonfinite_sweep(analyzer, oracle, what)


@pytest.mark.parametrize("what", list(sc.NONFINITE_KINDS))
def test_non_finite_sample_at_every_position_auto_mode(_ctx, oracle, what):
    _ctx.set_kernel(0)
    for key in (1, 2, 3, 4):
        _ctx.set_tuning(key, 0)
    _nonfinite_sweep(_ctx, oracle, what)
