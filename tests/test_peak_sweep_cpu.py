"""Preconditions of the position sweeps (tests/sweep_cases.py), on the references alone: what the two GPU modules
(tests/test_gpu_peak_sweep.py, tests/test_gpu_r128_peak_sweep.py) take for granted about their own inputs."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import r128ref  # noqa: E402
import sweep_cases as sc  # noqa: E402
from test_gpu_r128 import TP_TOL  # noqa: E402

SWEEPS = sc.all_sweeps()
IDS = [s.name for s in SWEEPS]


def test_the_set_is_what_the_gpu_modules_run():
    assert len(SWEEPS) == 10 and len(set(IDS)) == 10
    assert [len(s) for s in SWEEPS[:4]] == [837, 837, 2241, 2241]
    assert sc.r128_exhaustive().frames == 4 * 800 + 45 and sc.r128_structured().frames == 40 * 800 + 333
    assert sc.rg1_structured(2).frames == 77 * 400 + 5 and sc.TP_FRAMES == 17 * 1024 + 100


@pytest.mark.parametrize("sw", SWEEPS, ids=IDS)
def test_markers_dwarf_the_background_and_are_unique(sw):
    bg = max(int(np.max(np.abs(c))) for c in sw.background)
    assert 0 < bg <= sc.BACKGROUND_MAX
    for rot in (0, 1, len(sw) // 3, len(sw) - 1):
        m = sc.markers(len(sw), rot)
        a = np.abs(m)
        assert int(a.min()) >= 32 * bg and int(a.min()) >= 16384 and int(a.max()) == 32768
        assert len(np.unique(a)) == len(sw)
        assert int(m[(len(sw) - rot) % len(sw)]) == -32768  # exactly negative full scale, once in every call
        flips = int(np.count_nonzero(np.sign(m[1:]) != np.sign(m[:-1])))
        assert flips >= len(sw) - 2  # the sign alternates (but where an odd list wraps round)
    assert sw.formats and all(sw.arena_bytes(fmt) < sc.MAX_ARENA for fmt in sw.formats)


def test_find_peak_tracks_meet_the_same_preconditions(oracle):
    """The three-channel track of the find_peak sweep: one marker per sample of the planar block, each its own magnitude."""
    total = sc.FIND_PEAK_FRAMES * sc.FIND_PEAK_CHANNELS
    bg = max(int(np.max(np.abs(c))) for c in sc.find_peak_background())
    a = np.abs(sc.markers(total))
    assert total == 2100 and 0 < bg <= sc.BACKGROUND_MAX and int(a.min()) >= 32 * bg and len(np.unique(a)) == total
    for fmt in sc.FORMATS:
        for index in (0, 699, 700, 1399, 1400, 2099):
            chans, m = sc.find_peak_track(index, fmt)
            assert chans[index // 700][index % 700] == sc.as_format(m, fmt)
            assert sum(int(np.count_nonzero(np.abs(r128ref.normalise(c)) > 0.5)) for c in chans) == 1
            assert oracle.find_peak(chans, sc.NP_TYPE[fmt]) == abs(m) / 32768.0


@pytest.mark.parametrize("fmt", sc.FORMATS)
def test_every_format_holds_the_same_signal(fmt):
    """The one float64 reference serves all three formats: each normalises to the 16-bit grid / 32768, bit for bit."""
    sw = sc.rg1_exhaustive(8000, 2)
    tracks, m = sw.tracks(fmt, rot=5)
    for i in (0, 1, 399, 400, 832, 836):
        want = sw.marked(i, rot=5)
        for c in range(2):
            assert tracks[i][c].dtype == sc.NP_TYPE[fmt]
            assert np.array_equal(r128ref.normalise(tracks[i][c]), sc.unit(want[c]))
        p = int(sw.positions[i])
        assert want[p % 2][p] == m[i] and r128ref.sample_peak(tracks[i]) == sc.expected_peaks(m)[i]


@pytest.mark.parametrize("sw", SWEEPS, ids=IDS)
def test_lists_hit_every_residue_and_both_sides_of_every_boundary(sw):
    p = sw.positions
    assert len(np.unique(p)) == len(p) and p.min() >= 0 and p.max() < sw.frames
    for mod in (4, 12, 16, 32):
        assert set(int(r) for r in p % mod) == set(range(mod)), (sw.name, mod)
    have = set(int(q) for q in p)
    if "exhaustive" in sw.name:
        assert have == set(range(sw.frames))
    else:
        assert len(sw.boundaries) >= 17
        for b in sw.boundaries:
            assert b - 1 in have and b in have, (sw.name, b)
    if sw.nch == 2:  # both channels carry markers
        assert set(int(c) for c in p % 2) == {0, 1}


def test_structure_lists_are_built_from_the_kernels_own_steps():
    rg = sc.rg1_structured(2)
    have = set(int(q) for q in rg.positions)
    w = sc.window(rg.rate)
    assert w == 400 and rg.frames // w == 77
    for k in range(1, 78):
        for d in sc.RG1_OFFSETS:
            assert k * w + d in have or k * w + d >= rg.frames
    assert set(range(sc.EDGE)) <= have and set(range(rg.frames - sc.EDGE, rg.frames)) <= have
    r = sc.r128_structured()
    have = set(int(q) for q in r.positions)
    h = sc.hop(r.rate)
    assert h == 800 and r.frames // h == 40
    for k in range(1, 41):
        for d in sc.R128_OFFSETS:
            assert k * h + d in have or k * h + d >= r.frames
    tp = sc.tp_structured(8000)
    assert len(tp) == 17 * 33 and {sc.tp_format_of(q) for q in tp.positions} == set(sc.FORMATS)
    assert [sc.tp_format_of(1024 * k - 16) for k in (1, 2, 3)] == [sc.tp_format_of(1024 * k + 16) for k in (1, 2, 3)]


def test_windows_and_peaks_of_marker_tracks_on_the_oracle(oracle):
    """The window count the GPU sweep expects (every window counted, the partial last one too) and the expected peak are
    what the ReplayGain 1.0 oracle gives, background and marker tracks alike, in every format."""
    for rate in sc.RG1_RATES:
        for nch in (2, 1):
            sw = sc.rg1_exhaustive(rate, nch)
            want_windows = sc.windows_of(rate, sw.frames)
            assert want_windows == 3
            for fmt in sc.FORMATS:
                bg = [sc.as_format(c, fmt) for c in sw.background]
                res, hist = oracle.analyze_pcm(bg[0], bg[1] if nch == 2 else None, rate)
                assert int(hist.sum()) == want_windows and res["peak"] <= sc.BACKGROUND_MAX / 32768.0
                tracks, m = sw.tracks(fmt, rot=3)
                for i in range(0, len(sw), 7):
                    res, hist = oracle.analyze_pcm(tracks[i][0], tracks[i][1] if nch == 2 else None, rate)
                    assert int(hist.sum()) == want_windows and res["peak"] == sc.expected_peaks(m)[i], (sw.name, fmt, i)
    sw = sc.rg1_structured(1)
    bg = sc.as_format(sw.background[0], "f32")
    assert int(oracle.analyze_pcm(bg, None, sw.rate)[1].sum()) == sc.windows_of(sw.rate, sw.frames) == 78


# ---- true peak ----------------------------------------------------------------------------------------------------------------
TP_SWEEPS = [sc.tp_structured(rate) for rate in sc.TP_RATES]


@pytest.mark.parametrize("sw", TP_SWEEPS, ids=[s.name for s in TP_SWEEPS])
def test_true_peak_cases_stand_clear_of_their_background(sw):
    background = r128ref.true_peak([sc.unit(c) for c in sw.background], sw.rate)
    print(f"{sw.name}: background true peak {background:.4f}")
    assert background <= 0.02
    refs = sw.true_peak_refs()
    assert len(refs) == len(sw) == 561 and float(refs.min()) >= 0.5
    m = sc.expected_peaks(sc.markers(len(sw)))
    single = np.array([p % 2 == 0 for p in sw.positions])
    # a single marker peaks in itself (the centre tap is 1, the rest of its phase 0), a doublet between its two samples
    assert np.all(np.abs(refs[single] / m[single] - 1.0) < 0.02)
    assert np.all(refs[~single] / m[~single] > 1.2) and np.all(refs[~single] / m[~single] < 1.3)
    print(f"{sw.name}: doublets peak at {float(np.min(refs[~single] / m[~single])):.4f} .. {float(np.max(refs[~single] / m[~single])):.4f} x the marker")


@pytest.mark.parametrize("sw", TP_SWEEPS, ids=[s.name for s in TP_SWEEPS])
def test_the_tolerance_cannot_hide_a_lost_frame_of_outputs(sw):
    """The F interpolator outputs of one frame, zeroed: for the frame that holds the peak (24 / F frames after the marker, a
    doublet's lies between its two samples) the reference moves by more than 100 x TP_TOL in every case.  That frame's history
    reaches back 48 / F frames, across the tile boundary for the positions of this list: a tile that lost its history would lose as much."""
    F = r128ref.tp_factor(sw.rate)
    h = r128ref.tp_taps(F)
    refs = sw.true_peak_refs()
    background = r128ref.true_peak([sc.unit(c) for c in sw.background], sw.rate)
    span = 48 // F + 4
    crossing = 0
    for i, p in enumerate(int(q) for q in sw.positions):
        x = sc.unit(sw.marked(i)[0])
        lo, hi = max(p - span, 0), min(p + span, sw.frames)
        u = np.zeros((hi - lo) * F)
        u[::F] = x[lo:hi]
        y = np.abs(np.convolve(u, h))  # outputs lo * F ...: those within 48 of either cut are not the track's
        at = int(np.argmax(y))
        assert 48 <= at < len(y) - 48 and y[at] == pytest.approx(refs[i], rel=1e-12), (sw.name, p)
        frame = lo + at // F
        assert frame - p in (24 // F, 24 // F + 1)
        crossing += (frame // sc.TP_TILE) != ((frame - 48 // F) // sc.TP_TILE)
        y[(at // F) * F:(at // F + 1) * F] = 0.0
        left = max(float(y[48:len(y) - 48].max()), background)
        assert (refs[i] - left) / refs[i] > 100.0 * TP_TOL, (sw.name, p, refs[i], left)
    assert crossing >= 17 * (48 // F)  # at every tile boundary, every depth of history


def test_exhaustive_r128_cases_have_their_own_references():
    """One reference per track, none left out; singles at even positions, doublets at odd ones."""
    sw = sc.r128_exhaustive()
    refs = sw.true_peak_refs()
    assert len(refs) == len(sw) == sw.frames and np.all(refs >= 0.5)
    m = sc.expected_peaks(sc.markers(len(sw)))
    even = sw.positions % 2 == 0
    assert np.all(np.abs(refs[even] / m[even] - 1.0) < 0.02)
    odd = ~even
    assert np.all(refs[odd] / m[odd] > 1.2)
    assert all(r128ref.true_peak([sc.unit(c) for c in sw.marked(i)], sw.rate) == refs[i] for i in (0, 1001, 2000, 3244))


def test_nan_references_drop_what_the_nan_touches():
    sp, tp = sc.r128_nonfinite_refs()
    assert len(sp) == len(tp) == sc.r128_exhaustive().frames
    assert np.all(np.isfinite(sp)) and np.all(np.isfinite(tp)) and np.all(sp > 0) and np.all(tp >= sp)
    assert float(tp.max()) <= 0.02
    assert len(np.unique(tp)) > 1  # the dropped outputs matter: where the background's own peak is touched, it is gone
