"""The host side of the spectral scan (include/mp3rgain_amd_spectrum.h): the serial twin in double (route 0) against the float64
numpy restatement of tests/spectrum_cases.py, the kernels' f32 arithmetic on the host (route 2) against the same restatement
within the measured tolerance (tests/golden/spectrum_measured.json, tools/spectrum_refcheck.py), the verdict function on
constructed band levels with ==, and the argument errors.  No GPU."""
import math
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import arena_layouts as al  # noqa: E402
import spectrum_cases as sc  # noqa: E402

import mp3rgain_amd as rg  # noqa: E402
from mp3rgain_amd import _capi  # noqa: E402

RG_ERR_INVALID_ARG, RG_ERR_FORMAT = -1, -9
BL, UP = _capi.SPEC_BANDLIMITED, _capi.SPEC_UPSAMPLED


@pytest.fixture(scope="module")
def routes(capi):
    tracks = sc.tracks()
    arena, descs, guards = al.pack(tracks, al.Layout("guard", "loud", "input", 3))
    descs = list(descs)[:len(tracks)]
    return tracks, {route: rg.spectrum_arena(None, route, descs, arena) for route in (0, 2)}, (arena, descs, guards)


def test_kernel_shape(capi):
    frame, hop, bands, t = rg.spectrum_kernel_shape()
    assert (frame, hop, bands) == (sc.L, sc.H, sc.BANDS) and t >= 2 and t % 2 == 0
    assert (_capi.load().rg_spectrum_kernel_shape(None, None, None, None)) == 0
    import ctypes as C
    assert C.sizeof(_capi.SpectrumChannel) == 32 and C.sizeof(_capi.SpectrumRecord) == 296


def test_cases_cover_what_they_should(capi):
    t = sc.shape()[3]
    tracks = sc.tracks()
    ks = {sc.frames_of(len(tr.channels[0])) for tr in tracks}
    assert {0, 1, 2, 3, t - 1, t, t + 1, 2 * t + 1} <= ks
    assert {len(tr.channels) for tr in tracks} >= {1, 2, 6}
    assert {tr.sample_rate for tr in tracks} >= {8000, 44100, 48000, 96000}
    assert {tr.channels[0].dtype for tr in tracks} == {np.dtype(np.int16), np.dtype(np.int32), np.dtype(np.float32)}
    assert max(len(tr.channels[0]) for tr in tracks) <= (2 * t + 2) * sc.H + 1
    # the 24-bit cases really are 24-bit samples in 32-bit containers
    assert all(not (tr.channels[0] & 0xFF).any() for tr in tracks if tr.channels[0].dtype == np.int32)


@pytest.mark.parametrize("route", (0, 2))
def test_host_routes_against_the_restatement(routes, route):
    """E[j] of every case within the float64 tolerance (route 0) or 8 times the recorded f32 error (route 2), the frame counts,
    the verdict arithmetic with == on the route's own energies, and on the verdict cases the restatement's cutoff and flags."""
    tracks, got, _ = routes
    recs, e = got[route]
    wants = sc.wants()
    of_total, relative = (sc.F64_TOLERANCE, 1e-9) if route == 0 else tuple(sc.TOLERANCE_FACTOR * x for x in sc.measured())
    for i, tr in enumerate(tracks):
        r = recs[i]
        assert (r.status, r.frames, r.sample_rate, r.channels, r.format, r.dropped_frames) == \
            (0, len(tr.channels[0]), tr.sample_rate, len(tr.channels), al.FMT[tr.channels[0].dtype], 0), tr.name
        for c, (ref, analysed, skipped) in enumerate(wants[tr.name]):
            ch = r.ch[c]
            assert (ch.analysed_frames, ch.skipped_frames) == (analysed, skipped), tr.name
            a, b = sc.errors(e[i, c], ref)
            assert a <= of_total and b <= relative, (tr.name, c, a, b)
            assert (ch.cutoff_hz, ch.edge_db, ch.flags) == sc.verdict_of_energy(e[i, c], analysed, tr.sample_rate), tr.name
            if tr.name.startswith("verdict-"):
                cutoff, edge, flags = sc.verdict_of_energy(ref, analysed, tr.sample_rate)
                assert (ch.cutoff_hz, ch.flags) == (cutoff, flags), tr.name
                if route == 0:
                    assert abs(ch.edge_db - edge) < 1e-6, tr.name
        assert not e[i, len(tr.channels):].any(), tr.name
        assert r.flags == sc.want_track_flags(tr, [x.flags for x in r.ch[:r.channels]], [w[2] for w in wants[tr.name]]), tr.name
        assert r.cutoff_hz == max(x.cutoff_hz for x in r.ch[:r.channels]), tr.name


def test_verdict_cases_read_as_designed(routes):
    """What the signals were built to show: a brick wall at 16 kHz reads within two bands of 16.2 kHz, noise reads no cutoff, the
    96 kHz file made from 44.1 kHz material reads as upsampled -- in double and in the kernels' f32 alike."""
    tracks, got, _ = routes
    by_name = {tr.name: i for i, tr in enumerate(tracks)}
    for route in (0, 2):
        recs, _ = got[route]
        for name, rate, fmt, slope, cut, transition, level, bandlimited, upsampled in sc.VERDICT_SIGNALS:
            ch = recs[by_name[f"verdict-{name}"]].ch[0]
            assert bool(ch.flags & BL) == bandlimited and bool(ch.flags & UP) == upsampled, (route, name, ch.cutoff_hz, ch.edge_db)
            if not bandlimited:
                assert (ch.cutoff_hz, ch.edge_db) == (rate / 2.0, 0.0), name
            else:
                assert ch.edge_db >= 30.0 and cut <= ch.cutoff_hz <= cut + transition / 2 + 6 * 8 * rate / sc.L, (name, ch.cutoff_hz)
        for name in ("white-16k", "pink-16k"):
            assert abs(recs[by_name[f"verdict-{name}"]].ch[0].cutoff_hz - 16200.0) <= 172.3, name
        sine = recs[by_name["verdict-sine-1k"]].ch[0]
        assert (sine.cutoff_hz, sine.flags) == (22050.0, 0)
        assert recs[by_name["verdict-pink-up96k"]].flags & UP and 21900.0 <= recs[by_name["verdict-pink-up96k"]].cutoff_hz <= 22800.0


def test_nonfinite_frames_are_skipped_alone(routes):
    tracks, got, _ = routes
    by_name = {tr.name: i for i, tr in enumerate(tracks)}
    t = sc.shape()[3]
    for route in (0, 2):
        recs, e = got[route]
        for name, skipped in (("nan-first", 1), ("nan-overlap", 2), ("nan-tail", 0), ("inf-mid", 2), ("neginf-last-frame", 1)):
            r = recs[by_name[name]]
            assert (r.ch[0].analysed_frames, r.ch[0].skipped_frames, r.ch[1].skipped_frames) == (5 - skipped, skipped, 0), (route, name)
            assert bool(r.flags & _capi.SPEC_NONFINITE) == (skipped > 0) and np.isfinite(e[by_name[name]]).all()
        r = recs[by_name["nan-across-tiles"]]
        assert (r.ch[0].analysed_frames, r.ch[0].skipped_frames) == (2 * t + 1 - 2, 2)
        r = recs[by_name["nan-everywhere"]]
        assert (r.ch[0].analysed_frames, r.ch[0].skipped_frames, r.ch[0].cutoff_hz, r.ch[0].flags) == (0, 5, 0.0, 0)
        assert not e[by_name["nan-everywhere"]].any()
        r = recs[by_name["silence"]]
        assert (r.ch[0].analysed_frames, r.ch[0].cutoff_hz, r.ch[0].edge_db, r.ch[0].flags) == (2, 0.0, 0.0, 0)


def test_guards_reach_no_record(routes):
    tracks, got, (arena, descs, guards) = routes
    assert guards
    other = arena.copy()
    for a, b in guards:
        other[a:b] ^= 0x5A
    for route in (0, 2):
        recs, e = rg.spectrum_arena(None, route, descs, other)
        assert b"".join(bytes(r) for r in recs) == b"".join(bytes(r) for r in got[route][0]) and e.tobytes() == got[route][1].tobytes()


# ---- the verdict on constructed band levels ------------------------------------------------------------------------------------
def _step(j, ratio, hi=1.0):
    """Level `hi` up to and including band j, hi / ratio above."""
    p = np.full(sc.BANDS, hi / ratio)
    p[:j + 1] = hi
    return p


def _verdict(p, fs=44100, frames=10, **kw):
    c = rg.spectrum_verdict(p, frames, fs, kw.get("edge_db"), kw.get("min_cutoff_hz"))
    want = sc.verdict(p, frames, fs, kw.get("edge_db") or 30.0, kw.get("min_cutoff_hz") or 4000.0)
    assert (c.cutoff_hz, c.edge_db, c.flags) == want
    assert (c.analysed_frames, c.skipped_frames) == (frames, 0)
    return c.cutoff_hz, c.edge_db, c.flags


def test_verdict_step_at_under_and_over_the_threshold(capi):
    f = lambda j: (8.0 * j + 8.5) * 44100 / sc.L  # noqa: E731
    assert 10.0 * math.log10(1000.0) == 30.0  # the step of 1000 sits exactly on the default threshold
    assert _verdict(_step(100, 1000.0)) == (f(100), 30.0, BL)
    assert _verdict(_step(100, 999.0)) == (22050.0, 0.0, 0)
    cutoff, edge, flags = _verdict(_step(100, 1001.0))
    assert (cutoff, flags) == (f(100), BL) and 30.0 < edge < 30.01
    # the same step under other options
    assert _verdict(_step(100, 999.0), edge_db=29.0)[2] == BL
    assert _verdict(_step(100, 1001.0), edge_db=31.0)[2] == 0
    # a deep step reads its depth, and only the bands at the step qualify best
    cutoff, edge, flags = _verdict(_step(150, 1e8))
    assert (cutoff, flags) == (f(150), BL) and abs(edge - 80.0) < 1e-9
    # the floor: nothing at all above the step reads 120 dB
    p = _step(150, 1.0)
    p[151:] = 0.0
    cutoff, edge, flags = _verdict(p)
    assert (cutoff, flags) == (f(150), BL) and abs(edge - 120.0) < 1e-9


def test_verdict_energy_coming_back_above_the_edge(capi):
    p = _step(100, 1e6)
    assert _verdict(p)[2] == BL
    p[200:] = 1.0  # as loud as the pass band again: the step at 100 is no cutoff, and nothing falls after band 200
    assert _verdict(p) == (22050.0, 0.0, 0)
    p[200:] = 1e-3 * (1.0 - 1e-9)  # just under the pass band less 30 dB: allowed, and the edge keeps its 60 dB
    cutoff, edge, flags = _verdict(p)
    assert (cutoff, flags) == ((8.0 * 100 + 8.5) * 44100 / sc.L, BL) and abs(edge - 60.0) < 1e-9
    p[200:] = 1e-3 * (1.0 + 1e-9)
    assert _verdict(p)[2] == 0
    p = _step(100, 1e6)
    p[255] = 1.0  # the very last band counts too
    assert _verdict(p)[2] == 0
    p[255] = 1e-4
    assert _verdict(p)[2] == BL


def test_verdict_tie_takes_the_lowest_band(capi):
    # two identical steps of 40 dB, far enough apart that their windows do not meet
    p = np.ones(sc.BANDS)
    p[61:] = 1e-4
    p[121:] = 1e-8
    cutoff, edge, flags = _verdict(p)
    assert (cutoff, flags) == ((8.0 * 60 + 8.5) * 44100 / sc.L, BL) and abs(edge - 40.0) < 1e-9
    d = [10.0 * math.log10((sum(p[j - 7:j + 1]) / 8) / (sum(p[j + 1:j + 9]) / 8)) for j in (60, 120)]
    assert d[0] == d[1]  # a tie in the arithmetic itself


def test_verdict_min_cutoff(capi):
    f = lambda j, fs: (8.0 * j + 8.5) * fs / sc.L  # noqa: E731
    p = _step(20, 1e6)
    assert f(20, 44100) < 4000.0 < f(50, 44100)
    assert _verdict(p)[2] == 0                       # an edge below min_cutoff_hz is no finding
    assert _verdict(p, min_cutoff_hz=1000.0)[2] == BL
    assert _verdict(p, min_cutoff_hz=f(20, 44100)) == (f(20, 44100), 10.0 * math.log10(1e6), BL)  # exactly at the band's upper edge
    # rate 8000: every candidate's upper edge lies below 4000 Hz, so the default finds nothing
    assert f(247, 8000) < 4000.0
    assert _verdict(_step(100, 1e6), fs=8000) == (4000.0, 0.0, 0)
    assert _verdict(_step(100, 1e6), fs=8000, min_cutoff_hz=4000.0) == (4000.0, 0.0, 0)   # at Nyquist
    assert _verdict(_step(100, 1e6), fs=8000, min_cutoff_hz=5000.0) == (4000.0, 0.0, 0)   # above Nyquist
    assert _verdict(_step(100, 1e6), fs=8000, min_cutoff_hz=1000.0)[2] == BL
    # upsampled: a high rate and an edge at or below 24.5 kHz
    cutoff, edge, flags = _verdict(_step(120, 1e6), fs=96000)
    assert (cutoff, flags) == (f(120, 96000), BL | UP) and abs(edge - 60.0) < 1e-9
    assert f(120, 96000) <= 24500.0 < f(140, 96000)
    assert _verdict(_step(140, 1e6), fs=96000)[2] == BL
    assert _verdict(_step(120, 1e6), fs=48000)[2] == BL


def test_verdict_without_input(capi):
    assert _verdict(np.zeros(sc.BANDS)) == (0.0, 0.0, 0)
    assert _verdict(_step(100, 1e6), frames=0) == (0.0, 0.0, 0)
    assert _verdict(np.ones(sc.BANDS)) == (22050.0, 0.0, 0)
    L = _capi.load()
    out = _capi.SpectrumChannel()
    import ctypes as C
    p = (C.c_double * 256)()
    assert L.rg_spectrum_verdict(None, 1, 44100, None, C.byref(out)) == RG_ERR_INVALID_ARG
    assert L.rg_spectrum_verdict(p, 1, 44100, None, None) == RG_ERR_INVALID_ARG
    assert L.rg_spectrum_verdict(p, 1, 0, None, C.byref(out)) == RG_ERR_INVALID_ARG
    assert L.rg_spectrum_verdict(p, 1, 44100, C.byref(_capi.SpectrumOpts(0.0, 4000.0)), C.byref(out)) == RG_ERR_INVALID_ARG
    assert L.rg_spectrum_verdict(p, 1, 44100, C.byref(_capi.SpectrumOpts(30.0, -1.0)), C.byref(out)) == RG_ERR_INVALID_ARG


def test_argument_errors(capi):
    L = _capi.load()
    arena = np.zeros(64, dtype=np.uint8)
    out = (_capi.SpectrumRecord * 1)()
    d = (_capi.TrackDesc * 1)(_capi.TrackDesc(0, 16, 44100, 2, _capi.FMT_S16_PLANAR))
    S16, S32, F32 = _capi.FMT_S16_PLANAR, _capi.FMT_S32_PLANAR, _capi.FMT_F32_PLANAR
    for route in (0, 2):
        assert L.rg_spectrum_arena(None, route, 1, d, None, arena.ctypes.data, 64, out, None) == 0
        assert L.rg_spectrum_arena(None, route, 1, None, None, arena.ctypes.data, 64, out, None) == RG_ERR_INVALID_ARG
        assert L.rg_spectrum_arena(None, route, 1, d, None, arena.ctypes.data, 64, None, None) == RG_ERR_INVALID_ARG
        assert L.rg_spectrum_arena(None, route, 1, d, None, None, 64, out, None) == RG_ERR_INVALID_ARG
        assert L.rg_spectrum_arena(None, route, 0, None, None, None, 0, None, None) == 0
        for desc, code, text in ((_capi.TrackDesc(0, 17, 44100, 2, S16), RG_ERR_INVALID_ARG, "beyond the arena"),
                                 (_capi.TrackDesc(2, 16, 44100, 2, S16), RG_ERR_INVALID_ARG, "beyond the arena"),
                                 (_capi.TrackDesc(66, 0, 44100, 1, S16), RG_ERR_INVALID_ARG, "beyond the arena"),
                                 (_capi.TrackDesc(0, 9, 44100, 2, F32), RG_ERR_INVALID_ARG, "beyond the arena"),
                                 (_capi.TrackDesc(1, 4, 44100, 2, S16), RG_ERR_INVALID_ARG, "sample-aligned"),
                                 (_capi.TrackDesc(2, 4, 44100, 2, S32), RG_ERR_INVALID_ARG, "sample-aligned"),
                                 (_capi.TrackDesc(6, 4, 44100, 2, F32), RG_ERR_INVALID_ARG, "sample-aligned"),
                                 (_capi.TrackDesc(0, 1, 44100, 9, S16), RG_ERR_FORMAT, "9 channel"),
                                 (_capi.TrackDesc(0, 1, 44100, 0, S16), RG_ERR_FORMAT, "0 channel"),
                                 (_capi.TrackDesc(0, 1, 44100, 2, 3), RG_ERR_FORMAT, "format 3"),
                                 (_capi.TrackDesc(0, 1 << 32, 44100, 2, S16), RG_ERR_FORMAT, "2^32")):
            with pytest.raises(rg.ReplayGainError) as e:
                rg.spectrum_arena(None, route, [desc], arena)
            assert e.value.code == code and text in str(e.value), (desc.frames, desc.channels, str(e.value))
        for opts in ((0.0, 4000.0), (30.0, 0.0), (-3.0, None), (float("nan"), 4000.0)):
            with pytest.raises(rg.ReplayGainError) as e:
                rg.spectrum_arena(None, route, list(d), arena, *opts)
            assert e.value.code == RG_ERR_INVALID_ARG and "greater than 0" in str(e.value)
    assert L.rg_spectrum_arena(None, 1, 1, d, None, arena.ctypes.data, 64, out, None) == RG_ERR_INVALID_ARG  # the kernels need a context
    assert L.rg_spectrum_arena(None, 3, 1, d, None, arena.ctypes.data, 64, out, None) == RG_ERR_INVALID_ARG
    # a track may end at the arena's last byte, and 8 channels are taken: too short for a frame
    recs, e = rg.spectrum_arena(None, 0, [_capi.TrackDesc(0, 4, 44100, 8, S16)], arena)
    assert (recs[0].channels, recs[0].flags, recs[0].cutoff_hz) == (8, _capi.SPEC_SHORT | _capi.SPEC_COMPLETE, 0.0) and not e.any()
