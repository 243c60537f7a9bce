"""Stage 1 of the tempo scan on the CPU (include/mp3rgain_amd_tempo.h): the serial host twin (rg_tempo_arena route 0) and the
kernels' arithmetic on the host (route 2) against the float64 numpy restatement of tests/tempo_cases.py, within the bounds
tools/tempo_refcheck.py recorded (tests/golden/tempo_measured.json, times TOLERANCE_FACTOR); the band table against the
formula; the records of the short, rate, silent, clipped and non-finite cases; descriptor and option errors.  No GPU."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import tempo_cases as tc  # noqa: E402

import mp3rgain_amd as rg  # noqa: E402
from mp3rgain_amd import _capi  # noqa: E402

RG_ERR_INVALID_ARG, RG_ERR_FORMAT = -1, -9


@pytest.fixture(scope="module")
def routes():
    cs = tc.cases()
    arena, descs = tc.pack(cs)
    return cs, {r: rg.tempo_arena(None, r, descs, arena) for r in (0, 2)}, [tc.reference(c) for c in cs]


def _slices(recs, onsets, bands):
    at = 0
    for r in recs:
        yield onsets[r.onsets_at:r.onsets_at + r.onsets], bands[at:at + r.band_frames].astype(np.float64)
        at += r.band_frames


@pytest.mark.parametrize("route", (0, 2))
def test_band_energies_within_the_recorded_bound(routes, route):
    cs, got, refs = routes
    recs, onsets, bands = got[route]
    bound = tc.TOLERANCE_FACTOR * tc.measured()[f"band_error_route{route}"]
    assert 0 < bound < 1e-5  # f32 band sums: a few units of 2^-24 of the frame's largest band
    for c, r, ref, (_, E) in zip(cs, recs, refs, _slices(recs, onsets, bands)):
        assert (r.band_frames, r.onsets, r.nonfinite_frames) == (ref.frames, len(ref.onsets), ref.nonfinite), c.name
        assert tc.band_error(E, ref.bands) <= bound, c.name


@pytest.mark.parametrize("route", (0, 2))
def test_onsets_differ_from_the_reference_in_no_more_than_the_recorded_share(routes, route):
    cs, got, refs = routes
    recs, onsets, bands = got[route]
    m = tc.measured()
    differ = total = 0
    for c, r, ref, (o, _) in zip(cs, recs, refs, _slices(recs, onsets, bands)):
        d = np.abs(o.astype(np.int64) - ref.onsets.astype(np.int64))
        assert d.max(initial=0) <= max(1, m["largest_onset_difference"]), c.name  # a band energy next to a step of q: a quarter of a step
        differ, total = differ + int((d != 0).sum()), total + len(d)
    assert total > 400 and differ <= tc.TOLERANCE_FACTOR * m[f"differing_share_route{route}"] * total, (differ, total)


def test_the_band_table_is_the_formula():
    for rate in (8000, 11025, 15996, 15997, 16000, 22050, 32000, 44100, 48000, 88200, 96000, 192000, 384000):
        want, ok = tc.bands_of(rate)
        got, supported = rg.tempo_bands(rate)
        assert got == want and supported == ok, rate
        assert all(b > a for a, b in zip(got, got[1:])) and got[0] >= 1
    # e[32] = floor(32768000 / fs + 0.5) <= 2048 from 15997 Hz up
    assert [rg.tempo_bands(rate)[1] for rate in (8000, 15996, 15997, 44100, 48000, 96000, 192000)] == [False, False, True, True, True, True, True]
    e = rg.tempo_bands(44100)[0]
    assert (e[0], e[32]) == (6, 743)
    e = rg.tempo_bands(192000)[0]
    assert e[:5] == [1, 2, 3, 4, 5] and e[32] == 171  # the low edges collide and are pushed apart
    for rate in range(16000, 200000, 977):
        assert rg.tempo_bands(rate)[1] and tc.bands_of(rate)[1], rate
    with pytest.raises(rg.ReplayGainError):
        rg.tempo_bands(0)


def test_records_of_the_short_rate_silent_and_nonfinite_cases(routes):
    cs, got, refs = routes
    by = {c.name: k for k, c in enumerate(cs)}
    T = tc.tile_onsets()
    C, S, R, N, G = _capi.TEMPO_COMPLETE, _capi.TEMPO_SHORT, _capi.TEMPO_RATE, _capi.TEMPO_NONFINITE, _capi.TEMPO_RANGE
    for route in (0, 2):
        recs, onsets, bands = got[route]
        each = list(_slices(recs, onsets, bands))
        for k, r in enumerate(recs):
            assert (r.status, r.dropped_frames, r.frames, r.period16, r.bpm_milli) == (0, 0, len(cs[k].channels[0]), 0, 0), cs[k].name
            assert (r.channels, r.sample_rate, r.windows) == (len(cs[k].channels), cs[k].sample_rate, 0)
        for fmt in ("s16", "s32", "f32"):
            for name, frames, k in (("n4095", 0, 0), ("n4096", 1, 0), ("n4607", 1, 0), ("n4608", 2, 1)):
                r = recs[by[f"{name}_{fmt}_1ch"]]
                assert (r.flags, r.band_frames, r.onsets, r.harmonics) == (C | S, frames, k, 8), (name, fmt)
            r = recs[by[f"n4608_{fmt}_3ch"]]
            assert (r.flags, r.band_frames, r.onsets, r.channels) == (C | S, 2, 1, 3)
            assert recs[by[f"k{T}_{fmt}_1ch"]].onsets == T and recs[by[f"k{T + 1}_{fmt}_2ch"]].onsets == T + 1 and recs[by[f"k{2 * T - 1}_{fmt}_1ch"]].onsets == 2 * T - 1
        r = recs[by["rate8000_s16_1ch"]]
        assert (r.flags, r.band_frames, r.onsets, r.sample_rate, r.harmonics) == (C | S | R, 0, 0, 8000, 0)
        for rate, kh in ((44100, 8), (48000, 8), (96000, 7), (192000, 3)):  # pmax = 1033, 1125, 2250, 4500
            r = recs[by[f"rate{rate}_s16_1ch"]]
            assert (r.flags, r.onsets, r.harmonics) == (C | S, 3, kh), rate
        k = by["nonfinite_f32_2ch"]
        r = recs[k]
        assert (r.flags, r.onsets, r.nonfinite_frames) == (C | S | N, 2 * T + 2, 9)  # frames 4 .. 11 (the NaN) and the last (the Inf)
        E = each[k][1]
        assert not E[4:12].any() and not E[-1].any() and E[:4].all() and E[12:-1].all()
        for fmt in ("s16", "f32"):
            o, E = each[by[f"silence_{fmt}_1ch"]]
            assert len(o) == T + 3 and not o.any() and not E.any()  # digital silence: every onset 0
            o, _ = each[by[f"silence_then_noise_{fmt}_2ch"]]
            assert o.max() == 1023 and not o[:3].any() and (o == 1023).sum() >= 1  # silence, then full scale: the clip
        assert not G & recs[by["music_2s_s16_2ch"]].flags
    # the third channel does not count: the onsets of the 3-channel case are those of its first two channels alone
    k = by["n4608_s16_3ch"]
    two = tc.Case("two", cs[k].channels[:2], 44100)
    arena, descs = tc.pack([two])
    r = got[2][0][k]
    assert rg.tempo_arena(None, 2, descs, arena)[1].tobytes() == got[2][1][r.onsets_at:r.onsets_at + r.onsets].tobytes()


def test_routes_agree_on_the_records_and_stage_2_runs_behind_stage_1(routes):
    cs, got, _ = routes
    for a, b in zip(got[0][0], got[2][0]):
        assert bytes(a) == bytes(b)
    # with a window short enough for the 2 s case, the record is the restatement's on the route's own onsets
    k = next(k for k, c in enumerate(cs) if c.name == "music_2s_s16_2ch")
    arena, descs = tc.pack([cs[k]])
    opts = dict(window=32, hop=8, min_bpm=300)
    for route in (0, 2):
        recs, onsets, _ = rg.tempo_arena(None, route, descs, arena, **opts)
        want, _ = tc.ref_stage2(onsets, 44100, **opts)
        assert tc.record_fields(recs[0]) == want and recs[0].period16 and recs[0].windows == (164 - 64) // 8 + 1


def test_descriptor_and_option_errors():
    arena = np.zeros(64, dtype=np.uint8)
    S16 = _capi.FMT_S16_PLANAR
    for desc, code, text in ((_capi.TrackDesc(0, 17, 44100, 2, S16), RG_ERR_INVALID_ARG, "beyond the arena"),
                             (_capi.TrackDesc(1, 4, 44100, 2, S16), RG_ERR_INVALID_ARG, "sample-aligned"),
                             (_capi.TrackDesc(0, 1, 44100, 9, S16), RG_ERR_FORMAT, "9 channel"),
                             (_capi.TrackDesc(0, 1, 44100, 0, S16), RG_ERR_FORMAT, "0 channel"),
                             (_capi.TrackDesc(0, 1, 44100, 1, 7), RG_ERR_FORMAT, "not a planar PCM format")):
        for route in (0, 2):
            with pytest.raises(rg.ReplayGainError) as e:
                rg.tempo_arena(None, route, [desc], arena)
            assert e.value.code == code and text in str(e.value)
    ok = _capi.TrackDesc(0, 4, 44100, 2, S16)
    with pytest.raises(rg.ReplayGainError) as e:
        rg.tempo_arena(None, 3, [ok], arena)
    assert e.value.code == RG_ERR_INVALID_ARG
    for bad in (dict(window=31), dict(window=1025), dict(window=64, hop=65), dict(min_bpm=29), dict(min_bpm=301)):
        for route in (0, 2):
            with pytest.raises(rg.ReplayGainError) as e:
                rg.tempo_arena(None, route, [ok], arena, **bad)
            assert e.value.code == RG_ERR_INVALID_ARG and "tempo: window" in str(e.value)
    r = rg.tempo_arena(None, 0, [_capi.TrackDesc(0, 4, 0, 8, S16)], arena)[0][0]  # no rate: not supported, no error
    assert (r.status, r.flags) == (0, _capi.TEMPO_COMPLETE | _capi.TEMPO_SHORT | _capi.TEMPO_RATE)
    assert rg.tempo_arena(None, 0, [], arena)[0] == []
    shape = rg.tempo_kernel_shape()
    assert shape[1] == 256 and shape[0] % 2 == 1 and shape[3] * shape[4] == _capi.TEMPO_MAX_WINDOW and shape[2] <= 80 * 1024
    assert _capi.TEMPO_BEAT_BIAS == tc.measured()["beat_bias"]  # the constant is the measured median
