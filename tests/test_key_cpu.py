"""Stage 1 of the key scan on the CPU (include/mp3rgain_amd_key.h): the serial host twin (rg_key_arena route 0) and the kernels'
arithmetic on the host (route 2) against the float64 numpy restatement of tests/key_cases.py, within the bounds
tools/key_refcheck.py recorded (tests/golden/key_measured.json, times TOLERANCE_FACTOR); the decimation factor, the band table
and the filter table against their formulas; the records of the short, rate, silent and non-finite cases; descriptor and option
errors.  No GPU."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import key_cases as kc  # noqa: E402

import mp3rgain_amd as rg  # noqa: E402
from mp3rgain_amd import _capi  # noqa: E402

RG_ERR_INVALID_ARG, RG_ERR_FORMAT = -1, -9


@pytest.fixture(scope="module")
def routes():
    cs = kc.cases()
    arena, descs = kc.pack(cs)
    return cs, {r: rg.key_arena(None, r, descs, arena) for r in (0, 2)}, [kc.reference(c) for c in cs]


def _slices(recs, y, bands, chroma):
    ya = 0
    for r in recs:
        yield y[ya:ya + r.decimated], bands[r.chroma_at:r.chroma_at + r.rows].astype(np.float64), chroma[r.chroma_at:r.chroma_at + r.rows]
        ya += r.decimated


@pytest.mark.parametrize("route", (0, 2))
def test_decimated_signal_and_band_energies_within_the_recorded_bounds(routes, route):
    cs, got, refs = routes
    recs = got[route][0]
    m = kc.measured()
    ybound, bbound = kc.TOLERANCE_FACTOR * m[f"y_error_route{route}"], kc.TOLERANCE_FACTOR * m[f"band_error_route{route}"]
    # an f32 sum of up to 609 products: some tens of units of 2^-24 of the largest |y|; f32 band sums as the tempo scan's
    assert 0 < ybound < 2e-5 and 0 < bbound < 1e-5
    for c, r, ref, (y, E, _) in zip(cs, recs, refs, _slices(*got[route])):
        want = (ref.decim if ref.supported else r.decim, len(ref.y), ref.frames, ref.nonfinite)
        assert (r.decim, r.decimated, r.rows, r.nonfinite_frames) == want, c.name
        assert kc.y_error(y, ref.y) <= ybound, c.name
        assert kc.band_error(E, ref.bands) <= bbound, c.name


@pytest.mark.parametrize("route", (0, 2))
def test_rows_differ_from_the_reference_in_no_more_than_the_recorded_share(routes, route):
    """A band energy within the band error of a step of q moves its entry by one; when it is the frame's largest band, every
    entry of that row moves, by up to five (five octaves, each by one step).  The tool met none on these cases; a libm with
    other roots for route 0's transform may meet one, so the bound is a row's twelve entries, times TOLERANCE_FACTOR."""
    cs, got, refs = routes
    m = kc.measured()
    differ = total = 0
    for c, r, ref, (_, _, rows) in zip(cs, got[route][0], refs, _slices(*got[route])):
        d = np.abs(rows.astype(np.int64) - ref.rows.astype(np.int64))
        assert d.max(initial=0) <= max(5, m["largest_entry_difference"]), c.name
        differ, total = differ + int((d != 0).sum()), total + d.size
    assert total == m[f"entries_route{route}"] and total > 2000
    assert differ <= kc.TOLERANCE_FACTOR * max(12, m[f"differing_entries_route{route}"]), (differ, total)


def test_the_factor_the_band_table_and_the_filter_are_their_formulas():
    assert [rg.key_bands(r)[0] for r in (44100, 48000, 96000, 192000, 8000, 5000, 4999, 384000, 404999, 405000)] == [8, 9, 19, 38, 1, 1, 0, 76, 80, 81]
    for rate in (5000, 8000, 9999, 11025, 22050, 32000, 44100, 48000, 88200, 96000, 176400, 192000, 384000, 404999):
        D, want, ok = kc.bands_of(rate)
        gd, got, supported = rg.key_bands(rate)
        assert (gd, got, supported) == (D, want, ok) and ok, rate
        assert all(b > a for a, b in zip(got, got[1:])) and got[0] >= 1 and got[60] <= 2048
        assert 5000 <= rate / D < 10000
    for rate in (1, 4000, 4999, 405000, 768000):
        assert rg.key_bands(rate)[1:] == (None, False)
    with pytest.raises(rg.ReplayGainError):
        rg.key_bands(0)
    e = rg.key_bands(44100)[1]
    assert (e[0], e[60]) == (47, 1511)  # 63.5 Hz and 2033 Hz at 5512.5 Hz
    for D in (2, 8, 9, 19, 38, 80):
        h = rg.key_filter(D)
        want = kc.filter_of(D)
        assert len(h) == 16 * D + 1 and abs(float(h.astype(np.float64).sum()) - 1.0) < 1e-6
        assert np.abs(h.astype(np.float64) - want.astype(np.float64)).max() <= 2.0 ** -24 * float(want.max()) * 4  # libm's sin and cos, then one rounding
        assert np.array_equal(h, h[::-1]) or np.abs(h - h[::-1]).max() < 1e-9
    for D in (0, 1, 81):
        with pytest.raises(rg.ReplayGainError):
            rg.key_filter(D)


def test_records_of_the_short_rate_silent_and_nonfinite_cases(routes):
    cs, got, refs = routes
    by = {c.name: k for k, c in enumerate(cs)}
    W, lanes, T, tile_lanes, lds = kc.shape()
    C, S, R, N, NONE = _capi.KEY_COMPLETE, _capi.KEY_SHORT, _capi.KEY_RATE, _capi.KEY_NONFINITE, _capi.KEY_NONE
    for route in (0, 2):
        recs = got[route][0]
        each = list(_slices(*got[route]))
        for k, r in enumerate(recs):
            assert (r.status, r.dropped_frames, r.frames, r.channels, r.sample_rate) == (0, 0, len(cs[k].channels[0]), len(cs[k].channels), cs[k].sample_rate), cs[k].name
        for fmt in ("s16", "s32", "f32"):
            for name, m, f, flags in (("n16D_%s_1ch", 0, 0, C | S), ("m1_%s_2ch", 1, 0, C | S), ("m4095_%s_1ch", 4095, 0, C | S), ("m4096_%s_1ch", 4096, 1, C),
                                      ("m4096_%s_3ch", 4096, 1, C), (f"f{T + 1}_%s_1ch", 4096 + T * 512, T + 1, C), (f"f{T + 2}_%s_2ch", 4096 + (T + 1) * 512 + 100, T + 2, C),
                                      (f"f{2 * T}_%s_1ch", 4096 + (2 * T - 1) * 512, 2 * T, C), (f"m{2 * W}_%s_2ch", 2 * W, 0, C | S), (f"m{2 * W + 1}_%s_1ch", 2 * W + 1, 0, C | S)):
                r = recs[by[name % fmt]]
                assert (r.decim, r.decimated, r.rows, r.flags & ~NONE) == (8, m, f, flags), (name, fmt)
        for name in ("rate4000_s16_1ch", "rate410000_f32_2ch"):
            r = recs[by[name]]
            assert (r.flags, r.decim, r.decimated, r.rows) == (C | S | R, 0, 0, 0)
        for name, D in (("rate8000_s16_2ch", 1), ("rate8000_f32_1ch", 1), ("rate48000_s32_2ch", 9), ("rate48000_s16_1ch", 9), ("rate192000_s16_1ch", 38), ("rate192000_f32_2ch", 38)):
            r = recs[by[name]]
            assert (r.decim, r.decimated, r.rows, r.flags & ~NONE) == (D, 4096 + 2 * 512 + 3, 3, C), name
        r = recs[by["rate8000_m255_s16_1ch"]]
        assert (r.decim, r.decimated, r.rows) == (1, 255, 0)
        k = by["nonfinite_f32_2ch"]
        r, (y, E, rows) = recs[k], each[k]
        assert r.flags & N and r.nonfinite_frames == refs[k].nonfinite and 0 < r.nonfinite_frames < r.rows
        bad = ~np.isfinite(np.lib.stride_tricks.sliding_window_view(y, 4096)[::512][:r.rows]).all(axis=1)
        assert int(bad.sum()) == r.nonfinite_frames and not E[bad].any() and not rows[bad].any() and rows[~bad].any(axis=1).all()
        assert r.silent_rows == r.nonfinite_frames
        for fmt in ("s16", "f32"):
            r, (y, E, rows) = recs[by[f"silence_{fmt}_1ch"]], each[by[f"silence_{fmt}_1ch"]]
            assert (r.flags, r.rows, r.silent_rows, r.key) == (C | NONE, 4, 4, 0) and not rows.any() and not y.any()
            r, (y, E, rows) = recs[by[f"silence_then_chord_{fmt}_2ch"]], each[by[f"silence_then_chord_{fmt}_2ch"]]
            assert r.rows == 21 and not rows[:5].any() and rows[8:].any(axis=1).all() and 5 <= r.silent_rows <= 8
            assert (r.flags, rg.key_name(r.key)) == (C, "C major")
        r = recs[by["chord_2s_s16_2ch"]]
        assert (r.flags, r.rows, rg.key_name(r.key)) == (C, 14, "A minor") and int(each[by["chord_2s_s16_2ch"]][2].max()) <= 800
    # the third channel does not count
    k = by["m4096_s16_3ch"]
    arena, descs = kc.pack([kc.Case("two", cs[k].channels[:2], 44100)])
    assert rg.key_arena(None, 2, descs, arena)[1].tobytes() == each[k][0].tobytes()


def test_routes_agree_on_the_records_and_stage_2_runs_behind_stage_1(routes):
    cs, got, _ = routes
    for c, a, b in zip(cs, got[0][0], got[2][0]):
        assert bytes(a) == bytes(b), c.name
    for route in (0, 2):
        for c, r, (_, _, rows) in zip(cs, got[route][0], _slices(*got[route])):
            want = kc.ref_stage2(rows)
            assert kc.record_fields(r) == want, c.name
    k = next(k for k, c in enumerate(cs) if c.name == "silence_then_chord_s16_2ch")
    arena, descs = kc.pack([cs[k]])
    recs, _, _, rows = rg.key_arena(None, 2, descs, arena, segment=8, bands=False)
    assert kc.record_fields(recs[0]) == kc.ref_stage2(rows, 8) and recs[0].segments == 2 and recs[0].stable_permille >= 500


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
                rg.key_arena(None, route, [desc], arena)
            assert e.value.code == code and text in str(e.value)
    ok = _capi.TrackDesc(0, 4, 44100, 2, S16)
    with pytest.raises(rg.ReplayGainError) as e:
        rg.key_arena(None, 3, [ok], arena)
    assert e.value.code == RG_ERR_INVALID_ARG
    for bad in (7, 4097):
        for route in (0, 2):
            with pytest.raises(rg.ReplayGainError) as e:
                rg.key_arena(None, route, [ok], arena, segment=bad)
            assert e.value.code == RG_ERR_INVALID_ARG and f"key: segment {bad}" in str(e.value)
    r = rg.key_arena(None, 0, [_capi.TrackDesc(0, 4, 0, 8, S16)], arena)[0][0]  # no rate: not supported, no error
    assert (r.status, r.flags) == (0, _capi.KEY_COMPLETE | _capi.KEY_SHORT | _capi.KEY_RATE)
    assert rg.key_arena(None, 0, [], arena)[0] == []
    W, lanes, T, tile_lanes, lds = rg.key_kernel_shape()
    assert (W, lanes, tile_lanes) == (256, 256, 256) and T % 2 == 1 and 64 * 1024 < lds <= 80 * 1024


def test_names_and_wheels():
    assert [rg.key_name(k) for k in (0, 21, 13, 10)] == ["C major", "A minor", "C# minor", "Bb major"]
    assert [rg.key_camelot(k) for k in (0, 21, 7, 12, 5, 16)] == ["8B", "8A", "9B", "5A", "7B", "9A"]
    assert [rg.key_open_key(k) for k in (0, 21, 7)] == ["1d", "1m", "2d"]
    assert sorted(rg.key_camelot(k) for k in range(24)) == sorted(f"{n}{l}" for n in range(1, 13) for l in "AB")
