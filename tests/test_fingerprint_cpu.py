"""Stage 1 of the duplicate finder on the CPU (include/mp3rgain_amd_fingerprint.h): the serial host twin (rg_fingerprint_arena
route 0) and the kernels' arithmetic on the host (route 2) against the float64 numpy reference of tests/fingerprint_cases.py,
within the bounds tools/fingerprint_refcheck.py recorded (tests/golden/fingerprint_measured.json, times TOLERANCE_FACTOR); the
edge table against the formula; the records of the short, rate and non-finite cases; descriptor errors.  No GPU."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import fingerprint_cases as fc  # noqa: E402

import mp3rgain_amd as rg  # noqa: E402
from mp3rgain_amd import _capi  # noqa: E402

RG_ERR_INVALID_ARG, RG_ERR_FORMAT = -1, -9
GAIN_RATES = (8000, 11025, 12000, 16000, 18900, 22050, 24000, 32000, 37800, 44100, 48000, 56000)


@pytest.fixture(scope="module")
def routes():
    cs = fc.cases()
    arena, descs = fc.pack(cs)
    return cs, {r: rg.fingerprint_arena(None, r, descs, arena) for r in (0, 2)}, [fc.reference(c) for c in cs]


def _slices(rec, codes, bands):
    return codes[rec.codes_at:rec.codes_at + rec.codes], bands[rec.frames_at:rec.frames_at + rec.fp_frames].astype(np.float64)


@pytest.mark.parametrize("route", (0, 2))
def test_band_energies_within_the_recorded_bound(routes, route):
    cs, got, refs = routes
    recs, codes, bands = got[route]
    bound = fc.TOLERANCE_FACTOR * fc.measured()[f"band_error_route{route}"]
    assert 0 < bound < 1e-5  # f32 band sums: a few units of 2^-24 of the frame's largest band
    for c, r, ref in zip(cs, recs, refs):
        assert (r.fp_frames, r.codes) == (ref.frames, len(ref.codes)), c.name
        assert fc.band_error(_slices(r, codes, bands)[1], ref.bands) <= bound, c.name


@pytest.mark.parametrize("route", (0, 2))
def test_code_bits_differ_from_the_reference_only_where_its_margin_is_tiny(routes, route):
    cs, got, refs = routes
    recs, codes, bands = got[route]
    m = fc.measured()
    flips = bits = 0
    for c, r, ref in zip(cs, recs, refs):
        f, margin = fc.flipped(_slices(r, codes, bands)[0], ref)
        flips, bits = flips + f, bits + 32 * int(r.codes)
        assert f == 0 or margin <= m["flipped_margin_max"], (c.name, f, margin)
    assert bits > 9000 and flips <= fc.TOLERANCE_FACTOR * m["flipped_share"] * bits, (flips, bits)


def test_the_edge_table_is_the_formula():
    for rate in GAIN_RATES + (64000, 88200, 96000, 192000, 4000):
        want, ok = fc.edges(rate)
        got, supported = rg.fingerprint_edges(rate)
        assert got == want and supported == ok == (4000 <= rate <= 88200), rate  # 4000: e[33] = 2048, the last bin used is 2047
    e = rg.fingerprint_edges(44100)[0]
    assert (e[0], e[33]) == (28, 186) and min(b - a for a, b in zip(e, e[1:])) == 1  # the narrowest band is one bin
    e = rg.fingerprint_edges(48000)[0]
    assert min(b - a for a, b in zip(e, e[1:])) == 1
    assert rg.fingerprint_edges(8000)[0][33] == 1024
    for rate in range(4000, 74373, 37):  # every rate from 4000 to 74372 Hz passes (a sweep; the formula says the same of all)
        assert rg.fingerprint_edges(rate)[1] and fc.edges(rate)[1], rate
    # above that two edges can round to the same bin: 74373 and 96000 Hz fail, 88200 Hz passes
    assert [rg.fingerprint_edges(rate)[1] for rate in (3999, 74372, 74373, 88200, 96000)] == [False, True, False, True, False]
    with pytest.raises(rg.ReplayGainError):
        rg.fingerprint_edges(0)


def test_records_of_the_short_rate_and_nonfinite_cases(routes):
    cs, got, refs = routes
    by = {c.name: k for k, c in enumerate(cs)}
    T = fc.tile_codes()
    C, S, R, N = _capi.FP_COMPLETE, _capi.FP_SHORT, _capi.FP_RATE, _capi.FP_NONFINITE
    for route in (0, 2):
        recs = got[route][0]
        for k, r in enumerate(recs):
            assert (r.status, r.dropped_frames, r.group, r.matches, r.frames) == (0, 0, k, 0, len(cs[k].channels[0])), cs[k].name
            assert (r.channels, r.sample_rate) == (len(cs[k].channels), cs[k].sample_rate)
        for fmt in ("s16", "s32", "f32"):
            r = recs[by[f"n4095_{fmt}_1ch"]]
            assert (r.flags, r.fp_frames, r.codes) == (C | S, 0, 0)
            r = recs[by[f"n4096_{fmt}_1ch"]]
            assert (r.flags, r.fp_frames, r.codes) == (C | S, 1, 0)
            r = recs[by[f"n4608_{fmt}_3ch"]]
            assert (r.flags, r.fp_frames, r.codes, r.channels) == (C, 2, 1, 3)
        r = recs[by["rate96000_s16_1ch"]]
        assert (r.flags, r.fp_frames, r.codes, r.sample_rate) == (C | S | R, 0, 0, 96000)
        r = recs[by["rate88200_s16_1ch"]]
        assert (r.flags, r.codes) == (C, 3)
        r = recs[by["nonfinite_f32_2ch"]]
        assert (r.flags, r.codes, r.nonfinite_frames) == (C | N, 2 * T + 2, 9)  # frames 4 .. 11 (the NaN) and the last (the Inf)
        E = got[route][2][r.frames_at:r.frames_at + r.fp_frames]
        assert not E[4:12].any() and not E[-1].any() and E[:4].all() and E[12:-1].all()
        r = recs[by["nan_first_f32_1ch"]]
        assert (r.flags, r.nonfinite_frames) == (C | N, 1)
    # the third channel does not count: the codes of the 3-channel case are those of its first two channels alone
    k = by["n4608_s16_3ch"]
    two = fc.Case("two", cs[k].channels[:2], 44100)
    arena, descs = fc.pack([two])
    r = got[2][0][k]
    assert rg.fingerprint_arena(None, 2, descs, arena)[1].tobytes() == got[2][1][r.codes_at:r.codes_at + r.codes].tobytes()


def test_routes_agree_on_everything_but_rounding(routes):
    cs, got, _ = routes
    for a, b in zip(got[0][0], got[2][0]):
        assert bytes(a) == bytes(b)


def test_descriptor_errors_are_the_plane_layers():
    arena = np.zeros(64, dtype=np.uint8)
    S16 = _capi.FMT_S16_PLANAR
    for desc, code, text in ((_capi.TrackDesc(0, 17, 44100, 2, S16), RG_ERR_INVALID_ARG, "beyond the arena"),
                             (_capi.TrackDesc(1, 4, 44100, 2, S16), RG_ERR_INVALID_ARG, "sample-aligned"),
                             (_capi.TrackDesc(0, 1, 44100, 9, S16), RG_ERR_FORMAT, "9 channel"),
                             (_capi.TrackDesc(0, 1, 44100, 0, S16), RG_ERR_FORMAT, "0 channel"),
                             (_capi.TrackDesc(0, 1, 44100, 1, 7), RG_ERR_FORMAT, "not a planar PCM format")):
        for route in (0, 2):
            with pytest.raises(rg.ReplayGainError) as e:
                rg.fingerprint_arena(None, route, [desc], arena)
            assert e.value.code == code and text in str(e.value)
    with pytest.raises(rg.ReplayGainError) as e:
        rg.fingerprint_arena(None, 3, [_capi.TrackDesc(0, 4, 44100, 2, S16)], arena)
    assert e.value.code == RG_ERR_INVALID_ARG
    r = rg.fingerprint_arena(None, 0, [_capi.TrackDesc(0, 4, 0, 8, S16)], arena)[0][0]  # no rate: not supported, no error
    assert (r.status, r.flags) == (0, _capi.FP_COMPLETE | _capi.FP_SHORT | _capi.FP_RATE)
    assert rg.fingerprint_arena(None, 0, [], arena)[0] == []
    assert rg.fingerprint_kernel_shape()[1] == 256 and rg.fingerprint_kernel_shape()[0] % 2 == 1  # T + 1 frames go through in pairs
