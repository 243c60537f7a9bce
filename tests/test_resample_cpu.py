"""The rational resampler and the cross-rate duplicate finder on the CPU (include/mp3rgain_amd_resample.h): the plan and the
window against Python integers, the tap tables, the host routes (0: the sum in double, 2: the kernels' arithmetic) on the shared
cases (tests/resample_cases.py) against lengths counted in Python integers and a float64 reference, the composition with the
existing fingerprint seam, and the behaviour: one piece rendered at six rates, found as one recording."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import resample_cases as rc  # noqa: E402

import mp3rgain_amd as rg  # noqa: E402
from mp3rgain_amd import _capi  # noqa: E402


@pytest.fixture(scope="module")
def routes():
    cases = rc.cases()
    arena, descs = rc.pack(cases)
    return cases, {route: rg.resample_arena(None, route, descs, arena) for route in (0, 2)}


# ---- plan, window, filter ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", rc.PLAN_RATES)
def test_plan_and_window_against_python_integers(rate):
    L, M, P, ok = rc.plan(rate)
    assert rg.resample_plan(rate) == (L, M, P, ok)
    assert ok == (rate not in (44056, 384000))
    if rate == 37800:
        assert (L, M) == (7, 24)
    if not ok:
        with pytest.raises(rg.ReplayGainError) as e:
            rg.resample_window(rate, 0)
        assert e.value.code == _capi.RG_ERR_UNSUPPORTED_RATE
        return
    for j in (0, 1, L - 1, L, 2 ** 31, 2 ** 32 - 1):
        b, p = rg.resample_window(rate, j)
        assert (b, p) == rc.window(rate, j) and 0 <= p < L and b * L - p == j * M
    assert M == 1 or (2 ** 32 - 1) * M > 2 ** 32


@pytest.mark.parametrize("D", (2, 4, 8, 16, 32))
def test_filter_of_one_phase_is_the_key_scans(D):
    assert rg.resample_filter(1, D).tobytes() == np.asarray(rg.key_filter(D), dtype=np.float32).tobytes()


@pytest.mark.parametrize("L,M", ((147, 640), (441, 320)))
def test_every_phase_sums_to_one(L, M):
    h = rg.resample_filter(L, M)
    assert h.shape == (L, 2 * 8 * max(L, M) // L + 1)
    assert np.abs(h.astype(np.float64).sum(axis=1) - 1.0).max() <= 2.0 ** -23


def test_filter_is_the_headers_prototype():
    """h[p][k] = G[p + k L - half] normalised per phase, restated in numpy float64."""
    L, M = 147, 640
    W, half, P = 640, 8 * 640, 70
    n = (np.arange(L)[:, None] + np.arange(P)[None, :] * L - half).astype(np.float64)
    c = 0.45 / W
    G = 2 * c * np.sinc(2 * c * n) * (0.42 + 0.5 * np.cos(np.pi * n / half) + 0.08 * np.cos(2 * np.pi * n / half))
    G[np.abs(n) > half] = 0.0
    G /= G.sum(axis=1, keepdims=True)
    # a normalised phase has taps up to 2c L = 0.21, in [0.125, 0.25): rounding to f32 moves one by at most half an ulp, 2^-27
    assert G.max() < 0.25 and np.abs(rg.resample_filter(L, M).astype(np.float64) - G).max() <= 2.0 ** -27 + 1e-12
    for bad in ((0, 1), (442, 1), (2, 65), (2, 4)):
        with pytest.raises(rg.ReplayGainError):
            rg.resample_filter(*bad)
    assert rg.resample_filter(1, 1).tolist() == [[1.0]]


def test_kernel_shape():
    outputs, lanes, span = rg.resample_kernel_shape()
    assert (outputs, lanes) == (256, 256) and span * 4 <= 65536
    assert span >= max(-(-255 * rc.plan(r)[1] // rc.plan(r)[0]) + rc.plan(r)[2] for r in rc.PLAN_RATES if rc.plan(r)[3])


# ---- the host routes on the shared cases -----------------------------------------------------------------------------------------
def test_lengths_and_records(routes):
    cases, got = routes
    assert _raw(got[0][0]) == _raw(got[2][0])
    at = 0
    for c, r in zip(cases, got[2][0]):
        n = len(c.channels[0])
        L, M, P, ok = rc.plan(c.sample_rate)
        m = rc.m_of(n, c.sample_rate)
        assert (r.status, r.frames, r.sample_rate, r.channels, r.up, r.down, r.taps, r.resampled, r.y_at) == \
            (0, n, c.sample_rate, len(c.channels), L, M, P, m, at), c.name
        assert r.flags == (0 if ok else _capi.RS_RATE) | (0 if m else _capi.RS_SHORT), c.name
        at += m
    names = {c.name.split("_r")[0]: rc.m_of(len(c.channels[0]), c.sample_rate) for c in cases if c.sample_rate == 48000}
    assert (names["m0"], names["m1"], names["m255"], names["m256"], names["m257"], names["m511"], names["m300_tail"]) == (0, 1, 255, 256, 257, 511, 300)


def _raw(recs):
    return b"".join(bytes(r) for r in recs)


@pytest.mark.parametrize("route", (0, 2))
def test_routes_against_the_float64_reference(routes, route):
    """The bound is the recorded error of route 2 per rate (tests/golden/xrate_measured.json) times TOLERANCE_FACTOR."""
    cases, got = routes
    recs, y = got[route]
    bound = rc.measured()["y_error_route2"]
    worst = {}
    for c, r in zip(cases, recs):
        mine = y[r.y_at:r.y_at + r.resampled]
        ref = rc.reference(c)
        assert len(ref) == len(mine), c.name
        assert (np.isnan(ref) == np.isnan(mine)).all(), c.name
        worst[c.sample_rate] = max(worst.get(c.sample_rate, 0.0), rc.y_error(mine, ref))
    print({k: f"{v:.3e}" for k, v in worst.items()})
    for rate, e in worst.items():
        assert e <= rc.TOLERANCE_FACTOR * bound[str(rate)], (rate, e, bound[str(rate)])


@pytest.mark.parametrize("route", (0, 2))
def test_a_nan_reaches_exactly_the_windows_that_hold_it(routes, route):
    cases, got = routes
    recs, y = got[route]
    seen = 0
    for c, r in zip(cases, recs):
        if not c.name.startswith("nan_"):
            continue
        mine = y[r.y_at:r.y_at + r.resampled]
        want = rc.nan_outputs(c.sample_rate, rc.nan_at(c.sample_rate), r.resampled)
        assert np.flatnonzero(np.isnan(mine)).tolist() == want and 0 < len(want) < 40, c.name
        seen += 1
    assert seen == 3


def test_identity_is_byte_for_byte(routes):
    cases, got = routes
    for route in (0, 2):
        recs, y = got[route]
        n = 0
        for c, r in zip(cases, recs):
            if c.sample_rate == rc.FC:
                assert y[r.y_at:r.y_at + r.resampled].tobytes() == rc.signal(c).tobytes()
                n += 1
        assert n == 2


def test_the_third_channel_does_not_count(routes):
    cases, got = routes
    c = next(c for c in cases if c.name.startswith("m257_r48000"))
    assert len(c.channels) == 3
    arena, descs = rc.pack([rc.Case("two", list(c.channels[:2]), c.sample_rate)])
    i = cases.index(c)
    r = got[2][0][i]
    assert rg.resample_arena(None, 2, descs, arena)[1].tobytes() == got[2][1][r.y_at:r.y_at + r.resampled].tobytes()


# ---- composition with the fingerprint ---------------------------------------------------------------------------------------------
def _long_cases():
    mk = lambda n, fmt, seed: rc.fc.as_format(rc.fc.noise(n, seed), fmt)  # noqa: E731
    return [rc.Case("c48", [mk(rc.n_for(4096 + 9 * 512 + 17, 48000), "s16", 1), mk(rc.n_for(4096 + 9 * 512 + 17, 48000), "s16", 2)], 48000),
            rc.Case("c8", [mk(rc.n_for(4096 + 512, 8000), "f32", 3)], 8000),
            rc.Case("c44", [mk(rc.n_for(4096 + 3 * 512, 44100), "s32", 4)], 44100),
            rc.Case("cshort", [mk(rc.n_for(4095, 32000), "s16", 5)], 32000),
            rc.Case("cbad", [mk(9000, "s16", 6)], 44056)]


@pytest.mark.parametrize("route", (0, 2))
def test_composition_with_the_fingerprint_seam(route):
    """y of route r handed to rg_fingerprint_arena (route r) as a mono f32 track at 11025 Hz: the codes and band energies
    of rg_xrate_fingerprint_arena, byte for byte."""
    cases = _long_cases()
    arena, descs = rc.pack(cases)
    recs, codes, bands, y = rg.xrate_fingerprint_arena(None, route, descs, arena)
    plain, py = rg.resample_arena(None, route, descs, arena)
    assert py.tobytes() == y.tobytes()
    ycases = [rc.Case(c.name, [y[r.y_at:r.y_at + r.resampled].copy()], rc.FC) for c, r in zip(cases, recs) if r.resampled]
    yarena, ydescs = rc.pack(ycases)
    frecs, fcodes, fbands = rg.fingerprint_arena(None, route, ydescs, yarena)
    assert fcodes.tobytes() == codes.tobytes() and fbands.tobytes() == bands.tobytes() and len(codes) == 9 + 1 + 3
    assert [int(r.codes) for r in recs] == [9, 1, 3, 0, 0] and [int(r.fp_frames) for r in recs] == [10, 2, 4, 0, 0]
    assert [int(r.flags) for r in recs] == [_capi.FP_COMPLETE, _capi.FP_COMPLETE, _capi.FP_COMPLETE, _capi.FP_COMPLETE | _capi.FP_SHORT,
                                            _capi.FP_COMPLETE | _capi.FP_SHORT | _capi.FP_RATE]
    for r, p, c in zip(recs, plain, cases):
        assert (r.up, r.down, r.resampled, r.y_at, r.sample_rate, r.frames) == (p.up, p.down, p.resampled, p.y_at, c.sample_rate, len(c.channels[0]))
    assert [int(r.group) for r in recs] == list(range(5))


def test_route0_and_route2_codes_differ_in_few_bits():
    cases = _long_cases()
    arena, descs = rc.pack(cases)
    a = rg.xrate_fingerprint_arena(None, 0, descs, arena, bands=False)[1]
    b = rg.xrate_fingerprint_arena(None, 2, descs, arena, bands=False)[1]
    flipped = int(rc.fc.popcount(a ^ b).sum())
    assert flipped <= max(2, rc.TOLERANCE_FACTOR * rc.measured()["flipped_share"] * 32 * len(a))


# ---- behaviour -------------------------------------------------------------------------------------------------------------------
def test_one_piece_at_six_rates_is_one_recording():
    """One continuous-time piece rendered at 44100, 48000, 96000, 32000, 22050 and 8000 Hz, the 48000 Hz one again delayed by
    133.7 ms, and an unrelated piece: at the default options every same-recording pair matches at its expected lag, and no
    pair with the unrelated piece does.  The same-rate finder skips every mixed-rate pair of these."""
    tracks = rc.behaviour_tracks()
    codes, recs = rc.xrate_codes(tracks)
    assert all(r.codes >= _capi.XR_BLOCK for r in recs) and len({int(r.sample_rate) for r in recs}) == 6
    rec = rc.match(codes)
    assert rc.match(codes).tobytes() == rg.fingerprint_match_codes(None, 0, codes, [rc.FC] * len(codes), block=_capi.XR_BLOCK, probes=_capi.XR_PROBES,
                                                                   radius=_capi.XR_RADIUS, max_ber_permille=_capi.XR_MAX_BER_PERMILLE).tobytes()
    k = 0
    for i in range(len(tracks)):
        for j in range(i + 1, len(tracks)):
            r = rec[k]
            k += 1
            same = tracks[i][4] == tracks[j][4]
            assert bool(r["flags"] & _capi.FP_PAIR_MATCH) == same, (tracks[i][0], tracks[j][0], int(r["errors"]), int(r["bits"]))
            if same:
                assert abs(int(r["lag"]) - rc.expected_lag(int(r["flags"]), tracks[i][3], tracks[j][3])) <= 0.5, (tracks[i][0], tracks[j][0], int(r["lag"]))
    groups, _, found = rg.fingerprint_groups(len(tracks), rec)
    assert groups.tolist() == [0] * 7 + [7] and found == 21
    # what the project could do before: the same-rate fingerprint and match skip every mixed-rate pair
    cs = [rc.Case(t[0], [t[2]], t[1]) for t in tracks]
    arena, descs = rc.pack(cs)
    frecs, fcodes, _ = rg.fingerprint_arena(None, 2, descs, arena, bands=False)
    old = rg.fingerprint_match_codes(None, 0, [fcodes[r.codes_at:r.codes_at + r.codes] for r in frecs], [t[1] for t in tracks])
    k = 0
    for i in range(len(tracks)):
        for j in range(i + 1, len(tracks)):
            if tracks[i][1] != tracks[j][1]:
                assert old[k]["flags"] == _capi.FP_PAIR_SKIPPED
            k += 1


def test_the_threshold_is_the_measured_midpoint():
    m = rc.measured()
    assert m["same_recording_max_ber"] < m["unrelated_min_ber"] and not m["overlap"] and not m["wrong_lags"]
    assert m["max_ber_permille"] == _capi.XR_MAX_BER_PERMILLE == int(round(1000 * (m["same_recording_max_ber"] + m["unrelated_min_ber"]) / 2))
    header = (rc.ROOT / "include" / "mp3rgain_amd_resample.h").read_text()
    assert f"#define RG_XR_MAX_BER_PERMILLE {m['max_ber_permille']}u" in header


def test_host_routes_refuse_bad_tracks():
    arena = np.zeros(64, dtype=np.uint8)
    S16 = _capi.FMT_S16_PLANAR
    for desc, code, text in ((_capi.TrackDesc(0, 17, 48000, 2, S16), -1, "beyond the arena"), (_capi.TrackDesc(1, 4, 48000, 2, S16), -1, "sample-aligned"),
                             (_capi.TrackDesc(0, 1, 48000, 9, S16), -9, "9 channel")):
        for fn in (rg.resample_arena, rg.xrate_fingerprint_arena):
            with pytest.raises(rg.ReplayGainError) as e:
                fn(None, 2, [desc], arena)
            assert e.value.code == code and text in str(e.value)
    with pytest.raises(rg.ReplayGainError):
        rg.resample_arena(None, 1, [], arena)  # route 1 needs a context
    with pytest.raises(rg.ReplayGainError):
        rg.resample_arena(None, 3, [], arena)
