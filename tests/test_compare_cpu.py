"""The null test of two tracks on the host (include/mp3rgain_amd_compare.h): the serial twin (rg_compare_arena route 0) and the
kernels' cutting and fold arithmetic (route 2) on the shared cases (tests/compare_cases.py), byte for byte against each other --
records, lag rows and block rows -- and field for field against the numpy / Python-int restatement: exactly in front of the
finish, 1e-12 relative behind it.  The tie rules of the pick, the refusals and the readings.  No GPU."""
import ctypes as C
import math
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import arena_layouts as al  # noqa: E402
import compare_cases as cc  # noqa: E402

import mp3rgain_amd as rg  # noqa: E402
from mp3rgain_amd import _capi  # noqa: E402

RG_ERR_INVALID_ARG, RG_ERR_FORMAT = -1, -9
S16, S32, F32 = _capi.FMT_S16_PLANAR, _capi.FMT_S32_PLANAR, _capi.FMT_F32_PLANAR
MAX_BLOCKS = 1200  # rows asked for per pair: more than any case has (2 T + 3 frames in blocks of 7)


def _raw(recs):
    return b"".join(bytes(r) for r in recs)


def _raw_blocks(blocks):
    return b"".join(bytes(b) for per in blocks for b in per)


def run(ctx, route, call, layout=al.Layout("guard", "loud", "input", 3)):
    tracks = list(call.tracks)
    arena, descs, _ = al.pack(tracks, layout)
    return rg.compare_arena(ctx, route, list(descs)[:len(tracks)], call.pairs, arena, blocks_per_pair=MAX_BLOCKS, lag_sums=True, **call.opts)


@pytest.mark.parametrize("call", cc.calls(), ids=lambda c: c.name)
def test_host_routes_match_each_other_and_the_restatement(call):
    want = cc.wants(call.name)
    serial, s_blocks, s_rows = run(None, 0, call)
    folded, f_blocks, f_rows = run(None, 2, call)
    bad = [(i, cc.differences(cc.got(r), w)) for i, (r, w) in enumerate(zip(serial, want)) if cc.differences(cc.got(r), w)]
    assert not bad, f"{len(bad)} of {len(want)} records of the serial twin differ from the restatement: {bad[:3]}"
    R = call.opts["radius"]
    for i, w in enumerate(want):
        assert w["blocks"] <= MAX_BLOCKS
        diff = cc.row_differences(s_rows[i], s_blocks[i], w, R)
        assert not diff, (i, diff[:3])
    diff = [(i, cc.differences(cc.got(a), cc.got(b))) for i, (a, b) in enumerate(zip(folded, serial)) if bytes(a) != bytes(b)]
    assert _raw(folded) == _raw(serial), diff[:3]
    assert f_rows.tobytes() == s_rows.tobytes()
    assert _raw_blocks(f_blocks) == _raw_blocks(s_blocks)


def test_the_case_list_covers_what_it_claims():
    P16, T = cc.shape(S16)
    assert (P16, T) == (8192, 4096) and cc.shape(S32) == cc.shape(F32) == (4096, 4096) and cc.shape(S16, F32) == (4096, 4096)
    assert rg.compare_kernel_shape(S16)[2:] == (16, 16, 2 * 4096 + 2 * 8192 + 8 * 4098)
    for R in cc.RADII:
        w = cc.wants(f"r{R}_s16")
        assert {x["frames_a"] for x in w[:8]} == {1, 15, 16, 17, T - 1, T, T + 1, 2 * T + 3}
        # the two hints that leave nothing, and the two that leave one frame
        assert [bool(x["flags"] & _capi.CMP_NO_OVERLAP) for x in w[8:12]] == [True, True, False, False]
        assert [x["segments"] and (x["frames_a"] - abs(x["hint"])) for x in w[10:12]] == [1, 1]
        # a copy at +-R from the hint is found at the edge, where the files are long enough to tell (channel 1 of these cases is
        # independent noise, so half of the energy correlates)
        if R:
            edge = [x for x in w[:8] if x["frames_a"] > 2 * R and abs(x["lag"]) == R]
            assert {x["lag"] for x in edge} == {-R, R} and all(x["flags"] & _capi.CMP_AT_EDGE and x["lock"] > 0.2 for x in edge), R
    # segments: 16 of them, the drifting copy flagged, the short pair one segment
    w = cc.wants(f"seg16x{T + 1}")
    assert (w[0]["segments"], w[0]["locked_segments"], w[0]["lag"]) == (16, 16, 3) and not w[0]["flags"] & _capi.CMP_DRIFT
    assert w[1]["flags"] & _capi.CMP_DRIFT and (w[1]["seg_lag_min"], w[1]["seg_lag_max"]) == (3, 5) and w[2]["segments"] == 1
    assert cc.wants(f"seg4x{T}")[2]["segments"] == 1 and cc.wants(f"seg1x{T}")[2]["segments"] == 1 and cc.wants("seg4x0")[0]["segments"] == 1
    # blocks of 1, 7, T + 1 and the default; mixed formats in both orders
    assert cc.wants("b1")[0]["blocks"] == 299 and cc.wants("b7")[0]["blocks"] == (2 * T + 2 + 6) // 7 and cc.wants(f"b{T + 1}")[0]["blocks"] == 2
    assert {(x["format_a"], x["format_b"]) for x in cc.wants("bNone")} == {(a, b) for a in (S16, S32, F32) for b in (S16, S32, F32)}
    assert all(x["lag"] == 1 and x["differing_blocks"] for x in cc.wants("bNone"))
    assert [x["channels"] for x in cc.wants("channels")] == [1, 1, 1, 2, 8]
    assert [bool(x["flags"] & _capi.CMP_CHANNELS_DIFFER) for x in cc.wants("channels")] == [False, True, True, True, False]
    v = cc.wants("values")
    assert all(x["polarity"] == -1 and x["lag"] == 2 and x["flags"] & _capi.CMP_INVERTED for x in v[:3])
    # a 32-bit sum cannot hold these
    assert v[3]["aa"] == v[3]["ab"] == 2 * (2 * T + 3) << 30 and v[3]["flags"] & _capi.CMP_IDENTICAL
    assert v[4]["ab"] == -(2 * T + 3) * 32768 * 32767 and v[4]["polarity"] == -1
    assert sum(bool(x["flags"] & _capi.CMP_NONFINITE) for x in v) == 5 and v[-1]["flags"] & _capi.CMP_RATE
    # the single differing sample
    P = P16
    assert [(x["first_diff"], x["differing_blocks"], x["max_diff"], x["equal"]) for x in cc.wants(f"single_b{T + 1}")] == \
        [(T + 1, 1, 1, 2 * (P + 10) - 1), (0, 1, 1, 2 * (P + 10) - 1)]
    assert [(x["first_diff"], x["differing_blocks"]) for x in cc.wants("single_bNone")] == [(P - 1, 1), (P + 9, 1)]
    assert sorted(x["lag"] for x in cc.wants("residues")) == sorted(list(range(-8, 9)) * 3)


def _pair(a, b, dtype=np.int16, **opts):
    tracks = [cc.Tr("a", [cc.scaled(a, dtype)], 44100), cc.Tr("b", [cc.scaled(b, dtype)], 44100)]
    arena, descs, _ = al.pack(tracks, al.Layout("guard", "loud", "input", 1))
    o = dict(radius=3, segments=1, segment_frames=0)
    o.update(opts)
    r = rg.compare_arena(None, 0, list(descs)[:2], [(0, 1, 0)], arena, **o)[0]
    f = rg.compare_arena(None, 2, list(descs)[:2], [(0, 1, 0)], arena, **o)[0]
    assert bytes(r) == bytes(f)
    assert not cc.differences(cc.got(r), cc.want_pair(tracks, 0, 1, 0, **o))
    return r


@pytest.mark.parametrize("dtype", [np.int16, np.int32, np.float32])
def test_the_tie_rules_of_the_pick(dtype):
    a = [0, 0, 0, 0, 9, 0, 0, 0, 0]
    # two equal maxima at +-1: the negative lag
    r = _pair(a, [0, 0, 0, 9, 0, 9, 0, 0, 0], dtype)
    assert (r.lag, r.polarity, r.ab) == (-1, 1, 81)
    # +81 at -1 against -81 at +1, and the other way round: the negative lag, whatever its sign
    r = _pair(a, [0, 0, 0, 9, 0, -9, 0, 0, 0], dtype)
    assert (r.lag, r.polarity, r.ab) == (-1, 1, 81)
    r = _pair(a, [0, 0, 0, -9, 0, 9, 0, 0, 0], dtype)
    assert (r.lag, r.polarity, r.ab) == (-1, -1, -81) and r.flags & _capi.CMP_INVERTED
    # +81 at -2 against -81 at +1: the smaller |d|, whatever its sign
    r = _pair(a, [0, 0, 9, 0, 0, -9, 0, 0, 0], dtype)
    assert (r.lag, r.polarity) == (1, -1)
    r = _pair(a, [0, 0, -9, 0, 0, 9, 0, 0, 0], dtype)
    assert (r.lag, r.polarity) == (1, 1)
    # nothing correlates anywhere: lag 0, polarity +1, no lock
    r = _pair(a, [0] * 9, dtype)
    assert (r.lag, r.polarity, r.lock) == (0, 1, 0.0) and r.flags & _capi.CMP_UNRELATED and not r.flags & _capi.CMP_AT_EDGE


def test_known_verdicts_and_readings():
    rng = np.random.default_rng(11)
    x = rng.integers(-20000, 20000, size=6000).astype(np.int16)

    def one(a, b, hint=0, rate_b=44100, **opts):
        tracks = [cc.Tr("a", [a], 44100), cc.Tr("b", [b], rate_b)]
        arena, descs, _ = al.pack(tracks, al.Layout("abut", "loud", "input"))
        o = dict(radius=64, segments=1, segment_frames=0)
        o.update(opts)
        return rg.compare_from_record(rg.compare_arena(None, 0, list(descs)[:2], [(0, 1, hint)], arena, **o)[0])

    c = one(x, x.copy())
    assert c.verdicts == ["identical"] and c.reading == "identical" and c.null_db == -math.inf and c.gain_db == 0.0 and c.residual_lsb2 == 0.0
    c = one(x[588:].copy(), x[:-1176].copy(), radius=1024)
    assert (c.lag, c.a_head, c.b_head, c.a_tail, c.b_tail) == (588, 0, 588, 1176, 0) and "identical" in c.verdicts and "shifted" in c.verdicts
    assert c.reading == "identical samples, starts 588 samples later, 1176 shorter at the end"
    half = np.rint(x * 10 ** (-3.01 / 20) + rng.triangular(-1, 0, 1, size=len(x))).astype(np.int16)
    c = one(half, x)
    assert c.verdicts == ["same master"] and c.reading.startswith("same master  (gain -3.01 dB, residual 0.") and 0.1 < c.residual_lsb2 < 0.5
    other = (x + rng.integers(-3000, 3000, size=len(x))).astype(np.int16)
    c = one(x, other)
    assert c.verdicts == ["differs"] and c.reading.startswith("same recording, differs  (null -") and "worst 0:00-0:01 at" in c.reading
    assert "first difference at 0:00.000" in c.reading
    c = one(x, rng.integers(-20000, 20000, size=6000).astype(np.int16))
    assert c.verdicts[0] == "unrelated" and c.reading.startswith("not the same recording  (best correlation 0.0")
    c = one(x, (-x).astype(np.int16))
    assert c.verdicts[:2] == ["same master", "inverted"] or c.verdicts[:2] == ["differs", "inverted"]
    assert c.polarity == -1 and c.equal == len(x) and c.reading.startswith("inverted copy, same master")
    c = one(x, x.copy(), rate_b=48000)
    assert c.verdicts == ["different sample rate"] and c.reading == "different sample rate: not compared" and c.overlap == 0
    c = one(x, x.copy(), hint=6000)
    assert c.verdicts == ["no overlap"]
    c = one(x, x.copy(), lock_permille=1000, requant_millilsb2=1)
    assert c.verdicts == ["identical"]
    c = one(half, x, requant_millilsb2=100)
    assert c.verdicts == ["differs"]


def test_options_and_refusals():
    arena = np.zeros(64, dtype=np.uint8)
    ok = [_capi.TrackDesc(0, 4, 44100, 2, S16), _capi.TrackDesc(16, 4, 44100, 2, S16)]
    pair = [(0, 1, 0)]
    for route in (0, 2):
        for descs, pairs, opts, code, text in (
                ([_capi.TrackDesc(0, 17, 44100, 2, S16), ok[1]], pair, {}, RG_ERR_INVALID_ARG, "beyond the arena"),
                ([ok[0], _capi.TrackDesc(1, 4, 44100, 2, S16)], pair, {}, RG_ERR_INVALID_ARG, "sample-aligned"),
                ([ok[0], _capi.TrackDesc(0, 1, 44100, 9, S16)], pair, {}, RG_ERR_FORMAT, "9 channel"),
                ([ok[0], _capi.TrackDesc(0, 1, 44100, 2, 7)], pair, {}, RG_ERR_FORMAT, "format 7"),
                (ok, [(0, 0, 0)], {}, RG_ERR_INVALID_ARG, "against itself"),
                (ok, [(0, 2, 0)], {}, RG_ERR_INVALID_ARG, "is not a pair of the 2 tracks"),
                (ok, [(5, 1, 0)], {}, RG_ERR_INVALID_ARG, "is not a pair of the 2 tracks"),
                (ok, [(0, 1, (1 << 32) + 1)], {}, RG_ERR_INVALID_ARG, "hint"),
                (ok, pair, {"radius": 2048}, RG_ERR_INVALID_ARG, "radius 2048"),
                (ok, pair, {"segments": 0}, RG_ERR_INVALID_ARG, "segments 0"),
                (ok, pair, {"segments": 17}, RG_ERR_INVALID_ARG, "segments 17"),
                (ok, pair, {"coarse_radius": 2048}, RG_ERR_INVALID_ARG, "coarse_radius 2048"),
                (ok, pair, {"coarse_radius": 0}, RG_ERR_INVALID_ARG, "coarse_radius 0"),
                (ok, pair, {"align": 2}, RG_ERR_INVALID_ARG, "align 2"),
                (ok, pair, {"block_frames": 384001}, RG_ERR_INVALID_ARG, "block_frames"),
                (ok, pair, {"lock_permille": 0}, RG_ERR_INVALID_ARG, "lock_permille"),
                (ok, pair, {"lock_permille": 1001}, RG_ERR_INVALID_ARG, "lock_permille"),
                (ok, pair, {"requant_millilsb2": 0}, RG_ERR_INVALID_ARG, "requant_millilsb2"),
                ([_capi.TrackDesc(0, 4, 384001, 2, S16), _capi.TrackDesc(16, 4, 384001, 2, S16)], pair, {}, RG_ERR_INVALID_ARG, "a block of 384001 frames")):
            with pytest.raises(rg.ReplayGainError) as e:
                rg.compare_arena(None, route, descs, pairs, arena, **opts)
            assert e.value.code == code and text in str(e.value), (route, str(e.value))
        r = rg.compare_arena(None, route, ok, pair, arena)[0]
        assert (r.status, r.channels, r.block_frames, r.radius, r.segments, r.overlap, r.lag) == (0, 2, 44100, 1024, 1, 4, 0)
        assert r.flags == _capi.CMP_COMPLETE | _capi.CMP_IDENTICAL | _capi.CMP_UNRELATED | _capi.CMP_RAW  # silence locks on nothing
        assert rg.compare_arena(None, route, ok, [], arena) == []
    with pytest.raises(rg.ReplayGainError) as e:
        rg.compare_arena(None, 3, ok, pair, arena)
    assert e.value.code == RG_ERR_INVALID_ARG
    assert _capi.load().rg_compare_arena(None, 1, 0, None, 0, None, None, None, 0, None, None, 0, None) == RG_ERR_INVALID_ARG  # the kernels need a context
    with pytest.raises(rg.ReplayGainError):
        rg.compare_kernel_shape(3)
    assert C.sizeof(_capi.CompareRecord) == 280 and C.sizeof(_capi.CompareOpts) == 36 and C.sizeof(_capi.CompareBlock) == 48 and C.sizeof(_capi.ComparePair) == 16
