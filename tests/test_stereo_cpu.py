"""The stereo image scan on the host (include/mp3rgain_amd_stereo.h): the serial twin (rg_stereo_arena route 0) and the kernels'
cutting and fold arithmetic (route 2) on the shared cases (tests/stereo_cases.py), byte for byte against each other, records and
lag sums, and field for field against the numpy / Python-int restatement: exactly in front of the finish, 1e-12 relative behind
it.  No GPU."""
import ctypes as C
import math
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import arena_layouts as al  # noqa: E402
import stereo_cases as sc  # noqa: E402

import mp3rgain_amd as rg  # noqa: E402
from mp3rgain_amd import _capi  # noqa: E402

RG_ERR_INVALID_ARG, RG_ERR_FORMAT = -1, -9
S16, S32, F32 = _capi.FMT_S16_PLANAR, _capi.FMT_S32_PLANAR, _capi.FMT_F32_PLANAR


def _raw(recs):
    return b"".join(bytes(r) for r in recs)


def _run(route, group, layout=al.Layout("guard", "loud", "input", 3)):
    tracks = list(group.tracks)
    arena, descs, _ = al.pack(tracks, layout)
    return rg.stereo_arena(None, route, list(descs)[:len(tracks)], arena, group.radius, group.block_frames, lag_sums=True)


@pytest.mark.parametrize("group", sc.groups(), ids=lambda g: g.name)
def test_host_routes_match_each_other_and_the_restatement(group):
    tracks, want = list(group.tracks), sc.wants(group.name)
    serial, s_sums = _run(0, group)
    folded, f_sums = _run(2, group)
    bad = [(tr.name, sc.differences(sc.got(r), want[tr.name])) for tr, r in zip(tracks, serial) if sc.differences(sc.got(r), want[tr.name])]
    assert not bad, f"{len(bad)} of {len(tracks)} records of the serial twin differ from the restatement: {bad[:3]}"
    R = 64 if group.radius is None else group.radius
    for tr, r, row in zip(tracks, serial, s_sums):
        assert [int(v) for v in row] == want[tr.name]["sums"], tr.name
        assert int(row[R]) == r.elr, tr.name  # C_0 == ELR (and the restatement holds ELR to the sum of the blocks')
    diff = [(tr.name, sc.differences(sc.got(a), sc.got(b))) for tr, a, b in zip(tracks, folded, serial) if bytes(a) != bytes(b)]
    assert _raw(folded) == _raw(serial), diff[:3]
    assert f_sums.tobytes() == s_sums.tobytes()


def test_the_case_list_covers_what_it_claims():
    by_name = {(g.name, tr.name): tr for g in sc.groups() for tr in g.tracks}
    assert {tr.channels[0].dtype for tr in by_name.values()} == {np.dtype(np.int16), np.dtype(np.int32), np.dtype(np.float32)}
    assert {len(tr.channels) for tr in by_name.values()} >= {1, 2, 8}
    assert sc.shape(S16) == (8192, 4096) and sc.shape(S32) == sc.shape(F32) == (4096, 4096)
    for fmt, tag in ((S16, "s16"), (S32, "s32"), (F32, "f32")):
        P, T = sc.shape(fmt)
        for R in (0, 1, 7, 64, 255):
            for N in (0, 1, 2, R, R + 1, 2 * R + 1, P - 1, P, P + 1, T - 1, T, T + 1, T + R, 2 * T + 3):
                assert (f"r{R}_bNone", f"{tag}_n{N}") in by_name
        for B in (1, 7, P, T + 1):
            assert (f"r7_b{B}", f"{tag}_n{2 * T + 3}") in by_name
    # more than one block in a default-length case, and a remainder
    w = sc.wants("r7_bNone")["s16_n8192"]
    assert w["blocks"] == 3 and w["block_frames"] == 3001
    # a 32-bit sum cannot hold these
    w = sc.wants("r64_bNone")["s16_all_minus_full_scale"]
    assert w["ell"] == w["elr"] == 8195 << 30 and w["lag"] == 0 and w["flags"] & _capi.ST_DUAL_MONO
    w = sc.wants("r64_bNone")["s16_minus_against_plus_full_scale"]
    assert w["elr"] == -8195 * 32768 * 32767 and w["anti_lag"] == 0 and w["neg_blocks"] == 1
    # the floor shift, and raw opposites
    w = sc.wants("r7_b7")["s32_floor_shift"]
    assert w["ell"] == sum(int(v) ** 2 for v in (-1, -1, -1, -2, 0, 1, 32767, -32768, -32768, 0, -4661, 0))
    w = sc.wants("r7_b7")["s32_opposite_raw"]
    assert w["opposite_frames"] == 11 and w["equal_frames"] == 1 and w["frames"] == 12 and not w["flags"] & _capi.ST_INVERTED_COPY
    # floats: +-1 and beyond are +32767 / -32768; halves go to even; NaN never equals; the zeros are equal whatever their sign
    w = sc.wants("r7_b7")["f32_signed_zeros"]
    assert w["equal_frames"] == 4 and w["zero_frames"] == 4 and w["opposite_frames"] == 1
    w = sc.wants("r7_b7")["f32_nan_against_itself"]
    assert (w["equal_frames"], w["nonfinite"], w["ell"]) == (0, 18, 0) and w["flags"] & _capi.ST_SILENT
    for where in ("first", "middle", "last"):
        assert sc.wants("r7_b7")[f"f32_nonfinite_{where}_one"]["nonfinite"] == 1 and sc.wants("r7_b7")[f"f32_nonfinite_{where}_both"]["nonfinite"] == 2
    q, _ = sc.quantise(np.array([1.0, -1.0, 1.5, -1e30, 1 / 65536, 3 / 65536, -1 / 65536, 5 / 65536, 32767.5 / 32768, 32766.5 / 32768], np.float32))
    assert list(q) == [32767, -32768, 32767, -32768, 0, 2, 0, 2, 32767, 32766]


@pytest.mark.parametrize("name", ["r64_bNone", "r7_b7"])
def test_known_verdicts(name):
    group = next(g for g in sc.groups() if g.name == name)
    recs, sums = _run(0, group)
    by = {tr.name: (tr, r) for tr, r in zip(group.tracks, recs)}
    ST = _capi
    for tag in ("s16", "s32", "f32"):
        _, r = by[f"{tag}_dual_mono"]
        assert r.flags == ST.ST_COMPLETE | ST.ST_DUAL_MONO and r.correlation == pytest.approx(1.0, abs=1e-12) and r.side_db == -math.inf and r.balance_db == 0.0
        assert r.lag == 0 and r.mono_blocks == r.active_blocks == r.blocks and r.equal_frames == r.frames
        _, r = by[f"{tag}_inverted"]
        assert r.flags == ST.ST_COMPLETE | ST.ST_INVERTED_COPY | ST.ST_OUT_OF_PHASE and r.correlation == pytest.approx(-1.0, abs=1e-12)
        assert r.side_db == math.inf and r.anti_lag == 0 and r.anti_sum == r.elr == -r.ell and r.neg_blocks > 0
        _, r = by[f"{tag}_left_only"]
        assert r.flags == ST.ST_COMPLETE | ST.ST_ONE_SIDED and r.balance_db == math.inf and r.correlation == 0.0 and r.side_db == 0.0
        _, r = by[f"{tag}_right_only"]
        assert r.flags == ST.ST_COMPLETE | ST.ST_ONE_SIDED and r.balance_db == -math.inf and r.lag == 0 and r.lag_sum == 0
        _, r = by[f"{tag}_silent"]
        assert r.flags == ST.ST_COMPLETE | ST.ST_SILENT | ST.ST_DUAL_MONO and (r.correlation, r.balance_db, r.side_db) == (0.0, 0.0, 0.0)
        _, r = by[f"{tag}_one_channel"]
        assert r.flags == ST.ST_COMPLETE | ST.ST_MONO and (r.frames, r.channels, r.blocks, r.ell, r.equal_frames) == (300, 1, 0, 0, 0)
        tr, r = by[f"{tag}_eight_channels"]
        two = sc.want_track(sc.Tr("", tr.channels[:2], tr.sample_rate), group.radius, group.block_frames)
        assert r.flags == two["flags"] | ST.ST_MORE_CHANNELS and (r.channels, r.ell, r.err, r.elr, r.lag) == (8, two["ell"], two["err"], two["elr"], two["lag"])
        _, r = by[f"{tag}_near_mono"]
        assert r.flags == ST.ST_COMPLETE | ST.ST_NEAR_MONO and r.equal_frames == r.frames - 1 and r.side_db < -40.0
        assert (by[f"{tag}_tie_sign"][1].lag, by[f"{tag}_tie_abs"][1].lag) == (-1, 1)
        assert (by[f"{tag}_tie_anti_sign"][1].anti_lag, by[f"{tag}_tie_anti_abs"][1].anti_lag) == (-1, 1)
        assert by[f"{tag}_tie_sign"][1].lag_sum == by[f"{tag}_tie_abs"][1].lag_sum == 81 and by[f"{tag}_tie_anti_abs"][1].anti_sum == -81


@pytest.mark.parametrize("name", ["r255_bNone", "r64_bNone"])
def test_a_delayed_copy_reads_its_delay(name):
    group = next(g for g in sc.groups() if g.name == name)
    recs, _ = _run(0, group)
    seen = 0
    for tr, r in zip(group.tracks, recs):
        if "_delay" not in tr.name:
            continue
        d = int(tr.name.split("_delay")[1])
        ql, _ = sc.quantise(tr.channels[0])
        n = len(ql)
        overlap = ql[max(0, -d):n - max(0, d)]
        assert (r.lag, r.lag_sum) == (d, int(np.dot(overlap, overlap))), tr.name
        assert r.flags & _capi.ST_DELAYED and r.lag_correlation > 0.9 and abs(r.correlation) < 0.2, tr.name
        seen += 1
    assert seen == 3 * (len(sc.DELAYS) if group.radius == 255 else 7)


def test_options_and_refusals():
    arena = np.zeros(64, dtype=np.uint8)
    ok = _capi.TrackDesc(0, 4, 44100, 2, S16)
    for route in (0, 2):
        for desc, opts, code, text in ((_capi.TrackDesc(0, 17, 44100, 2, S16), {}, RG_ERR_INVALID_ARG, "beyond the arena"),
                                       (_capi.TrackDesc(1, 4, 44100, 2, S16), {}, RG_ERR_INVALID_ARG, "sample-aligned"),
                                       (_capi.TrackDesc(2, 4, 44100, 2, S32), {}, RG_ERR_INVALID_ARG, "sample-aligned"),
                                       (_capi.TrackDesc(0, 1, 44100, 9, S16), {}, RG_ERR_FORMAT, "9 channel"),
                                       (_capi.TrackDesc(0, 1, 44100, 0, S16), {}, RG_ERR_FORMAT, "0 channel"),
                                       (_capi.TrackDesc(0, 1, 44100, 2, 7), {}, RG_ERR_FORMAT, "format 7"),
                                       (ok, {"radius": 256}, RG_ERR_INVALID_ARG, "radius 256"),
                                       (ok, {"block_frames": sc.MAX_BLOCK + 1}, RG_ERR_INVALID_ARG, "block_frames"),
                                       (ok, {"phase_permille": 0}, RG_ERR_INVALID_ARG, "phase_permille"),
                                       (ok, {"delay_permille": 1001}, RG_ERR_INVALID_ARG, "delay_permille"),
                                       (ok, {"mono_db": 0}, RG_ERR_INVALID_ARG, "mono_db"),
                                       (ok, {"balance_db_limit": 1001}, RG_ERR_INVALID_ARG, "balance_db_limit"),
                                       (_capi.TrackDesc(0, 4, 0, 2, S16), {}, RG_ERR_INVALID_ARG, "a block of 0 frames"),
                                       (_capi.TrackDesc(0, 4, 384001, 2, S16), {}, RG_ERR_INVALID_ARG, "a block of 384001 frames")):
            with pytest.raises(rg.ReplayGainError) as e:
                rg.stereo_arena(None, route, [desc], arena, **opts)
            assert e.value.code == code and text in str(e.value), (route, str(e.value))
        r = rg.stereo_arena(None, route, [_capi.TrackDesc(0, 4, 384000, 8, S16)], arena)[0]
        assert (r.status, r.channels, r.block_frames, r.radius) == (0, 8, sc.MAX_BLOCK, 64)
        assert r.flags == _capi.ST_COMPLETE | _capi.ST_SILENT | _capi.ST_DUAL_MONO | _capi.ST_MORE_CHANNELS
        r, rows = rg.stereo_arena(None, route, [_capi.TrackDesc(0, 4, 0, 2, S16)], arena, radius=0, block_frames=3, lag_sums=True)
        assert (r[0].block_frames, r[0].radius, r[0].blocks, rows.shape) == (3, 0, 2, (1, 1))
        assert rg.stereo_arena(None, route, [], arena) == []
    with pytest.raises(rg.ReplayGainError) as e:
        rg.stereo_arena(None, 3, [ok], arena)
    assert e.value.code == RG_ERR_INVALID_ARG
    assert _capi.load().rg_stereo_arena(None, 1, 0, None, None, None, 0, None, None) == RG_ERR_INVALID_ARG  # the kernels need a context
    with pytest.raises(rg.ReplayGainError):
        rg.stereo_kernel_shape(3)
    assert C.sizeof(_capi.StereoRecord) == 176 and C.sizeof(_capi.StereoOpts) == 24


def test_thresholds_move_the_flags_and_records_become_objects():
    rng = np.random.default_rng(5)
    x = rng.integers(-20000, 20000, size=500).astype(np.int16)
    y = (x // 8).astype(np.int16)  # 18 dB down
    arena = np.concatenate([x, y]).view(np.uint8)
    d = [_capi.TrackDesc(0, 500, 44100, 2, S16)]
    r = rg.stereo_arena(None, 0, d, arena)[0]
    assert r.flags == _capi.ST_COMPLETE | _capi.ST_ONE_SIDED and 17.9 < r.balance_db < 18.2
    assert rg.stereo_arena(None, 0, d, arena, balance_db_limit=19)[0].flags == _capi.ST_COMPLETE
    assert rg.stereo_arena(None, 0, d, arena, mono_db=1)[0].flags == _capi.ST_COMPLETE | _capi.ST_ONE_SIDED | _capi.ST_NEAR_MONO
    s = rg.stereo_from_record(r)
    assert (s.frames, s.channels, s.radius, s.block_frames, s.ell, s.lag) == (500, 2, 64, 44100, r.ell, 0) and s.complete and s.error is None
    assert s.verdicts == ["one-sided"] and s.balance_db == r.balance_db
    late = np.concatenate([x, sc.delayed(x, 3)]).view(np.uint8)
    assert rg.stereo_from_record(rg.stereo_arena(None, 2, d, late)[0]).verdicts == ["delayed"]
    assert rg.stereo_from_record(rg.stereo_arena(None, 2, d, late, delay_permille=1000)[0]).verdicts == ["stereo"]
