"""The dynamic range figure on the host (include/mp3rgain_amd_dr.h): the serial twin (rg_dr_arena route 0) and the kernels' cutting
and fold arithmetic (route 2) on the shared cases (tests/dr_cases.py), byte for byte against each other and field for field
against the numpy / Python-int restatement: exactly in front of the logarithms, 1e-12 relative behind them.  No GPU."""
import ctypes as C
import math
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import arena_layouts as al  # noqa: E402
import dr_cases as dc  # noqa: E402

import mp3rgain_amd as rg  # noqa: E402
from mp3rgain_amd import _capi  # noqa: E402

RG_ERR_INVALID_ARG, RG_ERR_FORMAT = -1, -9
S16, S32, F32 = _capi.FMT_S16_PLANAR, _capi.FMT_S32_PLANAR, _capi.FMT_F32_PLANAR


def _raw(recs):
    return b"".join(bytes(r) for r in recs)


@pytest.mark.parametrize("group", dc.groups(), ids=lambda g: g.name)
def test_host_routes_match_each_other_and_the_restatement(group):
    tracks, want = list(group.tracks), dc.wants(group.name)
    arena, descs, _ = al.pack(tracks, al.Layout("guard", "loud", "input", 3))
    descs = list(descs)[:len(tracks)]
    serial = rg.dr_arena(None, 0, descs, arena, group.block_frames, group.top_permille)
    folded = rg.dr_arena(None, 2, descs, arena, group.block_frames, group.top_permille)
    bad = [(tr.name, dc.differences(dc.got(r), want[tr.name])) for tr, r in zip(tracks, serial) if dc.differences(dc.got(r), want[tr.name])]
    assert not bad, f"{len(bad)} of {len(tracks)} records of the serial twin differ from the restatement: {bad[:3]}"
    diff = [(tr.name, dc.differences(dc.got(a), dc.got(b))) for tr, a, b in zip(tracks, folded, serial) if bytes(a) != bytes(b)]
    assert _raw(folded) == _raw(serial), diff[:3]


def test_the_case_list_covers_what_it_claims():
    names = {tr.name: (g, tr) for g in dc.groups() for tr in g.tracks}
    assert {tr.channels[0].dtype for _, tr in names.values()} == {np.dtype(np.int16), np.dtype(np.int32), np.dtype(np.float32)}
    assert {len(tr.channels) for _, tr in names.values()} >= {1, 2, 6, 8}
    c, t = dc.shape(S16)
    assert (c, t) == (16 // 2, t) and t % c == 0 and dc.shape(S32) == dc.shape(F32) == (16 // 4, t // 2)
    for n in (0, 1, c - 1, c, c + 1, t - 1, t, t + 1, 2 * t + 3):
        for b in {1, 7, c, t, t + 1, n, n + 1} - {0}:
            assert f"s16_n{n}_b{b}" in names
    # a last block of one sample that holds the plane's peak
    g, tr = names[f"s16_n{t + 1}_b{t}"]
    w = dc.wants(g.name)[tr.name]["ch"][0]
    assert w["blocks"] == 2 and w["peak"] == 32768 and w["peak2"] < 32768
    # k at 200 per mille
    for blocks, k in ((1, 1), (4, 1), (5, 1), (9, 1), (10, 2)):
        assert dc.wants("b7_pNone")[f"s16_blocks{blocks}"]["ch"][0]["top_blocks"] == k
        assert dc.wants("b7_p1")[f"s16_blocks{blocks}"]["ch"][0]["top_blocks"] == 1
        assert dc.wants("b7_p1000")[f"s16_blocks{blocks}"]["ch"][0]["top_blocks"] == blocks
    # the tie: the two largest of [5, 3, 3, 3, 1] are 5 and one 3
    w = dc.wants("b5_p400")["s16_ladder"]["ch"][0]
    assert w["top_blocks"] == 2 and w["top_ms"] == (2.0 * 5 / (5 * 2.0 ** 30) + 2.0 * 3 / (5 * 2.0 ** 30)) / 2
    # more blocks than the selection has counters, 2^64 passed, both peaks
    assert dc.wants("b3_pNone")["s16_many_blocks"]["ch"][0]["blocks"] > 4 * rg.dr_kernel_shape(S16)[3]
    assert dc.wants("b8_pNone")["s32_int_min_blocks_of_8"]["ch"][0]["top_ms"] == 2.0
    assert dc.wants("b7_pNone")["s16_peak_twice"]["ch"][0]["peak2"] == 9 and dc.wants("b7_pNone")["s16_peak_once"]["ch"][0]["peak2"] == 5
    assert dc.wants("b7_pNone")["s16_minus_full_scale_alone"]["ch"][0]["peak"] == 32768
    assert dc.wants("b7_pNone")["f32_at_256_and_beyond"]["ch"][0]["peak"] == 1 << 31


def test_known_values():
    """A full-scale 997 Hz sine reads 0 dB and a full-scale square wave -3.01 dB; a sine at a tenth of full scale with single
    full-scale samples in two different blocks reads 19.99 dB, with one such sample 0.00 dB (the second-highest block peak)."""
    g = next(g for g in dc.groups() if g.name == "bNone_pNone")
    tracks = list(g.tracks)
    arena, descs, _ = al.pack(tracks, al.Layout("guard", "loud", "input", 3))
    recs = rg.dr_arena(None, 0, list(descs)[:len(tracks)], arena)
    for tr, r in zip(tracks, recs):
        print(tr.name, r.dr, r.dr_mean, r.peak_db, r.rms_db)
        assert abs(r.dr_mean - dc.KNOWN[tr.name]) <= dc.KNOWN_TOL, (tr.name, r.dr_mean)
        assert r.block_frames == 132300 and r.flags == _capi.DR_COMPLETE
    assert recs[0].dr == 0 and recs[1].dr == -3 and recs[2].dr == 20 and recs[3].dr == 0


def test_flags_and_the_values_of_silence():
    x = np.zeros(10, np.int16)
    y = np.arange(10, dtype=np.int16)
    arena = np.concatenate([x, y]).view(np.uint8)
    r = rg.dr_arena(None, 0, [_capi.TrackDesc(0, 10, 44100, 2, S16)], arena, 4)[0]
    assert r.flags == _capi.DR_COMPLETE and r.ch[0].dr == 0.0 and r.ch[0].peak_db == -math.inf and r.ch[0].rms_db == -math.inf
    assert r.ch[1].dr != 0.0 and r.dr_mean == r.ch[1].dr / 2 and r.peak_db == r.ch[1].peak_db
    r = rg.dr_arena(None, 2, [_capi.TrackDesc(0, 10, 44100, 1, S16)], arena, 11)[0]
    assert r.flags == _capi.DR_COMPLETE | _capi.DR_SILENT | _capi.DR_SHORT and (r.dr, r.dr_mean, r.peak_db, r.rms_db) == (0, 0.0, -math.inf, -math.inf)
    r = rg.dr_arena(None, 0, [_capi.TrackDesc(0, 0, 44100, 2, S16)], arena)[0]
    assert r.flags == _capi.DR_COMPLETE | _capi.DR_SILENT | _capi.DR_SHORT and r.block_frames == 132300 and r.ch[0].blocks == 0
    f = np.array([0.5, np.nan, -0.25, 0.125], np.float32).view(np.uint8)
    r = rg.dr_arena(None, 0, [_capi.TrackDesc(0, 4, 44100, 1, F32)], f, 2)[0]
    assert r.flags == _capi.DR_COMPLETE | _capi.DR_NONFINITE and r.ch[0].nonfinite == 1 and r.ch[0].peak == 1 << 22


def test_options_and_refusals():
    arena = np.zeros(64, dtype=np.uint8)
    ok = _capi.TrackDesc(0, 4, 44100, 2, S16)
    for route in (0, 2):
        for desc, opts, code, text in ((_capi.TrackDesc(0, 17, 44100, 2, S16), (None, None), RG_ERR_INVALID_ARG, "beyond the arena"),
                                       (_capi.TrackDesc(1, 4, 44100, 2, S16), (None, None), RG_ERR_INVALID_ARG, "sample-aligned"),
                                       (_capi.TrackDesc(2, 4, 44100, 2, S32), (None, None), RG_ERR_INVALID_ARG, "sample-aligned"),
                                       (_capi.TrackDesc(0, 1, 44100, 9, S16), (None, None), RG_ERR_FORMAT, "9 channel"),
                                       (_capi.TrackDesc(0, 1, 44100, 0, S16), (None, None), RG_ERR_FORMAT, "0 channel"),
                                       (_capi.TrackDesc(0, 1, 44100, 1, 7), (None, None), RG_ERR_FORMAT, "format 7"),
                                       (ok, (None, 0), RG_ERR_INVALID_ARG, "top_permille"),
                                       (ok, (None, 1001), RG_ERR_INVALID_ARG, "top_permille"),
                                       (ok, (dc.MAX_BLOCK + 1, None), RG_ERR_INVALID_ARG, "block_frames"),
                                       (_capi.TrackDesc(0, 4, 0, 2, S16), (None, None), RG_ERR_INVALID_ARG, "a block of 0 frames"),
                                       (_capi.TrackDesc(0, 4, 384001, 2, S16), (None, None), RG_ERR_INVALID_ARG, "a block of 1152003 frames")):
            with pytest.raises(rg.ReplayGainError) as e:
                rg.dr_arena(None, route, [desc], arena, *opts)
            assert e.value.code == code and text in str(e.value), (route, str(e.value))
        r = rg.dr_arena(None, route, [_capi.TrackDesc(0, 4, 384000, 8, S16)], arena)[0]
        assert (r.status, r.channels, r.block_frames, r.flags) == (0, 8, dc.MAX_BLOCK, _capi.DR_COMPLETE | _capi.DR_SILENT | _capi.DR_SHORT)
        assert rg.dr_arena(None, route, [_capi.TrackDesc(0, 4, 0, 2, S16)], arena, 3)[0].block_frames == 3
        assert rg.dr_arena(None, route, [], arena) == []
    with pytest.raises(rg.ReplayGainError) as e:
        rg.dr_arena(None, 3, [ok], arena)
    assert e.value.code == RG_ERR_INVALID_ARG
    assert _capi.load().rg_dr_arena(None, 1, 0, None, None, None, 0, None) == RG_ERR_INVALID_ARG  # the kernels need a context
    with pytest.raises(rg.ReplayGainError):
        rg.dr_kernel_shape(3)
    assert C.sizeof(_capi.DrRecord) == 576 and C.sizeof(_capi.DrChannel) == 64


def test_records_and_album_dr():
    def rec(dr, flags=_capi.DR_COMPLETE, error=None):
        return rg.DynamicRange(1, 44100, S16, 0 if flags & _capi.DR_COMPLETE else 3, 132300, flags, dr, float(dr), -0.1, -12.0, [], error)

    assert rg.album_dr([rec(12), rec(13)]) == 12 and rg.album_dr([rec(13), rec(14)]) == 14  # half to even
    assert rg.album_dr([rec(8), rec(11), rec(12)]) == 10
    assert rg.album_dr([rec(8), rec(20, 0), rec(20, _capi.DR_COMPLETE, rg.ReplayGainError(-9, "x"))]) == 8
    assert rg.album_dr([]) is None and rg.album_dr([rec(20, 0)]) is None
    x = (np.arange(40, dtype=np.int16) * 800 - 16000)
    r = rg.dr_arena(None, 0, [_capi.TrackDesc(0, 20, 44100, 2, S16)], x.view(np.uint8), 8)[0]
    d = rg.dynamic_range_from_record(r)
    assert (d.frames, d.sample_rate, d.format, d.block_frames, d.dr, d.dr_mean) == (20, 44100, S16, 8, r.dr, r.dr_mean)
    assert len(d.channels) == 2 and d.channels[1].peak == r.ch[1].peak and d.channels[0].top_blocks == 1 and d.channels[0].blocks == 3
    assert d.complete and not d.silent and not d.short and not d.nonfinite and d.verdicts == ["ok"] and d.error is None
    short = rg.dynamic_range_from_record(rg.dr_arena(None, 0, [_capi.TrackDesc(0, 20, 44100, 2, S16)], x.view(np.uint8), 21)[0])
    assert short.short and short.verdicts == ["short"]
