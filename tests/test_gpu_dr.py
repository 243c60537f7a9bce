"""The dynamic range figure on the GPU (include/mp3rgain_amd_dr.h): the two kernels through their seam (rg_dr_arena, route 1) on
the shared cases (tests/dr_cases.py), byte for byte against the serial host twin (route 0), which tests/test_dr_cpu.py holds to
the numpy / Python-int restatement, in the arena layouts every PCM-reading kernel is held to.  One launch per group of cases (the
block length is an option of the call); no tolerance anywhere in front of the logarithms, and those are host code on every
route."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import arena_layouts as al  # noqa: E402
import dr_cases as dc  # noqa: E402

from mp3rgain_amd import _capi  # noqa: E402

pytestmark = pytest.mark.gpu

RG_ERR_INVALID_ARG, RG_ERR_FORMAT = -1, -9


def _raw(recs):
    return b"".join(bytes(r) for r in recs)


def _first_difference(tracks, a, b):
    for tr, x, y in zip(tracks, a, b):
        if bytes(x) != bytes(y):
            return tr.name, dc.differences(dc.got(x), dc.got(y))
    return None


@pytest.mark.parametrize("group", dc.groups(), ids=lambda g: g.name)
def test_kernels_match_the_host_twin_on_every_case(_ctx, group):
    """Every case of a group, all three formats in one launch, between loud guards at odd alignments: route 1 == route 0 byte for
    byte, and field for field the restatement; the same call twice gives the same bytes."""
    tracks, want = list(group.tracks), dc.wants(group.name)
    arena, descs, guards = al.pack(tracks, al.Layout("guard", "loud", "input", 3))
    descs = list(descs)[:len(tracks)]
    assert guards
    opts = (group.block_frames, group.top_permille)
    dev = _ctx.dr_arena(1, descs, arena, *opts)
    host = _ctx.dr_arena(0, descs, arena, *opts)
    assert _raw(dev) == _raw(host), _first_difference(tracks, dev, host)
    bad = [(tr.name, dc.differences(dc.got(r), want[tr.name])) for tr, r in zip(tracks, dev) if dc.differences(dc.got(r), want[tr.name])]
    assert not bad, f"{len(bad)} of {len(tracks)} records differ from the restatement: {bad[:3]}"
    assert _raw(_ctx.dr_arena(1, descs, arena, *opts)) == _raw(dev)


def test_known_values_on_the_kernels(_ctx):
    g = next(g for g in dc.groups() if g.name == "bNone_pNone")
    tracks = list(g.tracks)
    arena, descs, _ = al.pack(tracks, al.Layout("guard", "loud", "input", 3))
    for tr, r in zip(tracks, _ctx.dr_arena(1, list(descs)[:len(tracks)], arena)):
        assert abs(r.dr_mean - dc.KNOWN[tr.name]) <= dc.KNOWN_TOL, (tr.name, r.dr_mean)


LAYOUTS = [al.Layout("abut", "loud", "input"), al.Layout("abut", "loud", "reversed"), al.Layout("guard", "nan", "reversed", 1)] + \
          [al.Layout("guard", "loud", "input", s) for s in (0, 2, 4, 5, 6)]
SHORT = [g for g in dc.groups() if g.short and (g.block_frames in (1, 7, 5) or g.block_frames in dc.shape(_capi.FMT_S16_PLANAR) + dc.shape(_capi.FMT_F32_PLANAR))]


@pytest.mark.parametrize("layout", LAYOUTS, ids=lambda l: f"{l.gap}-{l.guard}-{l.order}-{l.shift}")
def test_kernels_in_every_layout(_ctx, layout):
    """Every residue of the planes' offsets modulo 128, abutting tracks, tracks stored back to front: what lies around a plane
    (other tracks, full-scale or NaN guards) reaches no record, and rewriting the guards changes no byte."""
    assert len(SHORT) >= 6
    for g in SHORT:
        tracks = list(g.tracks)
        arena, descs, guards = al.pack(tracks, layout)
        descs = list(descs)[:len(tracks)]
        opts = (g.block_frames, g.top_permille)
        dev = _ctx.dr_arena(1, descs, arena, *opts)
        host = _ctx.dr_arena(0, descs, arena, *opts)
        assert _raw(dev) == _raw(host), (g.name, _first_difference(tracks, dev, host))
        if guards:
            other = arena.copy()
            for a, b in guards:
                other[a:b] ^= 0x5A
            assert _raw(_ctx.dr_arena(1, descs, other, *opts)) == _raw(dev), g.name


def test_kernels_refuse_what_the_host_routes_refuse(_ctx):
    import mp3rgain_amd as rg

    arena = np.zeros(64, dtype=np.uint8)
    S16 = _capi.FMT_S16_PLANAR
    ok = _capi.TrackDesc(0, 4, 44100, 2, S16)
    for desc, opts, code, text in ((_capi.TrackDesc(0, 17, 44100, 2, S16), (None, None), RG_ERR_INVALID_ARG, "beyond the arena"),
                                   (_capi.TrackDesc(1, 4, 44100, 2, S16), (None, None), RG_ERR_INVALID_ARG, "sample-aligned"),
                                   (_capi.TrackDesc(0, 1, 44100, 9, S16), (None, None), RG_ERR_FORMAT, "9 channel"),
                                   (ok, (None, 0), RG_ERR_INVALID_ARG, "top_permille"),
                                   (ok, (dc.MAX_BLOCK + 1, None), RG_ERR_INVALID_ARG, "block_frames"),
                                   (_capi.TrackDesc(0, 4, 384001, 2, S16), (None, None), RG_ERR_INVALID_ARG, "a block of 1152003 frames")):
        texts = []
        for route in (1, 0):
            with pytest.raises(rg.ReplayGainError) as e:
                _ctx.dr_arena(route, [desc], arena, *opts)
            assert e.value.code == code and text in str(e.value)
            texts.append(str(e.value))
        assert texts[0] == texts[1]
    r = _ctx.dr_arena(1, [_capi.TrackDesc(0, 4, 44100, 8, S16)], arena)[0]
    assert (r.status, r.channels, r.block_frames, r.flags) == (0, 8, 132300, _capi.DR_COMPLETE | _capi.DR_SILENT | _capi.DR_SHORT)
    assert _ctx.dr_arena(1, [], arena) == []
