"""The lossy ancestry scan on the GPU (include/mp3rgain_amd_ancestry.h): the kernels through their seam (rg_ancestry_arena,
route 1) on the shared cases (tests/ancestry_cases.py), byte for byte against the serial host twin (route 0), which
tests/test_ancestry_cpu.py holds to the float64 reference: the records and the raw counts of every view and alignment, in the
arena layouts every PCM-reading kernel is held to.  No tolerance anywhere: the counts are integers and the arithmetic in front
of them is the same chains of fused multiply-adds on both sides."""
import sys
from collections import namedtuple
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import ancestry_cases as ac  # noqa: E402
import arena_layouts as al  # noqa: E402

from mp3rgain_amd import _capi  # noqa: E402

pytestmark = pytest.mark.gpu

RG_ERR_INVALID_ARG, RG_ERR_FORMAT = -1, -9
Tr = namedtuple("Tr", "channels sample_rate")


def _raw(recs):
    return b"".join(bytes(r) for r in recs)


def _groups():
    """The cases by the options of their call: one launch per group."""
    by = {}
    for c in ac.cases():
        by.setdefault((c.segments, c.granules), []).append(c)
    return sorted(by.items())


def _first_difference(cases, dev, host, dcnt, hcnt):
    for i, c in enumerate(cases):
        if bytes(dev[i]) != bytes(host[i]) or not np.array_equal(dcnt[i], hcnt[i]):
            where = np.argwhere(dcnt[i] != hcnt[i])
            return c.name, dev[i].flags, host[i].flags, dev[i].grid_offset, host[i].grid_offset, where[:4].tolist()
    return None


@pytest.mark.parametrize("opts,cases", _groups(), ids=lambda v: f"s{v[0]}_g{v[1]}" if isinstance(v, tuple) else None)
def test_kernels_match_the_host_twin_on_every_case(_ctx, opts, cases):
    """Every case of a group, all three formats in one launch, between loud guards at odd sample offsets: route 1 == route 0 byte
    for byte, counts included; the same call twice gives the same bytes."""
    arena, descs, guards = al.pack([Tr(list(c.channels), c.sample_rate) for c in cases], al.Layout("guard", "loud", "input", 3))
    descs = list(descs)[:len(cases)]
    assert guards
    dev, dcnt = _ctx.ancestry_arena(1, descs, arena, *opts)
    host, hcnt = _ctx.ancestry_arena(0, descs, arena, *opts)
    assert _raw(dev) == _raw(host) and np.array_equal(dcnt, hcnt), _first_difference(cases, dev, host, dcnt, hcnt)
    again, acnt = _ctx.ancestry_arena(1, descs, arena, *opts)
    assert _raw(again) == _raw(dev) and np.array_equal(acnt, dcnt)
    for c, r in zip(cases, dev):
        if c.kind == "found":
            assert r.flags & _capi.ANC_MP3_GRID and r.grid_offset == c.offset, c.name
        elif c.kind in ("miss", "clean"):
            assert not r.flags & _capi.ANC_MP3_GRID, c.name


LAYOUTS = [al.Layout("abut", "loud", "input"), al.Layout("abut", "loud", "reversed"), al.Layout("guard", "nan", "reversed", 1)] + \
          [al.Layout("guard", "loud", "input", s) for s in (0, 2, 4, 5, 6)]


@pytest.mark.parametrize("layout", LAYOUTS, ids=lambda l: f"{l.gap}-{l.guard}-{l.order}-{l.shift}")
def test_kernels_in_every_layout(_ctx, layout):
    """Every residue of the planes' offsets, abutting tracks, tracks stored back to front: what lies around a plane (other
    tracks, full-scale or NaN guards) reaches no count -- the history before frame 0 and the granules past N - 1 read zeros --
    and rewriting the guards changes no byte."""
    cases = [c for c in ac.cases() if c.kind == "shape" and (c.segments, c.granules) == (2, 1)] + \
            [c for c in ac.cases() if c.name in ("shape_g1_s1_n1728", "shape_g1_s1_n1727", "shape_2ch_f32", "shape_2ch_s32")]
    assert len(cases) >= 6
    for opts in ((2, 1), (1, 1)):
        arena, descs, guards = al.pack([Tr(list(c.channels), c.sample_rate) for c in cases], layout)
        descs = list(descs)[:len(cases)]
        dev, dcnt = _ctx.ancestry_arena(1, descs, arena, *opts)
        host, hcnt = _ctx.ancestry_arena(0, descs, arena, *opts)
        assert _raw(dev) == _raw(host) and np.array_equal(dcnt, hcnt), (opts, _first_difference(cases, dev, host, dcnt, hcnt))
        if guards:
            other = arena.copy()
            for a, b in guards:
                other[a:b] ^= 0x5A
            again, acnt = _ctx.ancestry_arena(1, descs, other, *opts)
            assert _raw(again) == _raw(dev) and np.array_equal(acnt, dcnt), opts


def test_the_floor_and_the_thresholds_are_options_of_the_kernels_too(_ctx):
    case = next(c for c in ac.cases() if c.name == "cut_medium_k2000")
    arena, descs = ac.pack_one(case)
    for kw in (dict(active_floor=50.0), dict(z_min=1000.0), dict(iso_min=1.0, z_min=1.0), dict(segments=0)):
        o = dict(segments=3, granules=3)
        o.update(kw)
        dev, dcnt = _ctx.ancestry_arena(1, descs, arena, **o)
        host, hcnt = _ctx.ancestry_arena(0, descs, arena, **o)
        assert _raw(dev) == _raw(host) and np.array_equal(dcnt, hcnt), kw
    assert not _ctx.ancestry_arena(1, descs, arena, 3, 3, z_min=1000.0)[0][0].flags & _capi.ANC_MP3_GRID


def test_kernels_refuse_what_the_host_routes_refuse(_ctx):
    import mp3rgain_amd as rg

    arena = np.zeros(64, dtype=np.uint8)
    S16 = _capi.FMT_S16_PLANAR
    ok = _capi.TrackDesc(0, 4, 44100, 2, S16)
    for desc, opts, code, text in ((_capi.TrackDesc(0, 17, 44100, 2, S16), {}, RG_ERR_INVALID_ARG, "beyond the arena"),
                                   (_capi.TrackDesc(1, 4, 44100, 2, S16), {}, RG_ERR_INVALID_ARG, "sample-aligned"),
                                   (_capi.TrackDesc(0, 1, 44100, 9, S16), {}, RG_ERR_FORMAT, "9 channel"),
                                   (ok, dict(segments=1, granules=0), RG_ERR_INVALID_ARG, "granules"),
                                   (ok, dict(z_min=-1.0), RG_ERR_INVALID_ARG, "z_min")):
        texts = []
        for route in (1, 0):
            with pytest.raises(rg.ReplayGainError) as e:
                _ctx.ancestry_arena(route, [desc], arena, **opts)
            assert e.value.code == code and text in str(e.value)
            texts.append(str(e.value))
        assert texts[0] == texts[1]
    r = _ctx.ancestry_arena(1, [_capi.TrackDesc(0, 4, 44100, 8, S16)], arena)[0][0]
    assert (r.status, r.channels, r.views, r.flags) == (0, 8, 8, _capi.ANC_COMPLETE | _capi.ANC_SHORT | _capi.ANC_SILENT)
    assert _ctx.ancestry_arena(1, [], arena)[0] == []
