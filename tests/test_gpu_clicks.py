"""The click scan on the GPU (include/mp3rgain_amd_clicks.h): the three kernels through their seam (rg_clicks_arena, route 1) on
the shared cases (tests/clicks_cases.py), byte for byte against the serial host twin (route 0), records and event lists, which
tests/test_clicks_cpu.py holds to the Python restatement, in the arena layouts every PCM-reading kernel is held to.  One launch
per group of cases (the options belong to the call); no tolerance anywhere."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import arena_layouts as al  # noqa: E402
import clicks_cases as cc  # noqa: E402

from mp3rgain_amd import _capi  # noqa: E402

pytestmark = pytest.mark.gpu

RG_ERR_INVALID_ARG, RG_ERR_FORMAT = -1, -9


def _raw(recs):
    return b"".join(bytes(r) for r in recs)


def _rows(rows, k, K):
    return rows[k * K:(k + 1) * K] if K else []


def _first_difference(tracks, a, b, ra, rb, K):
    for k, (tr, x, y) in enumerate(zip(tracks, a, b)):
        gx, gy = cc.got(x, _rows(ra, k, K)), cc.got(y, _rows(rb, k, K))
        if gx != gy:
            return tr.name, [(f, gx[f], gy[f]) for f in gx if gx[f] != gy[f]][:4]
    return None


@pytest.mark.parametrize("group", cc.groups(), ids=lambda g: g.name)
def test_kernels_match_the_host_twin_on_every_case(_ctx, group):
    """Every case of a group, all three formats in one launch, between loud guards at odd alignments: route 1 == route 0 byte for
    byte, records and event lists, and field for field the restatement; the same call twice gives the same bytes."""
    tracks, want, K = list(group.tracks), cc.wants(group.name), group.opts.max_events
    arena, descs, guards = al.pack(tracks, al.Layout("guard", "loud", "input", 3))
    descs = list(descs)[:len(tracks)]
    assert guards
    opts = group.opts._asdict()
    dev, drows = _ctx.clicks_arena(1, descs, arena, **opts)
    host, hrows = _ctx.clicks_arena(0, descs, arena, **opts)
    assert _raw(dev) == _raw(host) and bytes(drows) == bytes(hrows), _first_difference(tracks, dev, host, drows, hrows, K)
    bad = [(tr.name, d) for k, (tr, r) in enumerate(zip(tracks, dev)) for d in [cc.differences(cc.got(r, _rows(drows, k, K)), want[tr.name])] if d]
    assert not bad, f"{len(bad)} of {len(tracks)} records differ from the restatement: {bad[:3]}"
    again, arows = _ctx.clicks_arena(1, descs, arena, **opts)
    assert _raw(again) == _raw(dev) and bytes(arows) == bytes(drows)


LAYOUTS = [al.Layout("abut", "loud", "input"), al.Layout("abut", "loud", "reversed"), al.Layout("guard", "nan", "reversed", 1)] + \
          [al.Layout("guard", "loud", "input", s) for s in (0, 2, 4, 5, 6)]
SHORT_SAMPLES = 1400  # what a layout run keeps of a group


@pytest.mark.parametrize("layout", LAYOUTS, ids=lambda l: f"{l.gap}-{l.guard}-{l.order}-{l.shift}")
def test_kernels_in_every_layout(_ctx, layout):
    """Every residue of the planes' offsets modulo 128, abutting tracks, tracks stored back to front: what lies around a plane
    (other tracks, full-scale or NaN guards) reaches no record and no event, and rewriting the guards changes no byte."""
    ran = 0
    for g in cc.groups():
        tracks = [tr for tr in g.tracks if len(tr.channels[0]) <= SHORT_SAMPLES]
        if len(tracks) < 3:
            continue
        ran += 1
        arena, descs, guards = al.pack(tracks, layout)
        descs = list(descs)[:len(tracks)]
        opts = g.opts._asdict()
        dev, drows = _ctx.clicks_arena(1, descs, arena, **opts)
        host, hrows = _ctx.clicks_arena(0, descs, arena, **opts)
        assert _raw(dev) == _raw(host) and bytes(drows) == bytes(hrows), (g.name, _first_difference(tracks, dev, host, drows, hrows, g.opts.max_events))
        if guards:
            other = arena.copy()
            for a, b in guards:
                other[a:b] ^= 0x5A
            again, arows = _ctx.clicks_arena(1, descs, other, **opts)
            assert _raw(again) == _raw(dev) and bytes(arows) == bytes(drows), g.name
    assert ran >= 3


def test_kernels_refuse_what_the_host_routes_refuse(_ctx):
    import mp3rgain_amd as rg

    arena = np.zeros(64, dtype=np.uint8)
    S16 = _capi.FMT_S16_PLANAR
    ok = _capi.TrackDesc(0, 4, 44100, 2, S16)
    for desc, opts, code, text in ((_capi.TrackDesc(0, 17, 44100, 2, S16), {}, RG_ERR_INVALID_ARG, "beyond the arena"),
                                   (_capi.TrackDesc(1, 4, 44100, 2, S16), {}, RG_ERR_INVALID_ARG, "sample-aligned"),
                                   (_capi.TrackDesc(0, 1, 44100, 9, S16), {}, RG_ERR_FORMAT, "9 channel"),
                                   (_capi.TrackDesc(0, 1, 44100, 2, 7), {}, RG_ERR_FORMAT, "format 7"),
                                   (ok, {"block_samples": 1000}, RG_ERR_INVALID_ARG, "block_samples 1000"),
                                   (ok, {"order": 7}, RG_ERR_INVALID_ARG, "order 7"),
                                   (ok, {"ratio_permille": 999}, RG_ERR_INVALID_ARG, "ratio_permille 999"),
                                   (ok, {"floor": 0}, RG_ERR_INVALID_ARG, "floor 0"),
                                   (ok, {"gap": 256}, RG_ERR_INVALID_ARG, "gap 256"),
                                   (ok, {"max_width": 4096}, RG_ERR_INVALID_ARG, "max_width 4096")):
        texts = []
        for route in (1, 0):
            with pytest.raises(rg.ReplayGainError) as e:
                _ctx.clicks_arena(route, [desc], arena, **opts)
            assert e.value.code == code and text in str(e.value)
            texts.append(str(e.value))
        assert texts[0] == texts[1]
    recs, rows = _ctx.clicks_arena(1, [_capi.TrackDesc(0, 4, 44100, 8, S16)], arena)
    r = recs[0]
    assert (r.status, r.channels, r.block_samples, r.order, r.max_events) == (0, 8, 1024, 8, 16) and r.flags == _capi.CK_COMPLETE | _capi.CK_SILENT
    assert _raw(recs) == _raw(_ctx.clicks_arena(0, [_capi.TrackDesc(0, 4, 44100, 8, S16)], arena)[0])
    assert _ctx.clicks_arena(1, [], arena)[0] == []
