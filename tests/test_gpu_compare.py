"""The null test of two tracks on the GPU (include/mp3rgain_amd_compare.h): the kernels through their seam (rg_compare_arena, route
1) on the shared cases (tests/compare_cases.py), byte for byte against the serial host twin (route 0) -- records, lag rows and
block rows -- which tests/test_compare_cpu.py holds to the numpy / Python-int restatement, in the arena layouts every PCM-reading
kernel is held to.  One call per set of options; no tolerance anywhere in front of the finish, and that is host code on every
route."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import arena_layouts as al  # noqa: E402
import compare_cases as cc  # noqa: E402

from mp3rgain_amd import _capi  # noqa: E402

pytestmark = pytest.mark.gpu

RG_ERR_INVALID_ARG, RG_ERR_FORMAT = -1, -9
MAX_BLOCKS = 1200


def _raw(recs):
    return b"".join(bytes(r) for r in recs)


def _raw_blocks(blocks):
    return b"".join(bytes(b) for per in blocks for b in per)


def _run(ctx, route, call, arena, descs):
    return ctx.compare_arena(route, descs, call.pairs, arena, blocks_per_pair=MAX_BLOCKS, lag_sums=True, **call.opts)


def _first_difference(dev, host):
    (d, db, dr), (h, hb, hr) = dev, host
    for i, (x, y) in enumerate(zip(d, h)):
        if bytes(x) != bytes(y):
            return "record", i, cc.differences(cc.got(x), cc.got(y))
        if dr[i].tobytes() != hr[i].tobytes():
            s, c, k = (int(v[0]) for v in np.nonzero(dr[i] != hr[i]))
            return "lag row", i, ("segment", s, "channel", c, "column", k, int(dr[i][s, c, k]), int(hr[i][s, c, k]))
        if _raw_blocks([db[i]]) != _raw_blocks([hb[i]]):
            k = next(k for k, (p, q) in enumerate(zip(db[i], hb[i])) if bytes(p) != bytes(q))
            return "block", i, k, {f: (getattr(db[i][k], f), getattr(hb[i][k], f)) for f in cc.BLOCK_FIELDS}
    return None


def _same(dev, host):
    return _raw(dev[0]) == _raw(host[0]) and dev[2].tobytes() == host[2].tobytes() and _raw_blocks(dev[1]) == _raw_blocks(host[1])


@pytest.mark.parametrize("call", cc.calls(), ids=lambda c: c.name)
def test_kernels_match_the_host_twin_on_every_case(_ctx, call):
    """Every pair of a call in one launch, between loud guards at odd alignments: route 1 == route 0 byte for byte, records, lag
    rows and block rows, and field for field the restatement; the same call twice gives the same bytes."""
    tracks, want = list(call.tracks), cc.wants(call.name)
    arena, descs, guards = al.pack(tracks, al.Layout("guard", "loud", "input", 3))
    descs = list(descs)[:len(tracks)]
    assert guards
    dev = _run(_ctx, 1, call, arena, descs)
    host = _run(_ctx, 0, call, arena, descs)
    assert _same(dev, host), _first_difference(dev, host)
    bad = [(i, cc.differences(cc.got(r), w)) for i, (r, w) in enumerate(zip(dev[0], want)) if cc.differences(cc.got(r), w)]
    assert not bad, f"{len(bad)} of {len(want)} records differ from the restatement: {bad[:3]}"
    again = _run(_ctx, 1, call, arena, descs)
    assert _same(again, dev)


LAYOUTS = [al.Layout("abut", "loud", "input"), al.Layout("abut", "loud", "reversed"), al.Layout("guard", "nan", "reversed", 1)] + \
          [al.Layout("guard", "loud", "input", s) for s in (0, 2, 4, 5, 6)]
LAYOUT_CALLS = tuple(c.name for c in cc.calls())  # the same cases: every radius, the segments, the blocks, the formats


@pytest.mark.parametrize("layout", LAYOUTS, ids=lambda l: f"{l.gap}-{l.guard}-{l.order}-{l.shift}")
def test_kernels_in_every_layout(_ctx, layout):
    """Every residue of the planes' offsets modulo 128, every residue of the two tracks' alignments against each other (the
    "residues" call moves b by -8 .. 8 samples in every format), abutting tracks, tracks stored back to front: what lies around
    a plane (other tracks, full-scale or NaN guards) reaches no record, no lag row and no block row, and rewriting the guards
    changes no byte."""
    for name in LAYOUT_CALLS:
        call = next(c for c in cc.calls() if c.name == name)
        arena, descs, guards = al.pack(list(call.tracks), layout)
        descs = list(descs)[:len(call.tracks)]
        dev = _run(_ctx, 1, call, arena, descs)
        host = _run(_ctx, 0, call, arena, descs)
        assert _same(dev, host), (name, _first_difference(dev, host))
        if guards:
            other = arena.copy()
            for a, b in guards:
                other[a:b] ^= 0x5A
            again = _run(_ctx, 1, call, other, descs)
            assert _same(again, dev), name


def test_kernels_refuse_what_the_host_routes_refuse(_ctx):
    import mp3rgain_amd as rg

    arena = np.zeros(64, dtype=np.uint8)
    S16 = _capi.FMT_S16_PLANAR
    ok = [_capi.TrackDesc(0, 4, 44100, 2, S16), _capi.TrackDesc(16, 4, 44100, 2, S16)]
    pair = [(0, 1, 0)]
    for descs, pairs, opts, code, text in (([_capi.TrackDesc(0, 17, 44100, 2, S16), ok[1]], pair, {}, RG_ERR_INVALID_ARG, "beyond the arena"),
                                           ([ok[0], _capi.TrackDesc(1, 4, 44100, 2, S16)], pair, {}, RG_ERR_INVALID_ARG, "sample-aligned"),
                                           ([ok[0], _capi.TrackDesc(0, 1, 44100, 9, S16)], pair, {}, RG_ERR_FORMAT, "9 channel"),
                                           (ok, [(1, 1, 0)], {}, RG_ERR_INVALID_ARG, "against itself"),
                                           (ok, [(0, 2, 0)], {}, RG_ERR_INVALID_ARG, "is not a pair"),
                                           (ok, pair, {"radius": 2048}, RG_ERR_INVALID_ARG, "radius 2048"),
                                           (ok, pair, {"segments": 17}, RG_ERR_INVALID_ARG, "segments 17"),
                                           (ok, pair, {"lock_permille": 0}, RG_ERR_INVALID_ARG, "lock_permille")):
        texts = []
        for route in (1, 0):
            with pytest.raises(rg.ReplayGainError) as e:
                _ctx.compare_arena(route, descs, pairs, arena, **opts)
            assert e.value.code == code and text in str(e.value)
            texts.append(str(e.value))
        assert texts[0] == texts[1]
    r = _ctx.compare_arena(1, ok, pair, arena)[0]
    assert (r.status, r.channels, r.block_frames, r.radius, r.overlap) == (0, 2, 44100, 1024, 4)
    assert r.flags == _capi.CMP_COMPLETE | _capi.CMP_IDENTICAL | _capi.CMP_UNRELATED | _capi.CMP_RAW
    assert _ctx.compare_arena(1, ok, [], arena) == []
