"""The stereo image scan on the GPU (include/mp3rgain_amd_stereo.h): the three kernels through their seam (rg_stereo_arena, route
1) on the shared cases (tests/stereo_cases.py), byte for byte against the serial host twin (route 0), records and lag sums, which
tests/test_stereo_cpu.py holds to the numpy / Python-int restatement, in the arena layouts every PCM-reading kernel is held to.
One launch per group of cases (the radius and the block length are options of the call); no tolerance anywhere in front of the
finish, and that is host code on every route."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import arena_layouts as al  # noqa: E402
import stereo_cases as sc  # noqa: E402

from mp3rgain_amd import _capi  # noqa: E402

pytestmark = pytest.mark.gpu

RG_ERR_INVALID_ARG, RG_ERR_FORMAT = -1, -9


def _raw(recs):
    return b"".join(bytes(r) for r in recs)


def _first_difference(tracks, a, b, sa, sb):
    for tr, x, y, p, q in zip(tracks, a, b, sa, sb):
        if bytes(x) != bytes(y) or p.tobytes() != q.tobytes():
            lags = [int(k) - (len(p) // 2) for k in np.nonzero(p != q)[0][:5]]
            return tr.name, sc.differences(sc.got(x), sc.got(y)), "lags that differ", lags
    return None


@pytest.mark.parametrize("group", sc.groups(), ids=lambda g: g.name)
def test_kernels_match_the_host_twin_on_every_case(_ctx, group):
    """Every case of a group, all three formats in one launch, between loud guards at odd alignments: route 1 == route 0 byte for
    byte, records and lag sums, and field for field the restatement; the same call twice gives the same bytes."""
    tracks, want = list(group.tracks), sc.wants(group.name)
    arena, descs, guards = al.pack(tracks, al.Layout("guard", "loud", "input", 3))
    descs = list(descs)[:len(tracks)]
    assert guards
    opts = dict(radius=group.radius, block_frames=group.block_frames, lag_sums=True)
    dev, dsum = _ctx.stereo_arena(1, descs, arena, **opts)
    host, hsum = _ctx.stereo_arena(0, descs, arena, **opts)
    assert _raw(dev) == _raw(host) and dsum.tobytes() == hsum.tobytes(), _first_difference(tracks, dev, host, dsum, hsum)
    bad = [(tr.name, sc.differences(sc.got(r), want[tr.name])) for tr, r in zip(tracks, dev) if sc.differences(sc.got(r), want[tr.name])]
    assert not bad, f"{len(bad)} of {len(tracks)} records differ from the restatement: {bad[:3]}"
    again, asum = _ctx.stereo_arena(1, descs, arena, **opts)
    assert _raw(again) == _raw(dev) and asum.tobytes() == dsum.tobytes()


LAYOUTS = [al.Layout("abut", "loud", "input"), al.Layout("abut", "loud", "reversed"), al.Layout("guard", "nan", "reversed", 1)] + \
          [al.Layout("guard", "loud", "input", s) for s in (0, 2, 4, 5, 6)]
SHORT_GROUPS = ("r0_bNone", "r1_bNone", "r7_b1", "r7_b7", "r64_bNone", "r255_bNone")
SHORT_FRAMES = 1200  # what a layout run keeps of a group: the cases up to this length (N < R, R + 1, 2R + 1, the values, the structures)


@pytest.mark.parametrize("layout", LAYOUTS, ids=lambda l: f"{l.gap}-{l.guard}-{l.order}-{l.shift}")
def test_kernels_in_every_layout(_ctx, layout):
    """Every residue of the planes' offsets modulo 128 -- the two planes of a track of odd length have different ones modulo 16
    -- abutting tracks, tracks stored back to front: what lies around a plane (other tracks, full-scale or NaN guards) reaches no
    record and no lag sum, and rewriting the guards changes no byte."""
    for name in SHORT_GROUPS:
        g = next(g for g in sc.groups() if g.name == name)
        tracks = [tr for tr in g.tracks if len(tr.channels[0]) <= SHORT_FRAMES]
        assert len(tracks) >= 9
        arena, descs, guards = al.pack(tracks, layout)
        descs = list(descs)[:len(tracks)]
        opts = dict(radius=g.radius, block_frames=g.block_frames, lag_sums=True)
        dev, dsum = _ctx.stereo_arena(1, descs, arena, **opts)
        host, hsum = _ctx.stereo_arena(0, descs, arena, **opts)
        assert _raw(dev) == _raw(host) and dsum.tobytes() == hsum.tobytes(), (name, _first_difference(tracks, dev, host, dsum, hsum))
        if guards:
            other = arena.copy()
            for a, b in guards:
                other[a:b] ^= 0x5A
            again, asum = _ctx.stereo_arena(1, descs, other, **opts)
            assert _raw(again) == _raw(dev) and asum.tobytes() == dsum.tobytes(), name


def test_kernels_refuse_what_the_host_routes_refuse(_ctx):
    import mp3rgain_amd as rg

    arena = np.zeros(64, dtype=np.uint8)
    S16 = _capi.FMT_S16_PLANAR
    ok = _capi.TrackDesc(0, 4, 44100, 2, S16)
    for desc, opts, code, text in ((_capi.TrackDesc(0, 17, 44100, 2, S16), {}, RG_ERR_INVALID_ARG, "beyond the arena"),
                                   (_capi.TrackDesc(1, 4, 44100, 2, S16), {}, RG_ERR_INVALID_ARG, "sample-aligned"),
                                   (_capi.TrackDesc(0, 1, 44100, 9, S16), {}, RG_ERR_FORMAT, "9 channel"),
                                   (ok, {"radius": 256}, RG_ERR_INVALID_ARG, "radius 256"),
                                   (ok, {"block_frames": sc.MAX_BLOCK + 1}, RG_ERR_INVALID_ARG, "block_frames"),
                                   (ok, {"delay_permille": 0}, RG_ERR_INVALID_ARG, "delay_permille"),
                                   (ok, {"mono_db": 1001}, RG_ERR_INVALID_ARG, "mono_db"),
                                   (_capi.TrackDesc(0, 4, 384001, 2, S16), {}, RG_ERR_INVALID_ARG, "a block of 384001 frames")):
        texts = []
        for route in (1, 0):
            with pytest.raises(rg.ReplayGainError) as e:
                _ctx.stereo_arena(route, [desc], arena, **opts)
            assert e.value.code == code and text in str(e.value)
            texts.append(str(e.value))
        assert texts[0] == texts[1]
    r = _ctx.stereo_arena(1, [_capi.TrackDesc(0, 4, 44100, 8, S16)], arena)[0]
    assert (r.status, r.channels, r.block_frames, r.radius) == (0, 8, 44100, 64)
    assert r.flags == _capi.ST_COMPLETE | _capi.ST_SILENT | _capi.ST_DUAL_MONO | _capi.ST_MORE_CHANNELS
    assert _ctx.stereo_arena(1, [], arena) == []
