"""The PCM defect scan on the GPU (include/mp3rgain_amd_stats.h): the two kernels through their seam (rg_pcm_stats_arena, route 1)
on the shared cases (tests/pcm_stats_cases.py), byte for byte against the serial host twin (route 0), which tests/test_pcm_stats_cpu.py
holds to the numpy restatement, in the arena layouts every PCM-reading kernel is held to.  A handful of launches; no tolerance
anywhere."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import arena_layouts as al  # noqa: E402
import pcm_stats_cases as pc  # noqa: E402

from mp3rgain_amd import _capi  # noqa: E402

pytestmark = pytest.mark.gpu

RG_ERR_INVALID_ARG, RG_ERR_FORMAT = -1, -9


def _raw(recs):
    return b"".join(bytes(r) for r in recs)


def _first_difference(tracks, a, b):
    for tr, x, y in zip(tracks, a, b):
        if bytes(x) != bytes(y):
            return tr.name, pc.differences(pc.got(x), pc.got(y))
    return None


@pytest.mark.parametrize("opts", pc.OPTIONS, ids=lambda o: f"{o[0]}-{o[1]}")
def test_kernels_match_the_host_twin_on_every_case(_ctx, opts):
    """Every case of all three formats in one launch, between loud guards at odd alignments: route 1 == route 0 byte for byte,
    and field for field the numpy restatement; the same call twice gives the same bytes."""
    tracks, wants = pc.tracks(), pc.wants(opts)
    arena, descs, guards = al.pack(tracks, al.Layout("guard", "loud", "input", 3))
    descs = list(descs)[:len(tracks)]
    assert {d.format for d in descs} == {0, 1, 2} and guards
    dev = _ctx.pcm_stats_arena(1, descs, pc.bits_of(tracks), arena, *opts)
    host = _ctx.pcm_stats_arena(0, descs, pc.bits_of(tracks), arena, *opts)
    assert _raw(dev) == _raw(host), _first_difference(tracks, dev, host)
    bad = [(tr.name, pc.differences(pc.got(r), wants[tr.name])) for tr, r in zip(tracks, dev) if pc.differences(pc.got(r), wants[tr.name])]
    assert not bad, f"{len(bad)} of {len(tracks)} records differ from the restatement: {bad[:3]}"
    assert _raw(_ctx.pcm_stats_arena(1, descs, pc.bits_of(tracks), arena, *opts)) == _raw(dev)


def _short(tracks):
    c, t, f = pc.shape()
    return [tr for tr in tracks if len(tr.channels[0]) <= t + c + 3]


LAYOUTS = [al.Layout("abut", "loud", "input"), al.Layout("abut", "loud", "reversed"), al.Layout("guard", "nan", "reversed", 1)] + \
          [al.Layout("guard", "loud", "input", s) for s in (0, 2, 4, 5, 6)]


@pytest.mark.parametrize("layout", LAYOUTS, ids=lambda l: f"{l.gap}-{l.guard}-{l.order}-{l.shift}")
def test_kernels_in_every_layout(_ctx, layout):
    """Every residue of the planes' offsets modulo 128, abutting tracks, tracks stored back to front: what lies around a plane
    (other tracks, full-scale or NaN guards) reaches no record, and rewriting the guards changes no byte."""
    tracks = _short(pc.tracks())
    arena, descs, guards = al.pack(tracks, layout)
    descs = list(descs)[:len(tracks)]
    dev = _ctx.pcm_stats_arena(1, descs, pc.bits_of(tracks), arena)
    host = _ctx.pcm_stats_arena(0, descs, pc.bits_of(tracks), arena)
    assert _raw(dev) == _raw(host), _first_difference(tracks, dev, host)
    if guards:
        other = arena.copy()
        for a, b in guards:
            other[a:b] ^= 0x5A
        assert _raw(_ctx.pcm_stats_arena(1, descs, pc.bits_of(tracks), other)) == _raw(dev)


def test_kernels_on_aliased_tracks_with_other_bits(_ctx):
    """Descriptors that share one copy of their PCM and differ in `bits`: a 16-bit plane read as 8, 12 and 16 bits in one launch."""
    c, t, f = pc.shape()
    base = [tr for tr in pc.tracks() if tr.channels[0].dtype == np.int16 and len(tr.channels) == 1 and len(tr.channels[0]) in (c + 1, t + 1)]
    tracks = base * 3
    bits = [8] * len(base) + [12] * len(base) + [16] * len(base)
    arena, descs, _ = al.pack(tracks, al.Layout("guard", "loud", "aliased"))
    descs = list(descs)[:len(tracks)]
    assert all(descs[k].offset_bytes == descs[k % len(base)].offset_bytes for k in range(len(tracks)))
    dev = _ctx.pcm_stats_arena(1, descs, bits, arena, 1, 1)
    assert _raw(dev) == _raw(_ctx.pcm_stats_arena(0, descs, bits, arena, 1, 1))
    for tr, b, r in zip(tracks, bits, dev):
        assert not pc.differences(pc.got(r), pc.want_track(tr._replace(bits=b), 1, 1)), (tr.name, b)


def test_kernels_refuse_what_the_host_routes_refuse(_ctx):
    import mp3rgain_amd as rg

    arena = np.zeros(64, dtype=np.uint8)
    S16 = _capi.FMT_S16_PLANAR
    for desc, bits, code, text in ((_capi.TrackDesc(0, 17, 44100, 2, S16), 16, RG_ERR_INVALID_ARG, "beyond the arena"),
                                   (_capi.TrackDesc(1, 4, 44100, 2, S16), 16, RG_ERR_INVALID_ARG, "sample-aligned"),
                                   (_capi.TrackDesc(0, 4, 44100, 2, S16), 17, RG_ERR_INVALID_ARG, "17 bits"),
                                   (_capi.TrackDesc(0, 1, 44100, 9, S16), 16, RG_ERR_FORMAT, "9 channel")):
        with pytest.raises(rg.ReplayGainError) as e:
            _ctx.pcm_stats_arena(1, [desc], [bits], arena)
        assert e.value.code == code and text in str(e.value)
    with pytest.raises(rg.ReplayGainError) as e:
        _ctx.pcm_stats_arena(1, [_capi.TrackDesc(0, 4, 44100, 2, S16)], [16], arena, 0, 1)
    assert e.value.code == RG_ERR_INVALID_ARG
    r = _ctx.pcm_stats_arena(1, [_capi.TrackDesc(0, 4, 44100, 8, S16)], [16], arena)[0]
    assert (r.status, r.channels, r.lead_silence_frames, r.flags) == (0, 8, 4, _capi.STATS_SILENT | _capi.STATS_COMPLETE)
    assert _ctx.pcm_stats_arena(1, [], [], arena) == []
