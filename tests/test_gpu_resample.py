"""The rational resampler on the GPU (include/mp3rgain_amd_resample.h): the kernels through their seams (rg_resample_arena and
rg_xrate_fingerprint_arena, route 1) byte for byte against the kernels' arithmetic on the host (route 2), which
tests/test_resample_cpu.py holds to the float64 reference: records and y on every shared case (tests/resample_cases.py), in the
arena layouts every PCM-reading kernel is held to, in one launch that mixes rates and formats, and on one track long enough
for j M to pass 2^32.  No tolerance anywhere."""
import sys
from collections import namedtuple
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import arena_layouts as al  # noqa: E402
import resample_cases as rc  # noqa: E402

from mp3rgain_amd import _capi  # noqa: E402

pytestmark = pytest.mark.gpu

RG_ERR_INVALID_ARG, RG_ERR_FORMAT = -1, -9
Tr = namedtuple("Tr", "channels sample_rate")


def _raw(recs):
    return b"".join(bytes(r) for r in recs)


def _first_difference(cases, dev, host):
    for c, d, h in zip(cases, dev[0], host[0]):
        if bytes(d) != bytes(h):
            return c.name, "record", {f: (getattr(d, f), getattr(h, f)) for f, _ in d._fields_ if getattr(d, f) != getattr(h, f)}
        a, b = dev[1][d.y_at:d.y_at + d.resampled], host[1][h.y_at:h.y_at + h.resampled]
        if a.tobytes() != b.tobytes():
            return c.name, "y", np.argwhere(a.view(np.uint32) != b.view(np.uint32))[:4].tolist()
    return None


def _same(dev, host):
    return _raw(dev[0]) == _raw(host[0]) and dev[1].tobytes() == host[1].tobytes()


def _tracks(cases):
    return [Tr(list(c.channels), c.sample_rate) for c in cases]


def test_kernels_match_their_host_arithmetic_on_every_case(_ctx):
    """Every shared case in one launch, abutting at sample alignment: route 1 == route 2 byte for byte, records and y; the same
    call twice gives the same bytes.  The last track's last window ends on the arena's last sample."""
    cases = rc.cases()
    arena, descs, _ = al.pack(_tracks(cases), al.Layout("abut", "loud", "input"))
    descs = list(descs)[:len(cases)]
    last = descs[-1]
    assert last.offset_bytes + last.frames * last.channels * 4 == arena.size and rc.m_of(last.frames, last.sample_rate) == 600
    dev = _ctx.resample_arena(1, descs, arena)
    host = _ctx.resample_arena(2, descs, arena)
    assert _same(dev, host), _first_difference(cases, dev, host)
    assert _same(_ctx.resample_arena(1, descs, arena), dev)
    recs = dev[0]
    assert {int(r.format) for r in recs} == {0, 1, 2} and {int(r.up) for r in recs if not r.flags & _capi.RS_RATE} == {1, 7, 147, 441}
    assert sum(1 for r in recs if r.flags & _capi.RS_RATE) == 2 and sum(1 for r in recs if r.flags & _capi.RS_SHORT) >= 6
    assert {255, 256, 257, 511} <= {int(r.resampled) for r in recs} and np.isnan(dev[1]).sum() > 10 and dev[1].size > 10000


LAYOUTS = [al.Layout("abut", "loud", "reversed"), al.Layout("guard", "nan", "reversed", 1)] + [al.Layout("guard", "loud", "input", s) for s in (0, 2, 3, 4, 5, 6)]


@pytest.mark.parametrize("layout", LAYOUTS, ids=lambda l: f"{l.gap}-{l.guard}-{l.order}-{l.shift}")
def test_kernels_in_every_layout(_ctx, layout):
    """Every residue of the planes' offsets, odd sample alignments, tracks stored back to front: what lies around a plane (other
    tracks, full-scale or NaN guards) reaches no y -- a read outside a plane would poison it -- and rewriting the guards changes
    no byte."""
    cases = rc.cases()
    arena, descs, guards = al.pack(_tracks(cases), layout)
    descs = list(descs)[:len(cases)]
    dev = _ctx.resample_arena(1, descs, arena)
    host = _ctx.resample_arena(2, descs, arena)
    assert _same(dev, host), _first_difference(cases, dev, host)
    if guards:
        other = arena.copy()
        for a, b in guards:
            other[a:b] ^= 0x5A
        assert _same(_ctx.resample_arena(1, descs, other), dev)


def test_a_batch_of_mixed_rates(_ctx):
    """One launch batch mixing 44100, 48000 and 8000 Hz in all three formats, with a zero-output track and a track at an
    unsupported rate between them: the run -> track lookup, the workgroups' starts and the per-rate table offsets, in the
    cross-rate seam, so the tile walk over y is held to its host twin too (records, codes, band energies, y)."""
    rng = np.random.default_rng(5)
    mk = lambda n, fmt, nch=1: [rc.fc.as_format(rc.fc.noise(n, int(rng.integers(1 << 30))), fmt) for _ in range(nch)]  # noqa: E731
    cases = [rc.Case("a48", mk(rc.n_for(5700, 48000), "s16", 2), 48000),
             rc.Case("zero48", mk(40, "f32"), 48000),
             rc.Case("a44", mk(rc.n_for(5000, 44100) + 1, "f32", 2), 44100),
             rc.Case("a8", mk(rc.n_for(4700, 8000), "s32"), 8000),
             rc.Case("bad", mk(6000, "s16"), 384000),
             rc.Case("b48", mk(rc.n_for(700, 48000), "s32", 2), 48000),
             rc.Case("b8", mk(rc.n_for(513, 8000), "s16", 2), 8000),
             rc.Case("b44", mk(rc.n_for(4608, 44100), "s16"), 44100),
             rc.Case("c8", mk(rc.n_for(300, 8000), "f32"), 8000)]
    arena, descs, _ = al.pack(_tracks(cases), al.Layout("guard", "nan", "input", 1))
    descs = list(descs)[:len(cases)]
    dev = _ctx.xrate_fingerprint_arena(1, descs, arena)
    host = _ctx.xrate_fingerprint_arena(2, descs, arena)
    assert _raw(dev[0]) == _raw(host[0]), [(c.name, f, getattr(d, f), getattr(h, f)) for c, d, h in zip(cases, dev[0], host[0]) for f, _ in d._fields_
                                            if getattr(d, f) != getattr(h, f)][:6]
    assert dev[3].tobytes() == host[3].tobytes() and dev[1].tobytes() == host[1].tobytes() and dev[2].tobytes() == host[2].tobytes()
    recs = dev[0]
    assert [int(r.resampled) for r in recs] == [5700, 0, 5000, 4700, 0, 700, 513, 4608, 300]
    assert [int(r.codes) for r in recs] == [3, 0, 1, 1, 0, 0, 0, 1, 0] and recs[4].flags & _capi.FP_RATE and not recs[1].flags & _capi.FP_RATE
    assert not np.isnan(dev[3]).any()


def test_beyond_two_to_the_32(_ctx):
    """One mono s16 track at 192 kHz of 29.5 M frames: 1.69 M outputs, so j M passes 2^32 in its last runs.  Route 1 == route 2."""
    n = 29_500_000
    x = (np.arange(n, dtype=np.int64) * 2654435761 >> 7).astype(np.int16)  # cheap, and no two windows alike
    arena, descs, _ = al.pack([Tr([x], 192000)], al.Layout("abut", "loud", "input"))
    descs = list(descs)[:1]
    dev = _ctx.resample_arena(1, descs, arena)
    host = _ctx.resample_arena(2, descs, arena)
    m = int(dev[0][0].resampled)
    assert m == rc.m_of(n, 192000) and (m - 1) * 2560 > 1 << 32
    assert _same(dev, host), int(np.argmax(dev[1].view(np.uint32) != host[1].view(np.uint32)))


def test_kernels_refuse_what_the_host_routes_refuse(_ctx):
    import mp3rgain_amd as rg

    arena = np.zeros(64, dtype=np.uint8)
    S16 = _capi.FMT_S16_PLANAR
    for desc, code, text in ((_capi.TrackDesc(0, 17, 48000, 2, S16), RG_ERR_INVALID_ARG, "beyond the arena"),
                             (_capi.TrackDesc(1, 4, 48000, 2, S16), RG_ERR_INVALID_ARG, "sample-aligned"),
                             (_capi.TrackDesc(0, 1, 48000, 9, S16), RG_ERR_FORMAT, "9 channel")):
        texts = []
        for route in (1, 2):
            with pytest.raises(rg.ReplayGainError) as e:
                _ctx.resample_arena(route, [desc], arena)
            assert e.value.code == code and text in str(e.value)
            texts.append(str(e.value))
        assert texts[0] == texts[1]
    r = _ctx.resample_arena(1, [_capi.TrackDesc(0, 4, 48000, 8, S16)], arena)[0][0]
    assert (r.status, r.channels, r.flags, r.up, r.down, r.taps) == (0, 8, _capi.RS_SHORT, 147, 640, 70)
    assert _ctx.resample_arena(1, [], arena)[0] == []
