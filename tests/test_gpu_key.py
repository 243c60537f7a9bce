"""The key scan on the GPU (include/mp3rgain_amd_key.h).  Stage 1 and the whole record: the kernels through their seam
(rg_key_arena, route 1) on the shared cases (tests/key_cases.py), byte for byte against the kernels' arithmetic on the host
(route 2), which tests/test_key_cpu.py holds to the float64 reference: records, the decimated signal, band energies and chroma
rows, in the arena layouts every PCM-reading kernel is held to.  Stage 2: the finish kernel (rg_key_from_chroma, route 1) byte
for byte against the serial host twin (route 0), which tests/test_key_stage2_cpu.py holds to the integer restatement.  No
tolerance anywhere."""
import sys
from collections import namedtuple
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import arena_layouts as al  # noqa: E402
import key_cases as kc  # noqa: E402

from mp3rgain_amd import _capi  # noqa: E402

pytestmark = pytest.mark.gpu

RG_ERR_INVALID_ARG, RG_ERR_FORMAT = -1, -9
Tr = namedtuple("Tr", "channels sample_rate")
NAMES = ("record", "decimated", "bands", "chroma")


def _raw(recs):
    return b"".join(bytes(r) for r in recs)


def _first_difference(cases, dev, host):
    ya = 0
    for c, d, h in zip(cases, dev[0], host[0]):
        if bytes(d) != bytes(h):
            return c.name, "record", {f: (getattr(d, f), getattr(h, f)) for f, _ in d._fields_ if getattr(d, f) != getattr(h, f)}
        a, b = dev[1][ya:ya + d.decimated], host[1][ya:ya + h.decimated]
        ya += d.decimated
        if a.tobytes() != b.tobytes():
            return c.name, "decimated", np.argwhere(a.view(np.uint32) != b.view(np.uint32))[:4].tolist()
        for which in (2, 3):
            if dev[which] is None:
                continue
            a, b = dev[which][d.chroma_at:d.chroma_at + d.rows], host[which][h.chroma_at:h.chroma_at + h.rows]
            if a.tobytes() != b.tobytes():
                return c.name, NAMES[which], np.argwhere(a != b)[:4].tolist()
    return None


def _same(dev, host):
    return _raw(dev[0]) == _raw(host[0]) and all(d.tobytes() == h.tobytes() for d, h in zip(dev[1:], host[1:]) if d is not None)


@pytest.mark.parametrize("segment", (None, 8), ids=("defaults", "s8"))
def test_kernels_match_their_host_arithmetic_on_every_case(_ctx, segment):
    """Every case, all three formats and four decimation factors in one launch, between loud guards at odd sample offsets:
    route 1 == route 2 byte for byte, the decimated signal, band energies and rows included; the same call twice gives the
    same bytes; without the band energies, the same rest."""
    cases = kc.cases()
    arena, descs, guards = al.pack([Tr(list(c.channels), c.sample_rate) for c in cases], al.Layout("guard", "loud", "input", 3))
    descs = list(descs)[:len(cases)]
    assert guards
    dev = _ctx.key_arena(1, descs, arena, segment=segment)
    host = _ctx.key_arena(2, descs, arena, segment=segment)
    assert _same(dev, host), _first_difference(cases, dev, host)
    again = _ctx.key_arena(1, descs, arena, segment=segment)
    assert _same(again, dev)
    lean = _ctx.key_arena(1, descs, arena, segment=segment, bands=False)
    assert lean[2] is None and _raw(lean[0]) == _raw(dev[0]) and lean[1].tobytes() == dev[1].tobytes() and lean[3].tobytes() == dev[3].tobytes()
    recs = dev[0]
    assert sum(int(r.rows) for r in recs) > 150 and any(r.flags & _capi.KEY_NONFINITE for r in recs) and any(r.flags & _capi.KEY_RATE for r in recs)
    assert {int(r.decim) for r in recs} == {0, 1, 8, 9, 38} and {int(r.format) for r in recs} == {0, 1, 2}
    assert any(r.flags & _capi.KEY_NONE for r in recs) and any(not r.flags & (_capi.KEY_NONE | _capi.KEY_SHORT) for r in recs)
    assert int(dev[3].max()) > 300 and dev[1].size > 100000
    if segment:
        assert any(r.segments > 1 and r.stable_permille for r in recs)


LAYOUTS = [al.Layout("abut", "loud", "input"), al.Layout("abut", "loud", "reversed"), al.Layout("guard", "nan", "reversed", 1)] + \
          [al.Layout("guard", "loud", "input", s) for s in (0, 2, 4, 5, 6)]


@pytest.mark.parametrize("layout", LAYOUTS, ids=lambda l: f"{l.gap}-{l.guard}-{l.order}-{l.shift}")
def test_kernels_in_every_layout(_ctx, layout):
    """Every residue of the planes' offsets, abutting tracks, tracks stored back to front: what lies around a plane (other
    tracks, full-scale or NaN guards) reaches no decimated sample, no band energy and no row, and rewriting the guards changes
    no byte."""
    cases = [c for c in kc.cases() if c.name != "chord_2s_s16_2ch"]
    arena, descs, guards = al.pack([Tr(list(c.channels), c.sample_rate) for c in cases], layout)
    descs = list(descs)[:len(cases)]
    dev = _ctx.key_arena(1, descs, arena, segment=8)
    host = _ctx.key_arena(2, descs, arena, segment=8)
    assert _same(dev, host), _first_difference(cases, dev, host)
    if guards:
        other = arena.copy()
        for a, b in guards:
            other[a:b] ^= 0x5A
        assert _same(_ctx.key_arena(1, descs, other, segment=8), dev)


def test_kernels_refuse_what_the_host_routes_refuse(_ctx):
    import mp3rgain_amd as rg

    arena = np.zeros(64, dtype=np.uint8)
    S16 = _capi.FMT_S16_PLANAR
    for desc, code, text in ((_capi.TrackDesc(0, 17, 44100, 2, S16), RG_ERR_INVALID_ARG, "beyond the arena"),
                             (_capi.TrackDesc(1, 4, 44100, 2, S16), RG_ERR_INVALID_ARG, "sample-aligned"),
                             (_capi.TrackDesc(0, 1, 44100, 9, S16), RG_ERR_FORMAT, "9 channel")):
        texts = []
        for route in (1, 2):
            with pytest.raises(rg.ReplayGainError) as e:
                _ctx.key_arena(route, [desc], arena)
            assert e.value.code == code and text in str(e.value)
            texts.append(str(e.value))
        assert texts[0] == texts[1]
    texts = []
    for route in (1, 2):
        with pytest.raises(rg.ReplayGainError) as e:
            _ctx.key_arena(route, [_capi.TrackDesc(0, 4, 44100, 2, S16)], arena, segment=7)
        assert e.value.code == RG_ERR_INVALID_ARG
        texts.append(str(e.value))
    assert texts[0] == texts[1] and "segment 7" in texts[0]
    r = _ctx.key_arena(1, [_capi.TrackDesc(0, 4, 44100, 8, S16)], arena)[0][0]
    assert (r.status, r.channels, r.flags, r.decim) == (0, 8, _capi.KEY_COMPLETE | _capi.KEY_SHORT, 8)
    assert _ctx.key_arena(1, [], arena)[0] == []


# ---- stage 2 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cc", kc.chroma_cases(), ids=lambda cc: cc.name)
def test_finish_kernel_equals_the_host_twin(_ctx, cc):
    host = _ctx.key_from_chroma(0, list(cc.rows), segment=cc.segment)
    for _ in range(2):
        dev = _ctx.key_from_chroma(1, list(cc.rows), segment=cc.segment)
        assert _raw(dev) == _raw(host), [(k, f, getattr(d, f), getattr(h, f)) for k, (d, h) in enumerate(zip(dev, host)) for f, _ in d._fields_
                                         if getattr(d, f) != getattr(h, f)][:6]


def test_finish_kernel_on_the_largest_sums(_ctx):
    """Rows of 800 and 799 over four segments of 4096: the largest H, sh > 0 in the track and in every segment."""
    rows = np.zeros((4096 * 4, 12), np.uint16)
    rows[:, 0] = 800
    rows[:, 7] = 799
    host = _ctx.key_from_chroma(0, [rows, kc.profile_rows(20, 5000, 77)], segment=4096)
    dev = _ctx.key_from_chroma(1, [rows, kc.profile_rows(20, 5000, 77)], segment=4096)
    assert _raw(dev) == _raw(host) and host[0].segments == 4 and host[1].key == 20
