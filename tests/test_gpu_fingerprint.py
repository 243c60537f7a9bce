"""The duplicate finder on the GPU (include/mp3rgain_amd_fingerprint.h).  Stage 1: the kernels through their seam
(rg_fingerprint_arena, route 1) on the shared cases (tests/fingerprint_cases.py), byte for byte against the kernels'
arithmetic on the host (route 2), which tests/test_fingerprint_cpu.py holds to the float64 reference: records, codes and band
energies, in the arena layouts every PCM-reading kernel is held to.  Stage 2: the match kernel (rg_fingerprint_match_codes,
route 1) byte for byte against the serial host twin (route 0), which tests/test_fingerprint_match_cpu.py holds to the numpy
restatement.  No tolerance anywhere."""
import sys
from collections import namedtuple
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import arena_layouts as al  # noqa: E402
import fingerprint_cases as fc  # noqa: E402

from mp3rgain_amd import _capi  # noqa: E402

pytestmark = pytest.mark.gpu

RG_ERR_INVALID_ARG, RG_ERR_FORMAT = -1, -9
Tr = namedtuple("Tr", "channels sample_rate")


def _raw(recs):
    return b"".join(bytes(r) for r in recs)


def _first_difference(cases, dev, host):
    (drec, dcodes, dbands), (hrec, hcodes, hbands) = dev, host
    for c, d, h in zip(cases, drec, hrec):
        if bytes(d) != bytes(h):
            return c.name, "record", d.flags, h.flags, d.nonfinite_frames, h.nonfinite_frames
        a, b = dcodes[d.codes_at:d.codes_at + d.codes], hcodes[h.codes_at:h.codes_at + h.codes]
        if not np.array_equal(a, b):
            return c.name, "codes", np.argwhere(a != b)[:4].tolist()
        a, b = dbands[d.frames_at:d.frames_at + d.fp_frames], hbands[h.frames_at:h.frames_at + h.fp_frames]
        if a.tobytes() != b.tobytes():
            return c.name, "bands", np.argwhere(a.view(np.uint32) != b.view(np.uint32))[:4].tolist()
    return None


def _same(dev, host):
    return _raw(dev[0]) == _raw(host[0]) and dev[1].tobytes() == host[1].tobytes() and dev[2].tobytes() == host[2].tobytes()


def test_kernels_match_their_host_arithmetic_on_every_case(_ctx):
    """Every case, all three formats in one launch, between loud guards at odd sample offsets: route 1 == route 2 byte for
    byte, codes and band energies included; the same call twice gives the same bytes; without the band energies, the same codes."""
    cases = fc.cases()
    arena, descs, guards = al.pack([Tr(list(c.channels), c.sample_rate) for c in cases], al.Layout("guard", "loud", "input", 3))
    descs = list(descs)[:len(cases)]
    assert guards
    dev = _ctx.fingerprint_arena(1, descs, arena)
    host = _ctx.fingerprint_arena(2, descs, arena)
    assert _same(dev, host), _first_difference(cases, dev, host)
    again = _ctx.fingerprint_arena(1, descs, arena)
    assert _same(again, dev)
    lean = _ctx.fingerprint_arena(1, descs, arena, bands=False)
    assert _raw(lean[0]) == _raw(dev[0]) and lean[1].tobytes() == dev[1].tobytes() and lean[2] is None
    assert sum(int(r.codes) for r in dev[0]) > 300 and any(r.flags & _capi.FP_NONFINITE for r in dev[0])


LAYOUTS = [al.Layout("abut", "loud", "input"), al.Layout("abut", "loud", "reversed"), al.Layout("guard", "nan", "reversed", 1)] + \
          [al.Layout("guard", "loud", "input", s) for s in (0, 2, 4, 5, 6)]


@pytest.mark.parametrize("layout", LAYOUTS, ids=lambda l: f"{l.gap}-{l.guard}-{l.order}-{l.shift}")
def test_kernels_in_every_layout(_ctx, layout):
    """Every residue of the planes' offsets, abutting tracks, tracks stored back to front: what lies around a plane (other
    tracks, full-scale or NaN guards) reaches no code and no band energy, and rewriting the guards changes no byte."""
    cases = [c for c in fc.cases() if c.name != "music_2s_s16_2ch"]
    arena, descs, guards = al.pack([Tr(list(c.channels), c.sample_rate) for c in cases], layout)
    descs = list(descs)[:len(cases)]
    dev = _ctx.fingerprint_arena(1, descs, arena)
    host = _ctx.fingerprint_arena(2, descs, arena)
    assert _same(dev, host), _first_difference(cases, dev, host)
    if guards:
        other = arena.copy()
        for a, b in guards:
            other[a:b] ^= 0x5A
        assert _same(_ctx.fingerprint_arena(1, descs, other), dev)


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
                _ctx.fingerprint_arena(route, [desc], arena)
            assert e.value.code == code and text in str(e.value)
            texts.append(str(e.value))
        assert texts[0] == texts[1]
    r = _ctx.fingerprint_arena(1, [_capi.TrackDesc(0, 4, 44100, 8, S16)], arena)[0][0]
    assert (r.status, r.channels, r.flags) == (0, 8, _capi.FP_COMPLETE | _capi.FP_SHORT)
    assert _ctx.fingerprint_arena(1, [], arena)[0] == []


# ---- stage 2 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mc", fc.match_cases() + (fc.default_case(),), ids=lambda mc: mc.name)
def test_match_kernel_equals_the_host_twin(_ctx, mc):
    dev = _ctx.fingerprint_match_codes(1, list(mc.codes), mc.rates, **mc.opts)
    host = _ctx.fingerprint_match_codes(0, list(mc.codes), mc.rates, **mc.opts)
    assert dev.tobytes() == host.tobytes(), np.argwhere(dev != host)[:4].tolist()
    assert _ctx.fingerprint_match_codes(1, list(mc.codes), mc.rates, **mc.opts).tobytes() == dev.tobytes()
    if mc.name == "defaults_40":  # copies of five originals, the later ones worn beyond the threshold or moved beyond the radius
        assert len(dev) == 780 and 20 < int((dev["flags"] & _capi.FP_PAIR_MATCH != 0).sum()) < 140
        assert int(np.abs(dev["lag"][dev["flags"] & _capi.FP_PAIR_MATCH != 0]).max()) > 256  # lags no single lane slot holds


def test_match_kernel_at_the_limits_of_its_options(_ctx):
    """The largest radius (16 lags per lane), a block that is no multiple of the lanes, the most probes."""
    a, b = fc.planted(700, 5000, 2047, 95, flips=[(5, 1), (350, 9)])
    c, d = fc.planted(700, 5000, -100, 97)
    for opts in (dict(block=300, probes=5, radius=2047, max_ber_permille=50), dict(block=7, probes=64, radius=2047, max_ber_permille=50),
                 dict(block=700, probes=2, radius=1, max_ber_permille=600)):
        codes = [a, b, c, d[100:]]
        dev = _ctx.fingerprint_match_codes(1, codes, [44100] * 4, **opts)
        host = _ctx.fingerprint_match_codes(0, codes, [44100] * 4, **opts)
        assert dev.tobytes() == host.tobytes(), (opts, dev.tolist(), host.tolist())
    assert host[0]["flags"] & _capi.FP_PAIR_COMPARED
