"""The spectral scan on the GPU (include/mp3rgain_amd_spectrum.h): the two kernels through their seam (rg_spectrum_arena, route 1) on
the shared cases (tests/spectrum_cases.py), byte for byte against the kernels' arithmetic on the host (route 2), which
tests/test_spectrum_cpu.py holds to the float64 restatement, in the arena layouts every PCM-reading kernel is held to.  A handful
of launches; the only tolerance is the measured one of tests/golden/spectrum_measured.json."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import arena_layouts as al  # noqa: E402
import spectrum_cases as sc  # noqa: E402

from mp3rgain_amd import _capi  # noqa: E402

pytestmark = pytest.mark.gpu

RG_ERR_INVALID_ARG, RG_ERR_FORMAT = -1, -9


def _raw(recs):
    return b"".join(bytes(r) for r in recs)


def _first_difference(tracks, a, ea, b, eb):
    for i, tr in enumerate(tracks):
        if bytes(a[i]) != bytes(b[i]):
            return tr.name, sc.got(a[i]), sc.got(b[i])
        if ea[i].tobytes() != eb[i].tobytes():
            c, j = np.argwhere(ea[i] != eb[i])[0]
            return tr.name, int(c), int(j), float(ea[i][c, j]), float(eb[i][c, j]), int((ea[i] != eb[i]).sum())
    return None


@pytest.fixture(scope="module")
def packed():
    tracks = sc.tracks()
    arena, descs, guards = al.pack(tracks, al.Layout("guard", "loud", "input", 3))
    return tracks, arena, list(descs)[:len(tracks)], guards


def test_kernels_match_their_host_arithmetic_on_every_case(_ctx, packed):
    """Every case of all three formats in one launch, between loud guards at odd alignments: route 1 == route 2 byte for byte,
    records and bands, and the same call twice gives the same bytes."""
    tracks, arena, descs, guards = packed
    assert {d.format for d in descs} == {0, 1, 2} and guards
    dev, e_dev = _ctx.spectrum_arena(1, descs, arena)
    host, e_host = _ctx.spectrum_arena(2, descs, arena)
    assert _raw(dev) == _raw(host) and e_dev.tobytes() == e_host.tobytes(), _first_difference(tracks, dev, e_dev, host, e_host)
    again, e_again = _ctx.spectrum_arena(1, descs, arena)
    assert _raw(again) == _raw(dev) and e_again.tobytes() == e_dev.tobytes()


def test_kernels_against_the_restatement(_ctx, packed):
    """Route 1 against float64 numpy within 8 times the recorded f32 error, and the verdicts those of the restatement."""
    tracks, arena, descs, _ = packed
    wants = sc.wants()
    of_total, relative = (sc.TOLERANCE_FACTOR * x for x in sc.measured())
    dev, e = _ctx.spectrum_arena(1, descs, arena)
    for i, tr in enumerate(tracks):
        for c, (ref, analysed, skipped) in enumerate(wants[tr.name]):
            ch = dev[i].ch[c]
            assert (ch.analysed_frames, ch.skipped_frames) == (analysed, skipped), tr.name
            a, b = sc.errors(e[i, c], ref)
            print(f"{tr.name} ch {c}: of total {a:.3e} (allowed {of_total:.3e}), relative {b:.3e} (allowed {relative:.3e})")
            assert a <= of_total and b <= relative, tr.name
            # the verdict arithmetic exactly, on the energies it was given; and on the verdict cases, which lie tens of dB from
            # every threshold, the band and flags the float64 energies give
            assert (ch.cutoff_hz, ch.edge_db, ch.flags) == sc.verdict_of_energy(e[i, c], analysed, tr.sample_rate), tr.name
            if tr.name.startswith("verdict-"):
                cutoff, edge, flags = sc.verdict_of_energy(ref, analysed, tr.sample_rate)
                assert (ch.cutoff_hz, ch.flags) == (cutoff, flags), tr.name
        assert dev[i].flags == sc.want_track_flags(tr, [x.flags for x in dev[i].ch[:len(tr.channels)]], [w[2] for w in wants[tr.name]]), tr.name


def _short(tracks):
    return [tr for tr in tracks if len(tr.channels[0]) <= sc.L + 6 * sc.H + 100]


LAYOUTS = [al.Layout("abut", "loud", "input"), al.Layout("abut", "loud", "reversed"), al.Layout("guard", "nan", "reversed", 1)] + \
          [al.Layout("guard", "loud", "input", s) for s in (0, 2, 4, 5, 6)]


@pytest.mark.parametrize("layout", LAYOUTS, ids=lambda l: f"{l.gap}-{l.guard}-{l.order}-{l.shift}")
def test_kernels_in_every_layout(_ctx, layout):
    """Every residue of the planes' offsets modulo 128, abutting tracks, tracks stored back to front: what lies around a plane
    (other tracks, full-scale or NaN guards) reaches no record, and rewriting the guards changes no byte."""
    tracks = _short(sc.tracks())
    arena, descs, guards = al.pack(tracks, layout)
    descs = list(descs)[:len(tracks)]
    dev, e_dev = _ctx.spectrum_arena(1, descs, arena)
    host, e_host = _ctx.spectrum_arena(2, descs, arena)
    assert _raw(dev) == _raw(host) and e_dev.tobytes() == e_host.tobytes(), _first_difference(tracks, dev, e_dev, host, e_host)
    if guards:
        other = arena.copy()
        for a, b in guards:
            other[a:b] ^= 0x5A
        again, e_again = _ctx.spectrum_arena(1, descs, other)
        assert _raw(again) == _raw(dev) and e_again.tobytes() == e_dev.tobytes()


def test_kernels_refuse_what_the_host_routes_refuse(_ctx):
    import mp3rgain_amd as rg

    arena = np.zeros(64, dtype=np.uint8)
    S16 = _capi.FMT_S16_PLANAR
    for desc, code, text in ((_capi.TrackDesc(0, 17, 44100, 2, S16), RG_ERR_INVALID_ARG, "beyond the arena"),
                             (_capi.TrackDesc(1, 4, 44100, 2, S16), RG_ERR_INVALID_ARG, "sample-aligned"),
                             (_capi.TrackDesc(0, 1, 44100, 9, S16), RG_ERR_FORMAT, "9 channel")):
        with pytest.raises(rg.ReplayGainError) as e:
            _ctx.spectrum_arena(1, [desc], arena)
        assert e.value.code == code and text in str(e.value)
    for opts in ((0.0, 4000.0), (30.0, 0.0), (-1.0, None)):
        with pytest.raises(rg.ReplayGainError) as e:
            _ctx.spectrum_arena(1, [_capi.TrackDesc(0, 4, 44100, 2, S16)], arena, *opts)
        assert e.value.code == RG_ERR_INVALID_ARG and "greater than 0" in str(e.value)
    recs, e = _ctx.spectrum_arena(1, [_capi.TrackDesc(0, 4, 44100, 8, S16)], arena)
    r = recs[0]
    assert (r.status, r.channels, r.cutoff_hz, r.flags) == (0, 8, 0.0, _capi.SPEC_SHORT | _capi.SPEC_COMPLETE) and not e.any()
    recs, e = _ctx.spectrum_arena(1, [], arena)
    assert recs == [] and e.shape[0] == 0
