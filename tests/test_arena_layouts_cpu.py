"""The arena-layout tests' own footing, on the CPU: the packer (tests/arena_layouts.py) lays out what it says, and the tracks
(tests/layout_cases.py) test what they are meant to, on the references alone."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import arena_layouts as al  # noqa: E402
import layout_cases  # noqa: E402
import r128ref  # noqa: E402

TOL = 100.0 * layout_cases.load_measured()["worst_relative_block_error"]

LAYOUTS = [al.Layout(gap, guard, order, shift) for shift in (0, 3)
           for gap, guard, order in (("abut", "loud", "input"), ("guard", "loud", "input"), ("guard", "nan", "input"),
                                     ("guard", "loud", "reversed"), ("guard", "loud", "aliased"), ("abut", "loud", "reversed"),
                                     ("abut", "loud", "aliased"))]


class _T:
    def __init__(self, channels, rate):
        self.channels, self.sample_rate = channels, rate


def _tracks():
    made = {}
    return [made.setdefault(cid, _T(ch, rate)) for cid, ch, rate in layout_cases.with_repeats(layout_cases.rg1_cases())]


@pytest.mark.parametrize("layout", LAYOUTS, ids=lambda l: f"{l.gap}-{l.guard}-{l.order}-{l.shift}")
def test_packer(layout):
    tracks = _tracks()
    arena, descs, guards = al.pack(tracks, layout)
    spans, seen = [], {}
    for i, t in enumerate(tracks):
        d = descs[i]
        dt = t.channels[0].dtype
        bps = dt.itemsize
        assert (d.frames, d.sample_rate, d.channels, d.format) == (len(t.channels[0]), t.sample_rate, len(t.channels), al.FMT[dt])
        need = d.offset_bytes + d.channels * d.frames * bps
        assert d.offset_bytes % bps == 0 and need <= arena.nbytes
        for c, want in enumerate(t.channels):  # bit for bit (NaN-safe: compared as bytes)
            assert al.channel_bytes(arena, d, dt, c).tobytes() == want.tobytes(), (i, c)
        spans.append((int(d.offset_bytes), int(need), id(t)))
        seen.setdefault(bps, set()).add(int(d.offset_bytes) % 128)
    if layout.gap == "guard":
        for bps, got in seen.items():  # every format meets every residue class
            assert got == set(al.residues(bps)), (bps, sorted(got))
    # storage order
    offs = [s[0] for s in spans]
    first = {}
    same = [first.setdefault(s[2], i) for i, s in enumerate(spans)]
    if layout.order == "aliased":
        assert all(offs[i] == offs[same[i]] for i in range(len(offs))) and any(same[i] != i for i in range(len(offs)))
    else:
        assert len({(s[0], s[1]) for s in spans if s[1] > s[0]}) == len([s for s in spans if s[1] > s[0]])  # a copy each
        order = [o for o in offs]
        assert order == sorted(order, reverse=layout.order == "reversed")
    # no two stored tracks overlap, no guard touches a track, every guard byte holds a guard
    stored = sorted({(a, b) for a, b, _ in spans if b > a})
    assert all(stored[k][1] <= stored[k + 1][0] for k in range(len(stored) - 1))
    for g0, g1 in guards:
        assert 0 <= g0 < g1 <= arena.nbytes
        assert all(g1 <= a or b <= g0 for a, b in stored), (g0, g1)
    if layout.gap == "abut":
        assert guards == []
        assert all(stored[k + 1][0] - stored[k][1] < 4 for k in range(len(stored) - 1))  # alignment bytes only
    else:
        covered = np.zeros(arena.nbytes, dtype=bool)
        for g0, g1 in guards:
            covered[g0:g1] = True
        for i, t in enumerate(tracks):
            dt = t.channels[0].dtype
            bps = dt.itemsize
            a, b, _ = spans[i]
            n = al.GUARD_FRAMES * bps
            assert a >= n and covered[a - n:a].all() and covered[b:b + n].all(), i
            for lo in (a - n, b):  # the samples directly before and behind the track, in its own format
                g = arena[lo:lo + n].view(dt)
                if dt == np.float32 and layout.guard == "nan":
                    assert np.isnan(g).all()
                elif dt == np.float32:
                    assert np.all(np.abs(g) == np.float32(1e30)) and np.all(g[:-1] == -g[1:])
                else:
                    assert set(g.tolist()) == {np.iinfo(dt).min, np.iinfo(dt).max} and np.all(g[:-1] != g[1:])


def test_cases_are_quiet_and_full_scale_is_exact():
    for cid, ch, rate in layout_cases.rg1_cases() + layout_cases.r128_cases():
        for c in ch:  # a guard is at least 128 times every sample but the few at full scale
            x = np.abs(r128ref.normalise(c))
            assert np.all((x <= layout_cases.QUIET) | (x == 1.0)) and np.count_nonzero(x == 1.0) <= 4, cid
        if cid.startswith(("edge", "tp")):
            assert r128ref.sample_peak(ch[:2]) == 1.0, cid
    ids = [c[0] for c in layout_cases.r128_cases()]
    assert len(set(ids)) == len(ids)
    ids = [c[0] for c in layout_cases.rg1_cases()]
    assert len(set(ids)) == len(ids)
    assert sum(c.nbytes for cases in (layout_cases.rg1_cases(), layout_cases.r128_cases()) for _, ch, _ in cases for c in ch) < 12 << 20


def test_r128_precondition_no_block_near_a_gate():
    """The rule of test_gpu_r128.test_parity_precondition_no_block_near_a_gate, for every layout case, none exempt."""
    for cid, ch, rate in layout_cases.r128_cases():
        z = r128ref.block_z(ch, rate)
        _, _, thr = r128ref.gate(z)
        for gate in (r128ref.ABS_GATE, thr):
            if len(z):
                d = float(np.min(np.abs(z - gate) / gate))
                assert d > 10.0 * TOL, (cid, gate, d)


def test_r128_album_precondition_no_block_near_a_gate():
    """The album the GPU test analyses (every layout track, the repeated ones too): no block near either of its gates."""
    _, album = r128ref.analyze_album([(ch, rate) for _, ch, rate in layout_cases.with_repeats(layout_cases.r128_cases())])
    _, _, thr = r128ref.gate(album["z"])
    for gate in (r128ref.ABS_GATE, thr):
        assert float(np.min(np.abs(album["z"] - gate) / gate)) > 10.0 * TOL


def _tp_outputs(x, rate):
    F = r128ref.tp_factor(rate)
    u = np.zeros(len(x) * F)
    u[::F] = r128ref.normalise(x)
    return np.abs(np.convolve(u, r128ref.tp_taps(F))), F


def test_true_peak_geometry_cases_test_the_tail():
    crossing = {8000: 0, 96000: 0}
    for cid, ch, rate, where in layout_cases.tp_geometry_cases():
        n = len(ch[0])
        assert r128ref.true_peak(ch, rate) == 1.0, cid
        if where != n - 1:
            continue
        y, F = _tp_outputs(ch[-1], rate)  # the channel that carries the sample
        # output frame k = outputs k F .. k F + F - 1; the sample at frame N - 1 peaks 24 / F frames later
        assert float(y[:n * F].max()) < 0.1, cid
        peak_frame = int(np.argmax(y)) // F
        assert peak_frame == n - 1 + 24 // F and y[int(np.argmax(y))] == 1.0, cid
        if peak_frame // layout_cases.TP_CHUNK != (n - 1) // layout_cases.TP_CHUNK:
            crossing[rate] += 1
    assert all(v >= 2 for v in crossing.values()), crossing


def test_true_peak_of_the_nonfinite_case_is_finite_and_decided_by_what_is_dropped():
    ch, rate = layout_cases.nonfinite_case()
    ref = r128ref.analyze(ch, rate, True)
    assert np.isfinite(ref["true_peak"]) and 0.6 < ref["true_peak"] < 0.7 and np.isnan(ref["loudness_lufs"])
    assert ref["sample_peak"] == 1.0
    # were the touched outputs counted, the true peak would be the full-scale samples'; were one frame more dropped behind
    # the NaN, the 0.63 would be gone
    clean = [np.nan_to_num(c, nan=0.0, posinf=0.0, neginf=0.0) for c in ch]
    assert r128ref.true_peak(clean, rate) >= 1.0
    m = len(ch[0]) // 2
    y, F = _tp_outputs(clean[0], rate)
    y[F * (m - 5):F * (m + 14)] = 0.0
    assert float(y.max()) <= 0.5  # the second 0.5 sample itself, one frame on
    y, F = _tp_outputs(clean[0], rate)
    assert int(np.argmax(y[F * (m + 13):F * (m + 14)])) == 2 and abs(float(y[F * (m + 13) + 2]) - ref["true_peak"]) < 1e-3


def test_measured_bar_was_recorded_over_exactly_these_cases():
    """tests/golden/r128_layout_measured.json is what `tools/r128_refcheck.py --layout-cases --record` writes for the cases as
    they are now; a short case measured again stays within the recorded worst."""
    rec = layout_cases.load_measured()
    cases = layout_cases.r128_cases()
    assert sorted(rec["per_case"]) == sorted(c[0] for c in cases)
    assert rec["worst_relative_block_error"] == max(rec["per_case"].values()) > 0.0
    _, ch, rate = next(c for c in cases if c[0].startswith("len-7hops+799"))
    z64, zld = r128ref.block_z(ch, rate), r128ref.block_z(ch, rate, np.longdouble)
    assert len(z64) == 4 and float(np.max(np.abs(z64 - zld) / zld)) <= rec["worst_relative_block_error"]
