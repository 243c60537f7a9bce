"""Loudness range and momentary / short-term maxima, CPU side: the checker (tests/r128range_ref.py) against the EBU Tech 3342
and Tech 3341 signals and on the edge rules; rg_r128_short_term_count against it; the precondition of the GPU comparison (no
block of any test signal sits at a gate), on the checker alone; the command line's --range switch."""
import io
import math
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import r128cases  # noqa: E402
import r128range_cases as cases  # noqa: E402
import r128range_ref as ref  # noqa: E402
import r128ref  # noqa: E402

TOL = 100.0 * cases.load_measured()["worst_relative_st_error"]
TOL_Z = 100.0 * r128cases.load_measured()["worst_relative_block_error"]  # the gating blocks' existing tolerance


@pytest.mark.parametrize("rate", [44100, 48000])
@pytest.mark.parametrize("name,segments,want", ref.TECH3342, ids=[c[0] for c in ref.TECH3342])
def test_checker_tech3342(rate, name, segments, want):
    got = ref.analyze(ref.tech3342_signal(rate, segments), rate)
    print(f"{name} at {rate} Hz: LRA {got['loudness_range_lu']:.4f} LU (expected {want} +- 1), {got['range_low_lufs']:.3f} .. "
          f"{got['range_high_lufs']:.3f} LUFS, {got['st_blocks_gated']} of {got['st_blocks']} blocks")
    assert abs(got["loudness_range_lu"] - want) <= 1.0


@pytest.mark.parametrize("name,segments,want", r128ref.TECH3341_LOUDNESS[:4], ids=[c[0] for c in r128ref.TECH3341_LOUDNESS[:4]])
def test_checker_maxima_on_tech3341(name, segments, want):
    loudest = max(db for _, db in segments)
    got = ref.analyze(r128ref.sine_segments(48000, segments), 48000)
    print(f"{name}: max momentary {got['max_momentary_lufs']:.4f}, max short-term {got['max_short_term_lufs']:.4f}, loudest segment {loudest}")
    assert abs(got["max_momentary_lufs"] - loudest) <= 0.1 and abs(got["max_short_term_lufs"] - loudest) <= 0.1


def test_checker_edges():
    rate = 48000
    rng = np.random.default_rng(3)
    short = [0.1 * rng.standard_normal(int(2.95 * rate))]  # under 3 s: gating blocks, no short-term block
    r = ref.analyze(short, rate)
    assert (r["st_blocks"], r["st_blocks_gated"], r["loudness_range_lu"]) == (0, 0, 0.0)
    assert r["range_low_lufs"] == r["range_high_lufs"] == r["max_short_term_lufs"] == -math.inf and math.isfinite(r["max_momentary_lufs"])
    r = ref.analyze([np.zeros(4 * rate)], rate)  # silence
    assert r["st_blocks"] == 11 and r["st_blocks_gated"] == 0 and r["loudness_range_lu"] == 0.0
    assert r["max_momentary_lufs"] == r["max_short_term_lufs"] == r["range_low_lufs"] == r["range_high_lufs"] == -math.inf
    r = ref.analyze([1e-5 * rng.standard_normal(4 * rate)], rate)  # under the absolute gate: n = 0, the maxima are finite
    assert r["st_blocks_gated"] == 0 and r["loudness_range_lu"] == 0.0 and r["range_low_lufs"] == -math.inf
    assert -120.0 < r["max_short_term_lufs"] < -70.0 and -120.0 < r["max_momentary_lufs"] < -70.0
    assert ref.analyze([np.zeros(100)], rate)["max_momentary_lufs"] == -math.inf  # no block at all
    x = 0.1 * rng.standard_normal(4 * rate)
    x[rate] = np.inf
    r = ref.analyze([x], rate)
    assert all(math.isnan(r[k]) for k in ("loudness_range_lu", "range_low_lufs", "range_high_lufs", "max_momentary_lufs", "max_short_term_lufs"))
    assert r["st_blocks"] == 11 and r["st_blocks_gated"] == 0
    _, album = ref.analyze_album([([x], rate), (short, rate)])
    assert math.isnan(album["loudness_range_lu"]) and math.isnan(album["max_momentary_lufs"]) and album["st_blocks"] == 11
    # the ranks: integer division, elements of the list
    assert [ref.ranks(n) for n in (1, 2, 10, 11, 100, 101)] == [(0, 0), (0, 1), (1, 9), (1, 10), (10, 94), (10, 95)]
    st = np.array([4.0, 1.0, 3.0, 2.0]) * 1e-3
    r = ref.loudness_range(st)
    assert (r["low"], r["high"], r["st_blocks_gated"]) == (1e-3, 4e-3, 4)


@pytest.mark.parametrize("rate", [8000, 11025, 22050, 44100, 96000, 176400, 192000, 384000])
def test_short_term_count(capi, rate):
    hop = (rate + 5) // 10
    for frames in (0, hop - 1, 3 * hop - 1, 3 * hop, 4 * hop - 1, 4 * hop, 4 * hop + 1, 5 * hop, 100 * hop + 7,
                   29 * hop - 1, 29 * hop, 30 * hop - 1, 30 * hop, 30 * hop + 1, 31 * hop):
        assert capi.rg_r128_short_term_count(rate, frames) == ref.short_term_count(rate, frames) == max(frames // hop - 29, 0)


def test_short_term_count_unsupported_rate(capi):
    assert capi.rg_r128_short_term_count(7999, 1 << 20) == 0 and capi.rg_r128_short_term_count(384001, 1 << 24) == 0


# ---- the precondition of the GPU comparison ------------------------------------------------------------------------------
def _no_block_near(name, values, gates, tol):
    for gate in gates:
        if len(values):
            d = float(np.min(np.abs(values - gate) / gate))
            assert d > 10.0 * tol, (name, gate, d)
            yield d


def test_precondition_no_block_near_a_gate():
    """On the checker alone, over every case of the range set, the Tech 3342 signals as the GPU test runs them and the album
    of the GPU tests: no short-term block within relative 10 x tol of the absolute gate or of the -20 LU threshold, and no
    gating block within 10 x its tolerance of the loudness gates.  A block then cannot change sides within the tolerance, and
    the comparison of counts, bounds and range is meaningful for every case: none is left out."""
    closest = 1.0
    tracks = [(c[0], cases.make(*c[1:]), c[2]) for c in cases.range_cases()]
    tracks += [(f"{name}-{rate}-{fmt}", ch, rate) for name, rate, fmt, ch, _ in cases.conformance_tracks()]
    album = cases.album_tracks()
    tracks += [(f"album-track-{i}", ch, rate) for i, (ch, rate, _, _) in enumerate(album)]
    for name, ch, rate in tracks:
        r = ref.analyze(ch, rate)
        _, _, zthr = r128ref.gate(r["z"])
        closest = min([closest, *_no_block_near(name, r["st"], (ref.ABS_GATE, r["thr"]), TOL),
                       *_no_block_near(name, r["z"], (r128ref.ABS_GATE, zthr), TOL_Z)])
    res, alb = ref.analyze_album([(ch, rate) for ch, rate, _, _ in album])
    _, zalb = r128ref.analyze_album([(ch, rate) for ch, rate, _, _ in album])
    _, _, zthr = r128ref.gate(zalb["z"])
    closest = min([closest, *_no_block_near("album", alb["st"], (ref.ABS_GATE, alb["thr"]), TOL),
                   *_no_block_near("album", zalb["z"], (r128ref.ABS_GATE, zthr), TOL_Z)])
    # the large album: tracks of the range set, some of them many times over
    by_id = {name: (ch, rate) for name, ch, rate in tracks}
    res_l, alb_l = ref.analyze_album([by_id[i] for i in cases.large_album_ids()])
    assert alb_l["st_blocks"] == 69029 and 0 < alb_l["st_blocks_gated"] < alb_l["st_blocks"]
    closest = min([closest, *_no_block_near("large-album", alb_l["st"], (ref.ABS_GATE, alb_l["thr"]), TOL)])
    print(f"closest block to a gate: {closest:.3e} relative (tolerances {TOL:.2e} short-term, {TOL_Z:.2e} gating)")
    # the album is what the GPU test says it is: the third track wholly under the album's -20 LU gate and whole in itself,
    # and the album's range is none of its tracks'
    quiet = res[2]
    assert np.all(quiet["st"] < alb["thr"]) and np.all(quiet["st"] >= ref.ABS_GATE) and quiet["st_blocks_gated"] == quiet["st_blocks"] > 0
    assert alb["st_blocks_gated"] == sum(int(np.count_nonzero(r["st"] >= alb["thr"])) for r in res) < alb["st_blocks"]
    assert all(abs(alb["loudness_range_lu"] - r["loudness_range_lu"]) > 0.1 for r in res)


@pytest.mark.parametrize("n_blocks", cases.EDGE_ALBUM_BLOCKS)
def test_precondition_edge_albums(n_blocks):
    """The albums at the sizes where the wide selection's partition changes shape (tests/test_gpu_r128_range.py:
    test_album_sizes_at_the_partition_edges): the union has exactly that many short-term blocks, and none of them lies within
    10 x tol of the absolute gate or of the album's -20 LU threshold, on the checker alone."""
    _, alb = ref.analyze_album(cases.edge_album_tracks(n_blocks))
    assert alb["st_blocks"] == n_blocks and alb["st_blocks_gated"] > 0
    closest = min(_no_block_near(f"edge-album-{n_blocks}", alb["st"], (ref.ABS_GATE, alb["thr"]), TOL))
    print(f"{n_blocks} blocks, {alb['st_blocks_gated']} kept: closest block to a gate {closest:.3e} relative (tolerance {TOL:.2e})")


# ---- command line -------------------------------------------------------------------------------------------------------
def test_cli_parses_range():
    from mp3rgain_amd import cli

    o = cli.parse_args(["--r128", "--range", "-r", "a.mp3"], io.StringIO(), io.StringIO())
    assert o.r128 and o.loudness_range and o.track_gain and [str(f) for f in o.files] == ["a.mp3"]
    o = cli.parse_args(["--r128", "-r", "a.mp3"], io.StringIO(), io.StringIO())
    assert o.r128 and not o.loudness_range
    o = cli.parse_args(["--range", "-r", "a.mp3"], io.StringIO(), io.StringIO())  # without --r128: accepted, as --true-peak is
    assert o.loudness_range and not o.r128
    out = io.StringIO()
    assert cli.main(["--help"], out, io.StringIO()) == 0
    assert "--range" in out.getvalue() and "--r128" in out.getvalue()


def test_python_surface():
    import dataclasses
    import inspect

    import mp3rgain_amd as rg

    assert [f.name for f in dataclasses.fields(rg.R128Dynamics)] == ["loudness_range_lu", "range_low_lufs", "range_high_lufs",
                                                                    "max_momentary_lufs", "max_short_term_lufs", "st_blocks", "st_blocks_gated"]
    assert rg.R128Result(0.0, 0.0, 0.0, 0.0, 48000).dynamics is None and rg.R128AlbumResult([], 0.0, 0.0, 0.0, 0.0).dynamics is None
    for name in ("analyze_tracks_r128", "analyze_album_r128", "analyze_track_files_r128", "analyze_album_files_r128"):
        p = inspect.signature(getattr(rg.Analyzer, name)).parameters
        assert p["dynamics"].default is False, name
