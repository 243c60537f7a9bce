"""Loudness range (EBU Tech 3342) and momentary / short-term maxima on the GPU (mp3rgain_amd/csrc/rg_r128_range.hip) against
the float64 checker tests/r128range_ref.py: Tech 3342 conformance, every short-term block of the range set
(tests/r128range_cases.py) within a tolerance MEASURED on the checker itself (tests/golden/r128_range_measured.json,
tools/r128_range_refcheck.py: 100 x the float64 checker's worst relative short-term block error against np.longdouble),
counts, bounds, range and maxima, albums (PCM and files, in one group and in several), edge rules, and the results of the
plain calls left as they were.  tests/test_r128_range_cpu.py holds the precondition: no block of these signals sits within
10 x the tolerance of a gate."""
import dataclasses
import math
import struct
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import flacenc as fe  # noqa: E402
import r128cases  # noqa: E402
import r128range_cases as cases  # noqa: E402
import r128range_ref as ref  # noqa: E402
from wavutil import wav_bytes  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = Path(__file__).parent / "golden"
TOL = 100.0 * cases.load_measured()["worst_relative_st_error"]
LU = 4.343  # d(10 log10 x) = 4.343 dx / x
FIELDS = ("loudness_range_lu", "range_low_lufs", "range_high_lufs", "max_momentary_lufs", "max_short_term_lufs")


@pytest.fixture()
def an(_ctx):
    _ctx.set_kernel(0)
    for key in (1, 2, 4, 10, 13):
        _ctx.set_tuning(key, 0)
    _ctx.set_tuning(14, 1)
    _ctx.set_tuning_r128(1, 0)
    _ctx.set_tuning_r128(2, 0)
    _ctx.set_decoder_command(None)
    yield _ctx
    _ctx.set_tuning_r128(1, 0)
    _ctx.set_tuning_r128(2, 0)
    _ctx.set_tuning(13, 0)


def _track(chans, rate):
    import mp3rgain_amd as rg

    return rg.PcmTrack(chans, rate)


def _bits(x):
    return struct.pack("<d", x)


def _dyn_bytes(d):
    return b"".join(_bits(getattr(d, k)) for k in FIELDS) + struct.pack("<2I", d.st_blocks, d.st_blocks_gated)


def _res_bytes(r):
    """The loudness side of a result (what the plain call returns), as bytes: NaN compares equal to itself."""
    head = struct.pack("<4d", r.loudness_lufs, r.gain_db, r.sample_peak, r.true_peak)
    return head + struct.pack("<3I", getattr(r, "sample_rate", 0), r.blocks, r.blocks_gated) + struct.pack("<I", getattr(r, "flags", 0))


def _close(cid, what, got, want, tol):
    if math.isinf(want) or math.isnan(want):
        assert _bits(got) == _bits(want) or (math.isnan(got) and math.isnan(want)), (cid, what, got, want)
    else:
        assert abs(got - want) <= tol, (cid, what, got, want, tol)


def _check_dynamics(cid, d, r, st=None):
    """d: R128Dynamics of the library, r: the checker's dict, st: the library's short-term blocks (or None)."""
    print(f"{cid}: LRA {d.loudness_range_lu:.6f} LU (ref {r['loudness_range_lu']:.6f}), {d.range_low_lufs:.4f} .. {d.range_high_lufs:.4f} LUFS, "
          f"max M {d.max_momentary_lufs:.4f} (ref {r['max_momentary_lufs']:.4f}), max S {d.max_short_term_lufs:.4f} "
          f"(ref {r['max_short_term_lufs']:.4f}), blocks {d.st_blocks} gated {d.st_blocks_gated}", end="")
    assert d.st_blocks == r["st_blocks"], cid
    if st is not None:
        sr = r["st"]
        assert len(st) == len(sr) == d.st_blocks, cid
        if len(sr):
            above = sr >= ref.ABS_GATE
            err_above = float(np.max(np.abs(st[above] - sr[above]) / sr[above])) if np.any(above) else 0.0
            err_below = float(np.max(np.abs(st[~above] - sr[~above]))) / ref.ABS_GATE if np.any(~above) else 0.0
            print(f", worst block error {err_above:.2e} relative above the gate, {err_below:.2e} of the gate below it (bar {TOL:.2e})", end="")
            assert err_above <= TOL and err_below <= TOL, (cid, err_above, err_below)
    print()
    assert d.st_blocks_gated == r["st_blocks_gated"], cid
    _close(cid, "lra", d.loudness_range_lu, r["loudness_range_lu"], 2.0 * LU * TOL)
    for k in FIELDS[1:]:
        _close(cid, k, getattr(d, k), r[k], LU * TOL)
    if st is not None and d.st_blocks_gated:
        # The bounds are elements of the library's own block list: its kept elements, sorted, at the definition's two ranks.
        # The struct carries them in LUFS, computed by the device's log10; the host's log10 of the very same element may round
        # the other way, so the comparison allows 4 ulp of the LUFS value (1.4e-14 at -20 LUFS) and no more: neither an
        # interpolated value nor a histogram bin's edge comes that near.  Steady signals have neighbouring elements a few ulp
        # apart, so "the nearest element" is not asked for.  The range is 10 log10 of exactly those two elements.
        K = np.sort(st[(st >= ref.ABS_GATE) & (st >= r["thr"])])
        assert len(K) == d.st_blocks_gated, cid
        lo, hi = (float(K[rank]) for rank in ref.ranks(len(K)))
        for k, want in (("range_low_lufs", lo), ("range_high_lufs", hi)):
            bound = getattr(d, k)
            assert abs((-0.691 + 10.0 * math.log10(want)) - bound) <= 4.0 * math.ulp(abs(bound)), (cid, k, bound, want)
        assert abs(10.0 * math.log10(hi / lo) - d.loudness_range_lu) <= 4.0 * math.ulp(max(d.loudness_range_lu, 1.0)), cid


# ---- conformance: EBU Tech 3342 -----------------------------------------------------------------------------------------
def test_tech3342(an):
    conf = cases.conformance_tracks()
    res = an.analyze_tracks_r128([_track(ch, rate) for _, rate, _, ch, _ in conf], dynamics=True)
    bad = []
    for (name, rate, fmt, ch, want), r in zip(conf, res):
        d = r.dynamics
        _check_dynamics(f"{name}-{rate}-{fmt}", d, ref.analyze(ch, rate))
        print(f"    expected {want} +- 1 LU")
        if not abs(d.loudness_range_lu - want) <= 1.0:
            bad.append((name, rate, fmt, d.loudness_range_lu))
    assert not bad, bad


# ---- parity per short-term block -----------------------------------------------------------------------------------------
_CACHE = {}


def _range_set():
    if not _CACHE:
        cs = cases.range_cases()
        chans = [cases.make(*c[1:]) for c in cs]
        refs = [ref.analyze(ch, c[2]) for ch, c in zip(chans, cs)]
        _CACHE["set"] = (cs, chans, refs)
    return _CACHE["set"]


@pytest.mark.parametrize("S", [0, 1, 5, 64], ids=lambda s: f"S{s}")
def test_parity_per_short_term_block(an, S):
    """The whole range set in ONE batch, at several hops-per-lane of the loudness kernel."""
    cs, chans, refs = _range_set()
    an.set_tuning_r128(1, S)
    res, blocks, st = an.analyze_tracks_r128([_track(ch, c[2]) for ch, c in zip(chans, cs)], return_blocks=True, dynamics=True,
                                             return_short_term=True)
    assert any(r["st_blocks"] > 2048 for r in refs)  # a track in several chunks of the block kernel
    for c, r, z, s, rf in zip(cs, res, blocks, st, refs):
        _check_dynamics(c[0], r.dynamics, rf, s)
        assert len(z) == len(rf["z"]) == r.blocks and r.flags == 0, c[0]


def test_plain_results_are_unchanged_and_runs_repeat(an):
    cs, chans, _ = _range_set()
    tracks = [_track(ch, c[2]) for ch, c in zip(chans, cs)]
    plain, zp = an.analyze_tracks_r128(tracks, true_peak=True, return_blocks=True)
    dyn, zd, st = an.analyze_tracks_r128(tracks, true_peak=True, return_blocks=True, dynamics=True, return_short_term=True)
    assert all(p.dynamics is None for p in plain) and all(d.dynamics is not None for d in dyn)
    assert [_res_bytes(p) for p in plain] == [_res_bytes(d) for d in dyn]
    assert [dataclasses.replace(d, dynamics=None) for d in dyn] == plain
    assert all(a.tobytes() == b.tobytes() for a, b in zip(zp, zd))
    again, za, sa = an.analyze_tracks_r128(tracks, true_peak=True, return_blocks=True, dynamics=True, return_short_term=True)
    assert [_res_bytes(d) + _dyn_bytes(d.dynamics) for d in dyn] == [_res_bytes(d) + _dyn_bytes(d.dynamics) for d in again]
    assert all(a.tobytes() == b.tobytes() for a, b in zip(st, sa)) and all(a.tobytes() == b.tobytes() for a, b in zip(zd, za))
    # one track per call: the same bits as in the batch
    for i in (0, 6, 11):
        one, s1 = an.analyze_tracks_r128([tracks[i]], true_peak=True, dynamics=True, return_short_term=True)
        assert _dyn_bytes(one[0].dynamics) == _dyn_bytes(dyn[i].dynamics) and s1[0].tobytes() == st[i].tobytes(), cs[i][0]
    # the album call
    pa = an.analyze_album_r128(tracks[:6], true_peak=True)
    da = an.analyze_album_r128(tracks[:6], true_peak=True, dynamics=True)
    assert _res_bytes(pa) == _res_bytes(da) and [_res_bytes(t) for t in pa.tracks] == [_res_bytes(t) for t in da.tracks]
    assert pa.dynamics is None and da.dynamics is not None
    assert [_dyn_bytes(t.dynamics) for t in da.tracks] == [_dyn_bytes(d.dynamics) for d in dyn[:6]]


# ---- album --------------------------------------------------------------------------------------------------------------
def _album():
    if "album" not in _CACHE:
        tr = cases.album_tracks()
        _CACHE["album"] = (tr, ref.analyze_album([(ch, rate) for ch, rate, _, _ in tr]))
    return _CACHE["album"]


def test_album_is_the_union_of_short_term_blocks(an):
    tr, (ref_tracks, ref_album) = _album()
    quiet = ref_tracks[2]  # wholly under the album's -20 LU gate, whole in itself
    assert np.all(quiet["st"] < ref_album["thr"]) and quiet["st_blocks_gated"] == quiet["st_blocks"] > 0
    tracks = [_track(ch, rate) for ch, rate, _, _ in tr]
    got = {}
    for mode in (0, 1, 2):  # chosen by the library, one workgroup, wide counting passes
        an.set_tuning_r128(2, mode)
        a, st = an.analyze_album_r128(tracks, true_peak=True, dynamics=True, return_short_term=True)
        got[mode] = a
        _check_dynamics(f"album-mode{mode}", a.dynamics, ref_album, np.concatenate(st))
        for i, (t, s, rf) in enumerate(zip(a.tracks, st, ref_tracks)):
            _check_dynamics(f"album-track-{i}", t.dynamics, rf, s)
        assert all(abs(a.dynamics.loudness_range_lu - t.dynamics.loudness_range_lu) > 0.1 for t in a.tracks)
        assert a.dynamics.max_momentary_lufs == max(t.dynamics.max_momentary_lufs for t in a.tracks)
        assert a.dynamics.max_short_term_lufs == max(t.dynamics.max_short_term_lufs for t in a.tracks)
        again = an.analyze_album_r128(tracks, true_peak=True, dynamics=True)
        assert _dyn_bytes(again.dynamics) == _dyn_bytes(a.dynamics) and _res_bytes(again) == _res_bytes(a)
    assert _dyn_bytes(got[0].dynamics) == _dyn_bytes(got[1].dynamics) == _dyn_bytes(got[2].dynamics)
    # the tracks of an album are the tracks of a batch
    batch = an.analyze_tracks_r128(tracks, true_peak=True, dynamics=True)
    assert [_dyn_bytes(t.dynamics) for t in got[0].tracks] == [_dyn_bytes(t.dynamics) for t in batch]


def test_large_album_by_one_workgroup_and_by_wide_passes(an):
    """69029 short-term blocks: above the size from which the library chooses the wide passes, 270 blocks per workgroup of a
    wide pass (two iterations, full waves, many equal digits in a wave).  Both forms and the library's own choice against
    the checker's union, and equal to each other bit for bit."""
    cs, chans, refs = _range_set()
    idx = [[c[0] for c in cs].index(i) for i in cases.large_album_ids()]
    tracks = [_track(chans[i], cs[i][2]) for i in idx]
    st_ref = np.concatenate([refs[i]["st"] for i in idx])
    ref_album = ref.loudness_range(st_ref)
    ref_album.update(max_momentary_lufs=max(refs[i]["max_momentary_lufs"] for i in idx),
                     max_short_term_lufs=max(refs[i]["max_short_term_lufs"] for i in idx), st=st_ref)
    assert ref_album["st_blocks"] == 69029
    got = {}
    for mode in (0, 1, 2):
        an.set_tuning_r128(2, mode)
        a, st = an.analyze_album_r128(tracks, dynamics=True, return_short_term=True)
        got[mode] = a
        _check_dynamics(f"large-album-mode{mode}", a.dynamics, ref_album, np.concatenate(st))
        for i, t in zip(idx, a.tracks):
            assert _dyn_bytes(t.dynamics) == _dyn_bytes(a.tracks[idx.index(i)].dynamics)
    assert _dyn_bytes(got[0].dynamics) == _dyn_bytes(got[1].dynamics) == _dyn_bytes(got[2].dynamics)
    for i, t in zip(idx[25:], got[2].tracks[25:]):
        _check_dynamics(cs[i][0], t.dynamics, refs[i])


def _edge_album(n_blocks):
    if ("edge", n_blocks) not in _CACHE:
        tr = cases.edge_album_tracks(n_blocks)
        _CACHE["edge", n_blocks] = (tr, ref.analyze_album(tr)[1])
    return _CACHE["edge", n_blocks]


@pytest.mark.parametrize("n_blocks,mode", [(n, 2) for n in cases.EDGE_ALBUM_BLOCKS] + [(257, 1)], ids=lambda v: str(v))
def test_album_sizes_at_the_partition_edges(an, n_blocks, mode):
    """The union sizes at which the wide passes' 256 slices and their counting workgroups change shape (1, 255, 257, 4095,
    8193 blocks: tests/r128range_cases.py), forced wide, and 257 by one workgroup too, against the checker's union."""
    tr, ref_album = _edge_album(n_blocks)
    an.set_tuning_r128(2, mode)
    a, st = an.analyze_album_r128([_track(ch, rate) for ch, rate in tr], dynamics=True, return_short_term=True)
    assert a.dynamics.st_blocks == n_blocks
    _check_dynamics(f"edge-album-{n_blocks}-mode{mode}", a.dynamics, ref_album, np.concatenate(st))


def _write_album(tmp_path):
    tr, _ = _album()
    files = []
    for i, (ch, rate, container, kind) in enumerate(tr):
        f = tmp_path / f"t{i}.{container}"
        if container == "wav":
            f.write_bytes(wav_bytes(ch, rate, kind))
        else:
            bps = 16 if kind == "s16" else 24
            pcm = np.stack([c.astype(np.int64) >> (0 if bps == 16 else 8) for c in ch])
            f.write_bytes(fe.encode(pcm, rate, bps))
        files.append(f)
    return files


def test_album_files_in_one_group_and_in_several(an, tmp_path):
    tr, (ref_tracks, ref_album) = _album()
    files = _write_album(tmp_path)
    for mode in (0, 2):
        an.set_tuning_r128(2, mode)
        one = an.analyze_album_files_r128(files, true_peak=True, dynamics=True)
        an.set_tuning(13, 1)  # groups of one file each
        many = an.analyze_album_files_r128(files, true_peak=True, dynamics=True)
        an.set_tuning(13, 0)
        assert _dyn_bytes(one.dynamics) == _dyn_bytes(many.dynamics) and _res_bytes(one) == _res_bytes(many)
        assert [_dyn_bytes(t.dynamics) + _res_bytes(t) for t in one.tracks] == [_dyn_bytes(t.dynamics) + _res_bytes(t) for t in many.tracks]
        pcm = an.analyze_album_r128([_track(ch, rate) for ch, rate, _, _ in tr], true_peak=True, dynamics=True)
        assert _dyn_bytes(one.dynamics) == _dyn_bytes(pcm.dynamics)
        assert [_dyn_bytes(t.dynamics) for t in one.tracks] == [_dyn_bytes(t.dynamics) for t in pcm.tracks]
        assert (one.loudness_lufs, one.blocks, one.blocks_gated, one.sample_peak, one.true_peak) == \
            (pcm.loudness_lufs, pcm.blocks, pcm.blocks_gated, pcm.sample_peak, pcm.true_peak)
        _check_dynamics(f"file-album-mode{mode}", one.dynamics, ref_album)
    # without dynamics the file calls return what they returned
    plain = an.analyze_album_files_r128(files, true_peak=True)
    assert plain.dynamics is None and _res_bytes(plain) == _res_bytes(one) and all(t.dynamics is None for t in plain.tracks)
    as_tracks = an.analyze_track_files_r128(files, true_peak=True, dynamics=True)
    assert [_dyn_bytes(t.dynamics) for t in as_tracks] == [_dyn_bytes(t.dynamics) for t in one.tracks]
    for i, (t, rf) in enumerate(zip(as_tracks, ref_tracks)):
        _check_dynamics(f"file-{i}", t.dynamics, rf)


def test_per_file_errors_leave_the_others_intact(an, tmp_path):
    import mp3rgain_amd as rg

    files = _write_album(tmp_path)
    junk = tmp_path / "junk.mp3"
    junk.write_bytes(b"ID3" + bytes(500))
    low = tmp_path / "low.wav"
    low.write_bytes(wav_bytes([np.zeros(8000, dtype=np.int16)], 7999, "s16"))
    missing = tmp_path / "missing.flac"
    clean = an.analyze_track_files_r128(files, true_peak=True, dynamics=True)
    res = an.analyze_track_files_r128([files[0], missing, files[1], junk, low, files[2], files[3]], true_peak=True, dynamics=True)
    for i, j in ((0, 0), (2, 1), (5, 2), (6, 3)):
        assert not isinstance(res[i], Exception)
        assert _dyn_bytes(res[i].dynamics) + _res_bytes(res[i]) == _dyn_bytes(clean[j].dynamics) + _res_bytes(clean[j])
    plain = an.analyze_track_files_r128([files[0], missing, files[1], junk, low, files[2], files[3]], true_peak=True)
    for i in (1, 3, 4):
        assert isinstance(res[i], rg.ReplayGainError) and (res[i].code, str(res[i])) == (plain[i].code, str(plain[i]))
    assert (res[1].code, res[3].code, res[4].code) == (-8, -9, -2)
    with pytest.raises(rg.ReplayGainError, match="Failed to open"):
        an.analyze_album_files_r128([files[0], missing], dynamics=True)
    ok = an.analyze_album_files_r128([files[0]], true_peak=True, dynamics=True)  # the failed album left nothing behind
    assert _dyn_bytes(ok.tracks[0].dynamics) == _dyn_bytes(clean[0].dynamics)


# ---- edge rules ---------------------------------------------------------------------------------------------------------
def test_edge_rules(an):
    rate = 48000
    rng = np.random.default_rng(3)
    good = [(0.1 * rng.standard_normal(5 * rate)).astype(np.float32) for _ in range(2)]
    short = [(0.1 * rng.standard_normal(int(2.95 * rate))).astype(np.float32)]  # gating blocks, no short-term block
    silence = [np.zeros(4 * rate, dtype=np.float32)] * 2
    faint = [(1e-5 * rng.standard_normal(4 * rate)).astype(np.float32)]  # under the absolute gate: n = 0
    tiny = [np.zeros(100, dtype=np.int16)]
    nan = [good[0].copy(), good[1].copy()]
    nan[1][rate + 17] = np.nan
    sig = [good, short, silence, faint, tiny, nan, good]
    alone = an.analyze_tracks_r128([_track(good, rate)], dynamics=True)[0]
    res, st = an.analyze_tracks_r128([_track(c, rate) for c in sig], dynamics=True, return_short_term=True)
    assert _dyn_bytes(res[0].dynamics) == _dyn_bytes(res[6].dynamics) == _dyn_bytes(alone.dynamics)
    for i in (0, 1, 2, 3, 4, 6):
        _check_dynamics(f"edge-{i}", res[i].dynamics, ref.analyze(sig[i], rate), st[i])
    d = res[1].dynamics
    assert (d.st_blocks, d.st_blocks_gated, d.loudness_range_lu) == (0, 0, 0.0) and math.isfinite(d.max_momentary_lufs)
    assert d.range_low_lufs == d.range_high_lufs == d.max_short_term_lufs == -math.inf
    d = res[2].dynamics
    assert (d.st_blocks, d.st_blocks_gated, d.loudness_range_lu) == (11, 0, 0.0)
    assert d.range_low_lufs == d.range_high_lufs == d.max_short_term_lufs == d.max_momentary_lufs == -math.inf
    d = res[3].dynamics
    assert d.st_blocks_gated == 0 and d.loudness_range_lu == 0.0 and d.range_low_lufs == -math.inf and -120.0 < d.max_short_term_lufs < -70.0
    d = res[4].dynamics
    assert d.st_blocks == 0 and d.max_momentary_lufs == -math.inf
    d = res[5].dynamics
    assert res[5].flags == 1 and all(math.isnan(getattr(d, k)) for k in FIELDS) and (d.st_blocks, d.st_blocks_gated) == (21, 0)
    album = an.analyze_album_r128([_track(good, rate), _track(nan, rate)], dynamics=True)
    assert all(math.isnan(getattr(album.dynamics, k)) for k in FIELDS) and album.dynamics.st_blocks == 42
    assert _dyn_bytes(album.tracks[0].dynamics) == _dyn_bytes(alone.dynamics)
    empty = an.analyze_album_r128([], dynamics=True)
    assert empty.dynamics.st_blocks == 0 and empty.dynamics.loudness_range_lu == 0.0 and empty.dynamics.max_momentary_lufs == -math.inf
    assert an.analyze_tracks_r128([], dynamics=True) == []
    with pytest.raises(ValueError):
        an.analyze_tracks_r128([_track(good, rate)], return_short_term=True)


# ---- nothing else moved ------------------------------------------------------------------------------------------------------
def test_rg1_results_unchanged_around_a_dynamics_call(an):
    cs, chans, _ = _range_set()
    rg1_rates = (96000, 48000, 44100, 22050, 11025, 8000)
    pick = [i for i, c in enumerate(cs) if c[2] in rg1_rates][:8]
    tracks = [_track(chans[i], cs[i][2]) for i in pick]
    before, hist_before = an.analyze_tracks(tracks, return_histograms=True)
    an.analyze_tracks_r128(tracks, true_peak=True, dynamics=True)
    an.set_tuning_r128(2, 2)
    an.analyze_album_r128(tracks[:3], dynamics=True)
    after, hist_after = an.analyze_tracks(tracks, return_histograms=True)
    assert np.array_equal(hist_before, hist_after) and before == after
