"""Many R 128 albums in one call (rg_r128_analyze_albums_pcm[_dynamics], rg_r128_analyze_albums[_dynamics], the node entry
points; mp3rgain_amd/csrc/rg_r128_albums.hip): every album equals the single-album call on its tracks or files as bytes of
the C records, under several hops per lane and every album selection mode; the albums against the float64 checkers
(tests/r128ref.py, tests/r128range_ref.py) within the tolerances measured on the checkers themselves; small and wide albums
in one call; album boundaries, empty albums, albums without a block, a NaN track; files under several routes, failing files;
the node; and the other paths left as they were.  tests/test_r128_albums_cpu.py holds the precondition of the comparisons
against the checkers: no block of any album's union sits within 10 x the tolerance of a gate."""
import ctypes as C
import math
import os
import struct
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import r128albums_cases as ac  # noqa: E402
import r128cases  # noqa: E402
import r128range_cases  # noqa: E402
import r128range_ref  # noqa: E402
import r128ref  # noqa: E402
import wavutil  # noqa: E402
from wavutil import wav_bytes  # noqa: E402

import mp3rgain_amd as rg  # noqa: E402
from mp3rgain_amd import _capi  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = Path(__file__).resolve().parent / "golden"
TOL = 100.0 * r128cases.load_measured()["worst_relative_block_error"]
ST_TOL = 100.0 * r128range_cases.load_measured()["worst_relative_st_error"]
TP_TOL = 2e-6
LU = 4.343  # d(10 log10 x) = 4.343 dx / x
FIELDS = ("loudness_range_lu", "range_low_lufs", "range_high_lufs", "max_momentary_lufs", "max_short_term_lufs")
_signal = wavutil.test_signal  # (not imported under its own name: pytest would collect it)


@pytest.fixture()
def an(_ctx):
    _ctx.set_kernel(0)
    for key in (1, 2, 4, 7, 10, 13):
        _ctx.set_tuning(key, 0)
    _ctx.set_tuning(14, 1)
    _ctx.set_tuning_r128(1, 0)
    _ctx.set_tuning_r128(2, 0)
    _ctx.set_decoder_command(None)
    yield _ctx
    _ctx.set_tuning_r128(1, 0)
    _ctx.set_tuning_r128(2, 0)
    for key in (7, 13):
        _ctx.set_tuning(key, 0)


def _bits(x):
    return struct.pack("<d", x)


def _dyn_bytes(d):
    if d is None:
        return b"-"
    return b"".join(_bits(getattr(d, k)) for k in FIELDS) + struct.pack("<2I", d.st_blocks, d.st_blocks_gated)


def _res_bytes(r):
    """A track's or an album's record as bytes (NaN compares equal to itself), its dynamics included."""
    head = struct.pack("<4d", r.loudness_lufs, r.gain_db, r.sample_peak, r.true_peak)
    return head + struct.pack("<4I", getattr(r, "sample_rate", 0), r.blocks, r.blocks_gated, getattr(r, "flags", 0)) + _dyn_bytes(r.dynamics)


def _album_bytes(a):
    return [_res_bytes(a)] + [_res_bytes(t) for t in a.tracks]


def _tracks(idx):
    sig = ac.signals()
    return [rg.PcmTrack(sig[i][1], sig[i][2]) for i in idx]


# ---- 1. albums equal the single-album calls ------------------------------------------------------------------------------
def _equal_single_album_calls(an, albums, **kw):
    got = an.analyze_albums_r128([_tracks(a) for a in albums], **kw)
    assert len(got) == len(albums)
    for a, g in zip(albums, got):
        want = an.analyze_album_r128(_tracks(a), **kw)
        assert _album_bytes(g) == _album_bytes(want), a
    return got


@pytest.mark.parametrize("mode", [0, 1, 2], ids=lambda m: f"select{m}")
@pytest.mark.parametrize("S", [0, 1, 7], ids=lambda s: f"S{s}")
def test_albums_equal_single_album_calls(an, S, mode):
    """62 tracks of eight rates and three formats (0 to 4 hops + 1 frame, 28 to 31 hops, one in several chunks) as albums of
    1 to 6 and two empty ones.  Selection mode 2 puts albums of 0, 1, 2, 3, 21 ... short-term blocks through the wide form:
    slices of one block and empty slices."""
    an.set_tuning_r128(1, S)
    an.set_tuning_r128(2, mode)
    for seed in ac.SEEDS:
        got = _equal_single_album_calls(an, ac.albums(seed), true_peak=True, dynamics=True)
        assert all(g.dynamics is not None and all(t.dynamics is not None for t in g.tracks) for g in got)
        if mode == 2:
            assert any(g.tracks and g.dynamics.st_blocks < 256 for g in got)  # fewer blocks than slices


def test_albums_without_dynamics_and_true_peak(an):
    got = _equal_single_album_calls(an, ac.albums(1))
    assert all(g.dynamics is None and math.isnan(g.true_peak) and all(t.dynamics is None for t in g.tracks) for g in got)
    with_tp = _equal_single_album_calls(an, ac.albums(1), true_peak=True)
    assert [(g.loudness_lufs, g.sample_peak) for g in got if g.blocks_gated] == [(g.loudness_lufs, g.sample_peak) for g in with_tp if g.blocks_gated]


# ---- 2. against the float64 checkers -------------------------------------------------------------------------------------
def _close(cid, what, got, want, tol):
    if math.isinf(want) or math.isnan(want):
        assert _bits(got) == _bits(want) or (math.isnan(got) and math.isnan(want)), (cid, what, got, want)
    else:
        assert abs(got - want) <= tol, (cid, what, got, want, tol)


def _check_blocks(cid, got, want, gate, tol):
    assert len(got) == len(want), cid
    if len(want):
        above = want >= gate
        err_above = float(np.max(np.abs(got[above] - want[above]) / want[above])) if np.any(above) else 0.0
        err_below = float(np.max(np.abs(got[~above] - want[~above]))) / gate if np.any(~above) else 0.0
        print(f"  {cid}: worst block error {err_above:.2e} above the gate, {err_below:.2e} of the gate below it (bar {tol:.2e})")
        assert err_above <= tol and err_below <= tol, (cid, err_above, err_below)


def _check_loudness(cid, r, ref):
    assert (r.blocks, r.blocks_gated) == (ref["blocks"], ref["blocks_gated"]), cid
    if ref["loudness_lufs"] == -math.inf:
        assert r.loudness_lufs == -math.inf and r.gain_db == 0.0, cid
    else:
        assert abs(r.loudness_lufs - ref["loudness_lufs"]) <= LU * TOL + 1e-12, cid
        assert abs(r.gain_db - (-18.0 - r.loudness_lufs)) <= 1e-12, cid
    assert r.sample_peak == ref["sample_peak"], cid
    assert abs(r.true_peak - ref["true_peak"]) <= TP_TOL * ref["true_peak"], (cid, r.true_peak, ref["true_peak"])


def _check_dynamics(cid, d, ref):
    assert (d.st_blocks, d.st_blocks_gated) == (ref["st_blocks"], ref["st_blocks_gated"]), cid
    _close(cid, "lra", d.loudness_range_lu, ref["loudness_range_lu"], 2.0 * LU * ST_TOL)
    for k in FIELDS[1:]:
        _close(cid, k, getattr(d, k), ref[k], LU * ST_TOL)


def test_albums_against_the_checkers(an):
    sig = ac.signals()
    albums = ac.albums(1)
    got, blocks, st = an.analyze_albums_r128([_tracks(a) for a in albums], true_peak=True, dynamics=True, return_blocks=True,
                                             return_short_term=True)
    for q, (a, g, zs, ss) in enumerate(zip(albums, got, blocks, st)):
        pairs = [(sig[i][1], sig[i][2]) for i in a]
        ref_tracks, ref_album = r128ref.analyze_album(pairs, True)
        dyn_tracks, dyn_album = r128range_ref.analyze_album(pairs)
        print(f"album {q} {a}: {g.loudness_lufs:.6f} LUFS (ref {ref_album['loudness_lufs']:.6f}), LRA {g.dynamics.loudness_range_lu:.6f} LU "
              f"(ref {dyn_album['loudness_range_lu']:.6f}), blocks {g.blocks} / {g.dynamics.st_blocks}")
        _check_loudness(f"album-{q}", g, ref_album)
        _check_dynamics(f"album-{q}", g.dynamics, dyn_album)
        assert len(g.tracks) == len(zs) == len(ss) == len(a)
        for i, t, z, s, rt, dt in zip(a, g.tracks, zs, ss, ref_tracks, dyn_tracks):
            _check_blocks(sig[i][0], z, rt["z"], r128ref.ABS_GATE, TOL)
            _check_blocks(sig[i][0] + "-st", s, dt["st"], r128range_ref.ABS_GATE, ST_TOL)
            _check_loudness(sig[i][0], t, rt)
            _check_dynamics(sig[i][0], t.dynamics, dt)
            assert t.sample_rate == sig[i][2] and t.flags == 0


# ---- 3. forms chosen by size in one call ---------------------------------------------------------------------------------
def test_small_and_wide_albums_in_one_call(an):
    """Two albums of more than 16384 short-term blocks each (13 of the 26 long tracks of the large album, and half of the
    rest) and three small ones before, between and after them: under the library's own choice the large ones take the wide
    passes and the small ones a workgroup each, in the same call."""
    cs = r128range_cases.range_cases()
    ids = [c[0] for c in cs]
    chans = {}
    large = r128range_cases.large_album_ids()
    for i in set(large):
        c = cs[ids.index(i)]
        chans[i] = (r128range_cases.make(*c[1:]), c[2])
    small = [(ch, rate) for ch, rate, _, _ in r128range_cases.album_tracks()]
    halves = [large[:13] + large[26:28], large[13:26] + large[28:]]
    pcm = [small[:2]] + [[chans[i] for i in halves[0]]] + [small[2:]] + [[chans[i] for i in halves[1]]] + [small]
    albums = [[rg.PcmTrack(ch, rate) for ch, rate in a] for a in pcm]
    refs = {i: r128range_ref.analyze(*chans[i]) for i in set(large)}
    got = {}
    for mode in (0, 1, 2):
        an.set_tuning_r128(2, mode)
        got[mode] = an.analyze_albums_r128(albums, true_peak=True, dynamics=True)
        for a, g in zip(albums, got[mode]):
            assert _album_bytes(g) == _album_bytes(an.analyze_album_r128(a, true_peak=True, dynamics=True)), mode
    assert [_album_bytes(g) for g in got[0]] == [_album_bytes(g) for g in got[1]] == [_album_bytes(g) for g in got[2]]
    for q, half in ((1, halves[0]), (3, halves[1])):
        st_ref = np.concatenate([refs[i]["st"] for i in half])
        want = r128range_ref.loudness_range(st_ref)
        want.update(max_momentary_lufs=max(refs[i]["max_momentary_lufs"] for i in half),
                    max_short_term_lufs=max(refs[i]["max_short_term_lufs"] for i in half))
        assert want["st_blocks"] > 16384
        for gate in (r128range_ref.ABS_GATE, want["thr"]):
            assert float(np.min(np.abs(st_ref - gate) / gate)) > 10.0 * ST_TOL
        _check_dynamics(f"large-{q}", got[0][q].dynamics, want)
    assert all(got[0][q].dynamics.st_blocks < 16384 for q in (0, 2, 4))


# ---- 4. album boundaries -------------------------------------------------------------------------------------------------
def _boundary_tracks():
    rate = 48000
    rng = np.random.default_rng(0xA1B)
    loud = [(0.25 * rng.standard_normal(6 * rate)).astype(np.float32) for _ in range(2)]
    mid = [(0.08 * rng.standard_normal(4 * rate + 100)).astype(np.float32) for _ in range(2)]
    quiet = [(0.0125 * rng.standard_normal(5 * rate)).astype(np.float32) for _ in range(2)]  # under the album's relative gate
    return [rg.PcmTrack(c, rate) for c in (loud, mid, quiet)]


def test_album_boundaries(an):
    loud, mid, quiet = _boundary_tracks()
    two = an.analyze_albums_r128([[loud], [quiet]], true_peak=True, dynamics=True)
    one = an.analyze_albums_r128([[loud, quiet]], true_peak=True, dynamics=True)
    assert len(two) == 2 and len(one) == 1
    assert two[1].blocks_gated == two[1].blocks > 0 and one[0].blocks_gated == two[0].blocks_gated  # the quiet track: gated out of the union
    assert abs(two[1].loudness_lufs - one[0].loudness_lufs) > 10.0 and one[0].blocks == two[0].blocks + two[1].blocks
    assert [_res_bytes(t) for t in one[0].tracks] == [_res_bytes(two[0].tracks[0]), _res_bytes(two[1].tracks[0])]
    # one album of all: the single-album entry point, byte for byte on the C records
    lib = _capi.load()
    tracks = [loud, mid, quiet]
    arena, descs = rg.replaygain.pack_tracks(tracks)
    n = len(tracks)
    first = (C.c_size_t * 2)(0, n)
    out, alb, dyn, adyn = (_capi.R128TrackResult * n)(), (_capi.R128AlbumResult * 1)(), (_capi.R128Dynamics * n)(), (_capi.R128Dynamics * 1)()
    out1, alb1, dyn1, adyn1 = (_capi.R128TrackResult * n)(), _capi.R128AlbumResult(), (_capi.R128Dynamics * n)(), _capi.R128Dynamics()
    assert lib.rg_r128_analyze_albums_pcm_dynamics(an._ctx, descs, n, first, 1, arena.ctypes.data, arena.nbytes, 0, 1, out, alb, None,
                                                   dyn, adyn, None) == 0
    assert lib.rg_r128_analyze_album_pcm_dynamics(an._ctx, descs, n, arena.ctypes.data, arena.nbytes, 0, 1, out1, C.byref(alb1), None,
                                                  dyn1, C.byref(adyn1), None) == 0
    assert (bytes(out), bytes(alb), bytes(dyn), bytes(adyn)) == (bytes(out1), bytes(alb1), bytes(dyn1), bytes(adyn1))
    # no albums at all, and albums without tracks
    assert lib.rg_r128_analyze_albums_pcm_dynamics(an._ctx, None, 0, (C.c_size_t * 1)(0), 0, None, 0, 0, 1, None, None, None, None, None,
                                                   None) == 0
    assert lib.rg_r128_analyze_albums_pcm(an._ctx, None, 0, None, 0, None, 0, 0, 0, None, None, None) == 0
    assert an.analyze_albums_r128([]) == []
    for kw in ({}, {"true_peak": True, "dynamics": True}):
        empty = an.analyze_album_r128([], **kw)
        assert [_album_bytes(g) for g in an.analyze_albums_r128([[], [], []], **kw)] == [_album_bytes(empty)] * 3
    # the same call twice: identical bytes
    again = an.analyze_albums_r128([[loud], [quiet]], true_peak=True, dynamics=True)
    assert [_album_bytes(g) for g in again] == [_album_bytes(g) for g in two]


def test_albums_without_a_block_and_with_a_nan_track(an):
    rate = 44100
    rng = np.random.default_rng(5)
    shorts = [rg.PcmTrack([(0.2 * rng.standard_normal(k)).astype(np.float32)] * 2, rate) for k in (0, 4409, 3 * 4410, 4 * 4410 - 1)]
    good = [rg.PcmTrack([(0.1 * rng.standard_normal(5 * rate)).astype(np.float32) for _ in range(2)], rate) for _ in range(3)]
    bad_ch = [c.copy() for c in good[1].channels]
    bad_ch[1][rate + 17] = np.nan
    bad = rg.PcmTrack(bad_ch, rate)
    albums = [[good[0]], shorts, [good[1], bad, good[2]], [good[2], good[0]]]
    got = an.analyze_albums_r128(albums, true_peak=True, dynamics=True)
    g = got[1]  # tracks shorter than four hops: no block
    assert (g.blocks, g.blocks_gated, g.loudness_lufs, g.gain_db) == (0, 0, -math.inf, 0.0) and g.sample_peak > 0.0
    assert g.dynamics.st_blocks == 0 and g.dynamics.max_momentary_lufs == -math.inf and g.dynamics.loudness_range_lu == 0.0
    g = got[2]  # a track that is not finite
    assert math.isnan(g.loudness_lufs) and math.isnan(g.gain_db) and g.tracks[1].flags == 1 and g.tracks[0].flags == 0
    assert all(math.isnan(getattr(g.dynamics, k)) for k in FIELDS) and g.dynamics.st_blocks_gated == 0 and g.dynamics.st_blocks == 3 * 21
    assert math.isfinite(g.sample_peak) and math.isfinite(g.tracks[0].loudness_lufs)
    for a, g in zip(albums, got):
        assert _album_bytes(g) == _album_bytes(an.analyze_album_r128(a, true_peak=True, dynamics=True))
    without = an.analyze_albums_r128([albums[0], albums[1], albums[3]], true_peak=True, dynamics=True)
    assert [_album_bytes(g) for g in without] == [_album_bytes(got[i]) for i in (0, 1, 3)]


# ---- 5. files ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def mixed(tmp_path_factory):
    """MP3 goldens, the undamaged FLAC fixtures (the 192 kHz ones too: R 128 takes them), synthesized WAVs at several rates."""
    d = tmp_path_factory.mktemp("r128_albums_mixed")
    files = sorted((GOLDEN / "mp3").glob("*.mp3")) + sorted((GOLDEN / "fixtures").glob("test_*.mp3"))
    files += [f for f in sorted((GOLDEN / "flac").glob("*.flac")) if not f.name.startswith("damaged_")]
    for k, (rate, nch, kind) in enumerate([(44100, 2, "s16"), (48000, 1, "f32"), (22050, 2, "s24"), (96000, 2, "s16"),
                                           (8000, 1, "u8"), (32000, 2, "s32"), (88200, 1, "s16"), (16000, 2, "f32")]):
        frames = int(rate * (0.4 + 0.15 * k))
        f = d / f"w{k}_{rate}_{nch}.wav"
        f.write_bytes(wav_bytes(_signal(kind, rate, frames, nch, 100 + k), rate, kind))
        files.append(f)
    assert any("192k" in f.name for f in files)
    return files


def _same_as_per_album_files(an, albums, got, **kw):
    assert len(got) == len(albums)
    for files, g in zip(albums, got):
        try:
            want = an.analyze_album_files_r128(files, **kw)
        except rg.ReplayGainError as e:
            assert isinstance(g, rg.ReplayGainError), files
            assert (g.code, str(g)) == (e.code, str(e))
            continue
        assert isinstance(g, rg.R128AlbumResult), (files, g)
        assert _album_bytes(g) == _album_bytes(want), files


ROUTES = {"default": {}, "small_groups": {13: 3 << 20}, "one_file_groups": {13: 1}, "one_loader": {7: 1}}


@pytest.mark.parametrize("route", list(ROUTES))
def test_files_albums_equal_per_album_calls(an, mixed, route):
    """one_file_groups: every album with several files straddles groups and is gated from several energy buffers."""
    for key, value in ROUTES[route].items():
        an.set_tuning(key, value)
    for seed in ac.SEEDS:
        albums = ac.partition(mixed, seed)
        got = an.analyze_albums_files_r128(albums, true_peak=True, dynamics=True)
        assert all(isinstance(g, rg.R128AlbumResult) for g in got)
        _same_as_per_album_files(an, albums, got, true_peak=True, dynamics=True)
    plain = an.analyze_albums_files_r128(ac.partition(mixed, 1))
    _same_as_per_album_files(an, ac.partition(mixed, 1), plain)
    assert all(g.dynamics is None for g in plain)


def _raw_call(lib, ctx, albums, want_tp=1, dynamics=True, fn=None):
    flat = [os.fsencode(str(f)) for a in albums for f in a]
    first = [0]
    for a in albums:
        first.append(first[-1] + len(a))
    n, na = len(flat), len(albums)
    paths = (C.c_char_p * max(1, n))(*flat)
    fa = (C.c_size_t * (na + 1))(*first)
    out, st = (_capi.R128TrackResult * max(1, n))(), (C.c_int32 * max(1, n))()
    alb, ast = (_capi.R128AlbumResult * max(1, na))(), (C.c_int32 * max(1, na))()
    dyn, adyn = (_capi.R128Dynamics * max(1, n))(), (_capi.R128Dynamics * max(1, na))()
    if dynamics:
        rc = (fn or lib.rg_r128_analyze_albums_dynamics)(ctx, paths, n, fa, na, -1, want_tp, out, st, alb, ast, dyn, adyn)
    else:
        rc = (fn or lib.rg_r128_analyze_albums)(ctx, paths, n, fa, na, -1, want_tp, out, st, alb, ast)
    return rc, first, flat, out, st, alb, ast, dyn, adyn


def test_files_raw_results_and_empty_albums(an, mixed):
    lib = _capi.load()
    albums = [[], mixed[:3], [], mixed[3:4], []]
    rc, first, flat, out, st, alb, ast, dyn, adyn = _raw_call(lib, an._ctx, albums)
    n = len(flat)
    assert rc == 0 and list(st)[:n] == [0] * n and list(ast) == [0] * 5
    empty, empty_dyn = _capi.R128AlbumResult(), _capi.R128Dynamics()
    none, none_dyn = (_capi.R128TrackResult * 1)(), (_capi.R128Dynamics * 1)()
    assert lib.rg_r128_analyze_album_dynamics(an._ctx, (C.c_char_p * 1)(), 0, -1, 1, none, C.byref(empty), none_dyn, C.byref(empty_dyn)) == 0
    for a in (0, 2, 4):
        assert bytes(alb[a]) == bytes(empty) and bytes(adyn[a]) == bytes(empty_dyn)
    for a in (1, 3):
        k = first[a + 1] - first[a]
        one, one_dyn = _capi.R128AlbumResult(), _capi.R128Dynamics()
        tr, td = (_capi.R128TrackResult * k)(), (_capi.R128Dynamics * k)()
        assert lib.rg_r128_analyze_album_dynamics(an._ctx, (C.c_char_p * k)(*flat[first[a]:first[a + 1]]), k, -1, 1, tr, C.byref(one), td,
                                                  C.byref(one_dyn)) == 0
        assert bytes(alb[a]) == bytes(one) and bytes(adyn[a]) == bytes(one_dyn)
        assert [bytes(out[i]) + bytes(dyn[i]) for i in range(first[a], first[a + 1])] == [bytes(t) + bytes(d) for t, d in zip(tr, td)]
    rc, *_ = _raw_call(lib, an._ctx, [])
    assert rc == 0


# ---- 6. failures ---------------------------------------------------------------------------------------------------------
def _raw_wav(tag, bits, body, rate=44100, nch=2):
    align = nch * bits // 8
    fmt = struct.pack("<HHIIHH", tag, nch, rate, rate * align, align, bits)
    chunks = b"fmt " + struct.pack("<I", len(fmt)) + fmt + b"data" + struct.pack("<I", len(body)) + body
    return b"RIFF" + struct.pack("<I", 4 + len(chunks)) + b"WAVE" + chunks


@pytest.mark.parametrize("route", ["default", "one_file_groups"])
def test_failing_file_ends_its_album_only(an, mixed, tmp_path, route):
    for key, value in ROUTES[route].items():
        an.set_tuning(key, value)
    missing = tmp_path / "missing.flac"
    f64 = tmp_path / "float64.wav"  # parses, passes every per-file check, but no de-interleave reads it
    f64.write_bytes(_raw_wav(3, 64, (0.25 * np.sin(np.arange(2 * 20000) / 9.0)).astype("<f8").tobytes()))
    low = tmp_path / "low.wav"
    low.write_bytes(wav_bytes(_signal("s16", 4000, 9000, 2, 9), 4000, "s16"))
    albums = ac.partition(mixed, 11, max_album=5, empty=False)
    assert len(albums) >= 8
    albums[1].insert(1, missing)
    albums[4].insert(0, low)
    albums[4].append(missing)  # a later failure does not replace the first
    albums[5].insert(1, f64)
    got = an.analyze_albums_files_r128(albums, true_peak=True, dynamics=True)
    codes = {1: -8, 4: -2, 5: -9}
    assert str(got[5]) == f"Failed to probe format: {f64}" and "Unsupported sample rate: 4000 Hz" in str(got[4])
    assert all(isinstance(g, rg.R128AlbumResult) for a, g in enumerate(got) if a not in codes)
    for a, code in codes.items():
        assert isinstance(got[a], rg.ReplayGainError) and got[a].code == code
    _same_as_per_album_files(an, albums, got, true_peak=True, dynamics=True)
    # the good files of a failed album keep their results, every file's status and text are those of the track call
    lib = _capi.load()
    rc, first, flat, out, st, alb, ast, dyn, adyn = _raw_call(lib, an._ctx, albums)
    assert rc == 0
    texts = [lib.rg_tracks_error(an._ctx, i).decode() for i in range(len(flat))]
    assert [ast[a] for a in range(len(albums))] == [codes.get(a, 0) for a in range(len(albums))]
    zero_alb, zero_dyn = bytes(_capi.R128AlbumResult()), bytes(_capi.R128Dynamics())
    assert all(bytes(alb[a]) == zero_alb and bytes(adyn[a]) == zero_dyn for a in codes)
    want = an.analyze_track_files_r128([f for a in albums for f in a], true_peak=True, dynamics=True)
    for i, w in enumerate(want):
        if isinstance(w, rg.ReplayGainError):
            assert (st[i], texts[i]) == (w.code, str(w)), flat[i]
        else:
            assert st[i] == 0 and _res_bytes(rg.replaygain._to_r128(out[i], rg.AudioFileType.Mp3, dyn[i])) == _res_bytes(w), flat[i]
    assert sum(1 for w in want if isinstance(w, rg.ReplayGainError)) == 4


@pytest.mark.parametrize("first, n_albums", [(None, 1), ([1, 2], 1), ([0, 1], 1), ([0, 2, 1, 2], 3)])
def test_malformed_album_first_is_refused(an, mixed, first, n_albums):
    lib = _capi.load()
    paths = (C.c_char_p * 2)(*[os.fsencode(str(f)) for f in mixed[:2]])
    fa = (C.c_size_t * len(first))(*first) if first is not None else None
    out, st = (_capi.R128TrackResult * 2)(), (C.c_int32 * 2)(7, 7)
    alb, ast = (_capi.R128AlbumResult * 3)(), (C.c_int32 * 3)(7, 7, 7)
    dyn, adyn = (_capi.R128Dynamics * 2)(), (_capi.R128Dynamics * 3)()
    for buf in (out, alb, dyn, adyn):
        C.memset(buf, 0x5A, C.sizeof(buf))
    before = [bytes(b) for b in (out, st, alb, ast, dyn, adyn)]
    assert lib.rg_r128_analyze_albums(an._ctx, paths, 2, fa, n_albums, -1, 1, out, st, alb, ast) == _capi.RG_ERR_INVALID_ARG
    assert lib.rg_last_error(an._ctx).decode().startswith("rg_r128_analyze_albums: ")
    assert lib.rg_r128_analyze_albums_dynamics(an._ctx, paths, 2, fa, n_albums, -1, 1, out, st, alb, ast, dyn, adyn) == _capi.RG_ERR_INVALID_ARG
    assert lib.rg_last_error(an._ctx).decode().startswith("rg_r128_analyze_albums_dynamics: ")
    arena, descs = rg.replaygain.pack_tracks(_boundary_tracks()[:2])
    assert lib.rg_r128_analyze_albums_pcm(an._ctx, descs, 2, fa, n_albums, arena.ctypes.data, arena.nbytes, 0, 1, out, alb, None) == _capi.RG_ERR_INVALID_ARG
    assert lib.rg_last_error(an._ctx).decode().startswith("rg_r128_analyze_albums_pcm: ")
    assert lib.rg_r128_analyze_albums_pcm_dynamics(an._ctx, descs, 2, fa, n_albums, arena.ctypes.data, arena.nbytes, 0, 1, out, alb, None, dyn,
                                                   adyn, None) == _capi.RG_ERR_INVALID_ARG
    assert lib.rg_last_error(an._ctx).decode().startswith("rg_r128_analyze_albums_pcm_dynamics: ")
    assert [bytes(b) for b in (out, st, alb, ast, dyn, adyn)] == before


# ---- 7. node -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("devices", [[0, 0], [0, 0, 0]], ids=lambda d: f"{len(d)}ctx")
def test_node_equals_the_single_context(an, mixed, tmp_path, devices):
    albums = ac.partition(mixed, 21)
    albums[2] = albums[2] + [tmp_path / "missing.flac"]
    flat = [f for a in albums for f in a]
    single = an.analyze_albums_files_r128(albums, true_peak=True, dynamics=True)
    single_plain = an.analyze_albums_files_r128(albums)
    single_tracks = an.analyze_track_files_r128(flat, true_peak=True, dynamics=True)
    with rg.Node(devices) as node:
        node.set_tuning(14, 1)
        got = node.analyze_albums_files_r128(albums, true_peak=True, dynamics=True)
        own = node.last_partition(len(flat))
        got_plain = node.analyze_albums_files_r128(albums)
        got_tracks = node.analyze_track_files_r128(flat, true_peak=True, dynamics=True)
        own_tracks = node.last_partition(len(flat))
        got_tracks_plain = node.analyze_track_files_r128(flat)
    for g_all, s_all in ((got, single), (got_plain, single_plain)):
        assert len(g_all) == len(s_all)
        for g, s in zip(g_all, s_all):
            if isinstance(s, rg.ReplayGainError):
                assert isinstance(g, rg.ReplayGainError) and (g.code, str(g)) == (s.code, str(s))
            else:
                assert _album_bytes(g) == _album_bytes(s)
    assert isinstance(single[2], rg.ReplayGainError) and sum(isinstance(s, rg.ReplayGainError) for s in single) == 1
    k = 0
    for a in albums:  # every file of an album on one device, every context had work
        assert len(set(own[k:k + len(a)])) <= 1
        k += len(a)
    assert set(own) == set(range(len(devices))) == set(own_tracks)
    for g, s, p in zip(got_tracks, single_tracks, got_tracks_plain):
        if isinstance(s, rg.ReplayGainError):
            assert (g.code, str(g)) == (s.code, str(s)) == (p.code, str(p))
        else:
            assert _res_bytes(g) == _res_bytes(s) and p.dynamics is None and p.loudness_lufs == s.loudness_lufs


def test_backend_node_has_no_r128_entries(mixed):
    from test_node_cpu import FakeEngines

    lib = _capi.load()
    fe = FakeEngines()
    with rg.Node([0, 1], _backend=fe.table) as node:
        with pytest.raises(rg.ReplayGainError) as e:
            node.analyze_albums_files_r128([mixed[:2]], dynamics=True)
        assert e.value.code == _capi.RG_ERR_STATE and "rg_r128_analyze_albums_node" in str(e.value)
        with pytest.raises(rg.ReplayGainError) as e:
            node.analyze_track_files_r128(mixed[:2])
        assert e.value.code == _capi.RG_ERR_STATE and "rg_r128_analyze_tracks_node" in str(e.value)
    assert not fe.calls and lib is not None


# ---- 8. nothing else moved -----------------------------------------------------------------------------------------------
def test_other_paths_unchanged_around_an_albums_call(an):
    sig = ac.signals()
    rg1_rates = (96000, 48000, 44100, 22050, 11025, 8000)
    pick = [i for i, s in enumerate(sig) if s[2] in rg1_rates and len(s[1][0]) > 0][:8]
    tracks = _tracks(pick)
    before, hist_before = an.analyze_tracks(tracks, return_histograms=True)
    r128_before = an.analyze_tracks_r128(tracks, true_peak=True, dynamics=True)
    album_before = an.analyze_album_r128(tracks[:4], true_peak=True, dynamics=True)
    an.analyze_albums_r128([tracks[:3], [], tracks[3:]], true_peak=True, dynamics=True)
    an.set_tuning_r128(2, 2)
    an.analyze_albums_r128([tracks[:5], tracks[5:]], dynamics=True)
    an.set_tuning_r128(2, 0)
    after, hist_after = an.analyze_tracks(tracks, return_histograms=True)
    assert np.array_equal(hist_before, hist_after) and before == after
    assert [_res_bytes(r) for r in an.analyze_tracks_r128(tracks, true_peak=True, dynamics=True)] == [_res_bytes(r) for r in r128_before]
    assert _album_bytes(an.analyze_album_r128(tracks[:4], true_peak=True, dynamics=True)) == _album_bytes(album_before)
