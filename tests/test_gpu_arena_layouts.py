"""Every kernel that reads PCM -- the transient-moment main kernel, the halo kernel, rg_peak_all_kernel, the R 128 main
kernel and the R 128 true-peak kernel -- against arena layouts `replaygain.pack_tracks` never produces, through the C ABI
directly: any sample-aligned offset residue modulo 128, tracks that abut, are stored back to front or share one copy, a
caller's device pointer as base, and guard samples around every track (tests/arena_layouts.py) that are at least 128 times
any sample of the quiet tracks (tests/layout_cases.py), so that one sample consumed from outside a track shows.

Results in every layout are held bit for bit to the canonical run (`pack_tracks`' layout) of the same kernel column / the same
hops per lane; the canonical run is held to the oracle (ReplayGain 1.0: exactly) and to the float64 checker (R 128: within
100 x the checker's own error against np.longdouble on exactly these tracks, tests/golden/r128_layout_measured.json,
tools/r128_refcheck.py --layout-cases).  No bar here comes from the GPU's output."""
import ctypes as C
import math
import struct
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import arena_layouts as al  # noqa: E402
import layout_cases  # noqa: E402
import r128ref  # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 100.0 * layout_cases.load_measured()["worst_relative_block_error"]
# true peak, f32 kernel: 14 roundings of 2^-24 (13 fused multiply-adds + the table's f32 rounding) x 2.31 (largest per-phase sum
# of |h|, F = 2) x max|x| <= true peak (the derivation of tests/test_gpu_r128.py)
TP_TOL = 2e-6
IMPRECISE, NONFINITE = 2, 1
LAYOUTS = {"abut": al.Layout("abut", "loud", "input"), "guard-loud": al.Layout("guard", "loud", "input"),
           "guard-nan": al.Layout("guard", "nan", "input", 1), "reversed": al.Layout("guard", "loud", "reversed", 2),
           "aliased": al.Layout("guard", "loud", "aliased", 4)}
_CACHE = {}


def _lib():
    from mp3rgain_amd import _capi

    return _capi, _capi.load()


def _tracks(cases):
    import mp3rgain_amd as rg

    made = {}
    rep = layout_cases.with_repeats(cases)  # the same PcmTrack objects again: an aliased layout stores them once
    tr = [made.setdefault(c[0], rg.PcmTrack(c[1], c[2])) for c in rep]
    ids = [c[0] + ("-again" if i >= len(cases) else "") for i, c in enumerate(rep)]
    return ids, tr


def _bits(x):
    return struct.pack("<d", x)


# ---- ReplayGain 1.0 ----------------------------------------------------------------------------------------------------------
def _rg1_set(oracle):
    if "rg1" not in _CACHE:
        ids, tr = _tracks(layout_cases.rg1_cases())
        refs = [oracle.analyze_pcm(t.channels[0], t.channels[1] if len(t.channels) > 1 else None, t.sample_rate) for t in tr]
        _CACHE["rg1"] = (ids, tr, refs)
    return _CACHE["rg1"]


def _rg1_fields(r):
    return (_bits(r.loudness_db), _bits(r.gain_db), _bits(r.peak), r.sample_rate, r.gain_steps, r.windows, r.flags)


def _rg1_batch(an, base, nbytes, descs, n, on_device=0):
    capi, lib = _lib()
    out = (capi.TrackResult * n)()
    hist = np.zeros((n, capi.HISTOGRAM_SIZE), dtype=np.uint32)
    an._check(lib.rg_analyze_pcm_batch(an.handle, descs, n, base, nbytes, on_device, out, hist.ctypes.data))
    return out, hist


def _rg1_album(an, base, nbytes, descs, n, on_device=0):
    capi, lib = _lib()
    out = (capi.TrackResult * n)()
    alb = capi.AlbumResult()
    hist = np.zeros(capi.HISTOGRAM_SIZE, dtype=np.uint32)
    an._check(lib.rg_analyze_album_pcm(an.handle, descs, n, base, nbytes, on_device, out, C.byref(alb), hist.ctypes.data))
    return out, alb, hist


def _rg1_layouts(an, oracle, column, exact):
    """exact: every track must equal the oracle (the halo column and auto mode); else every track that does not carry
    RG_TRACK_FLAG_IMPRECISE must (a forced TM column: full-scale impulses in quiet noise are what that flag exists for; auto
    mode runs the same TM kernels on every track first and has no exemption)."""
    from mp3rgain_amd import replaygain

    ids, tr, refs = _rg1_set(oracle)
    n = len(tr)
    # a host arena above the ingest chunk (key 5) is streamed, and the streamed route lays every track out again at aligned
    # offsets: the default (2 GiB) keeps these arenas as they are packed
    an.set_tuning(5, 0)
    arena, descs = replaygain.pack_tracks(tr)
    canon, canon_hist = _rg1_batch(an, arena.ctypes.data, arena.nbytes, descs, n)
    c_tracks, c_alb, c_alb_hist = _rg1_album(an, arena.ctypes.data, arena.nbytes, descs, n)
    flagged = [i for i in range(n) if canon[i].flags & IMPRECISE]
    print(f"{column}: {len(flagged)} of {n} tracks flagged imprecise in the canonical layout")
    assert not exact or not flagged
    for i, (cid, (want, want_hist)) in enumerate(zip(ids, refs)):
        assert not canon[i].flags & NONFINITE and canon[i].flags == c_tracks[i].flags, cid
        if canon[i].flags & IMPRECISE:
            continue
        assert canon[i].flags == 0, cid
        assert np.array_equal(canon_hist[i], want_hist), cid
        assert canon[i].peak == want["peak"] and canon[i].loudness_db == want["loudness_db"], (cid, canon[i].peak, want["peak"])
        assert canon[i].gain_steps == want["gain_steps"] and canon[i].sample_rate == want["sample_rate"], cid
        assert canon[i].windows == int(want_hist.sum()), cid
        assert _rg1_fields(c_tracks[i]) == _rg1_fields(canon[i]), cid
    if not flagged:
        want_alb, want_alb_hist = oracle.album_from_hists([h for _, h in refs], [w["peak"] for w, _ in refs])
        assert np.array_equal(c_alb_hist, want_alb_hist)
        assert (c_alb.album_loudness_db, c_alb.album_peak) == (want_alb["album_loudness_db"], want_alb["album_peak"])
    for name, layout in LAYOUTS.items():
        arena, descs, _ = al.pack(tr, layout)
        got, hist = _rg1_batch(an, arena.ctypes.data, arena.nbytes, descs, n)
        a_tracks, a_alb, a_hist = _rg1_album(an, arena.ctypes.data, arena.nbytes, descs, n)
        for i, cid in enumerate(ids):  # no exemption: bit for bit the canonical run of the same column
            assert _rg1_fields(got[i]) == _rg1_fields(canon[i]), (column, name, cid, got[i].peak, canon[i].peak, got[i].flags)
            assert np.array_equal(hist[i], canon_hist[i]), (column, name, cid)
            assert _rg1_fields(a_tracks[i]) == _rg1_fields(c_tracks[i]), (column, name, cid, "album")
        assert np.array_equal(a_hist, c_alb_hist), (column, name)
        assert (_bits(a_alb.album_loudness_db), _bits(a_alb.album_gain_db), _bits(a_alb.album_peak), a_alb.album_gain_steps,
                a_alb.windows) == (_bits(c_alb.album_loudness_db), _bits(c_alb.album_gain_db), _bits(c_alb.album_peak),
                                   c_alb.album_gain_steps, c_alb.windows), (column, name)


def test_rg1_layouts(analyzer, oracle, request):
    column = request.node.callspec.id
    _rg1_layouts(analyzer, oracle, column, exact=column == "halo")


def test_rg1_layouts_auto_mode(_ctx, oracle):
    _ctx.set_kernel(0)
    for key in (1, 2, 4):
        _ctx.set_tuning(key, 0)
    _rg1_layouts(_ctx, oracle, "auto", exact=True)


# ---- EBU R 128 ---------------------------------------------------------------------------------------------------------------
@pytest.fixture()
def an(_ctx):
    _ctx.set_kernel(0)
    for key in (1, 2, 4, 5):  # 5: the default ingest chunk, so that no host arena here is streamed and laid out again
        _ctx.set_tuning(key, 0)
    _ctx.set_tuning_r128(1, 0)
    yield _ctx
    _ctx.set_tuning_r128(1, 0)


def _r128_set():
    if "r128" not in _CACHE:
        ids, tr = _tracks(layout_cases.r128_cases())
        refs = [r128ref.analyze(t.channels, t.sample_rate, True) for t in tr]
        _CACHE["r128"] = (ids, tr, refs)
    return _CACHE["r128"]


def _r128_call(an, tr, base, nbytes, descs, mode, on_device=0):
    """mode: "batch" | "album" | "dynamics" -> a dict of everything the call returns, structs as bytes."""
    capi, lib = _lib()
    n = len(tr)
    out = (capi.R128TrackResult * n)()
    counts = [int(lib.rg_r128_block_count(t.sample_rate, t.frames)) for t in tr]
    z = np.zeros(max(1, sum(counts)), dtype=np.float64)
    res = {"counts": counts}
    if mode == "batch":
        an._check(lib.rg_r128_analyze_pcm_batch(an.handle, descs, n, base, nbytes, on_device, 1, out, z.ctypes.data))
    elif mode == "album":
        alb = capi.R128AlbumResult()
        an._check(lib.rg_r128_analyze_album_pcm(an.handle, descs, n, base, nbytes, on_device, 1, out, C.byref(alb), z.ctypes.data))
        res["album"] = bytes(alb)
        res["album_struct"] = alb
    else:
        st_counts = [int(lib.rg_r128_short_term_count(t.sample_rate, t.frames)) for t in tr]
        st = np.zeros(max(1, sum(st_counts)), dtype=np.float64)
        dyn = (capi.R128Dynamics * n)()
        an._check(lib.rg_r128_analyze_pcm_batch_dynamics(an.handle, descs, n, base, nbytes, on_device, 1, out, z.ctypes.data, dyn,
                                                         st.ctypes.data))
        res["dyn"] = [bytes(dyn[i]) for i in range(n)]
        res["st"] = st.tobytes()
        res["st_count"] = sum(st_counts)
    res["out"] = out
    res["tracks"] = [bytes(out[i]) for i in range(n)]
    res["z"] = z
    return res


def _r128_same(got, want, ids, what):
    for i, cid in enumerate(ids):
        assert got["tracks"][i] == want["tracks"][i], (what, cid, got["out"][i].sample_peak, want["out"][i].sample_peak,
                                                        got["out"][i].true_peak, want["out"][i].true_peak, got["out"][i].flags)
    assert got["z"].tobytes() == want["z"].tobytes(), what
    for key in ("album", "dyn", "st"):
        assert got.get(key) == want.get(key), (what, key)


def _r128_against_the_checker(ids, tr, refs, got):
    p, worst_above, worst_below = 0, 0.0, 0.0
    for cid, t, ref, r, k in zip(ids, tr, refs, got["out"], got["counts"]):
        z, zr = got["z"][p:p + k], ref["z"]
        p += k
        assert k == len(zr) == r.blocks == ref["blocks"], cid
        if k:
            above = zr >= r128ref.ABS_GATE
            err_above = float(np.max(np.abs(z[above] - zr[above]) / zr[above])) if np.any(above) else 0.0
            err_below = float(np.max(np.abs(z[~above] - zr[~above]))) / r128ref.ABS_GATE if np.any(~above) else 0.0
            worst_above, worst_below = max(worst_above, err_above), max(worst_below, err_below)
            assert err_above <= TOL and err_below <= TOL, (cid, err_above, err_below, TOL)
        assert r.blocks_gated == ref["blocks_gated"], cid
        if ref["loudness_lufs"] == -math.inf:
            assert r.loudness_lufs == -math.inf and r.gain_db == 0.0, cid
        else:
            assert abs(r.loudness_lufs - ref["loudness_lufs"]) <= 4.343 * TOL, cid
        assert r.sample_peak == ref["sample_peak"], (cid, r.sample_peak, ref["sample_peak"])
        assert abs(r.true_peak - ref["true_peak"]) <= TP_TOL * ref["true_peak"], (cid, r.true_peak, ref["true_peak"])
        assert r.sample_rate == t.sample_rate and r.flags == 0, cid
    return worst_above, worst_below


@pytest.mark.parametrize("S", [0, 1, 5, 64], ids=lambda s: f"S{s}")
def test_r128_layouts(an, S):
    """The lane assignment depends on the hop counts and on S, not on addresses: every layout gives the canonical run's bits."""
    from mp3rgain_amd import replaygain

    ids, tr, refs = _r128_set()
    an.set_tuning_r128(1, S)
    arena, descs = replaygain.pack_tracks(tr)
    canon = {mode: _r128_call(an, tr, arena.ctypes.data, arena.nbytes, descs, mode) for mode in ("batch", "album", "dynamics")}
    worst = _r128_against_the_checker(ids, tr, refs, canon["batch"])
    print(f"S = {S}: worst block error {worst[0]:.2e} relative above the gate, {worst[1]:.2e} of the gate below it (bar {TOL:.2e})")
    assert canon["dynamics"]["st_count"] > 0
    for mode in ("album", "dynamics"):  # the same per-track results and blocks, bit for bit
        assert canon[mode]["tracks"] == canon["batch"]["tracks"] and canon[mode]["z"].tobytes() == canon["batch"]["z"].tobytes(), mode
    _, ref_album = r128ref.analyze_album([(t.channels, t.sample_rate) for t in tr], True)
    alb = canon["album"]["album_struct"]
    assert (alb.blocks, alb.blocks_gated, alb.sample_peak) == (ref_album["blocks"], ref_album["blocks_gated"], ref_album["sample_peak"])
    assert abs(alb.loudness_lufs - ref_album["loudness_lufs"]) <= 4.343 * TOL
    assert abs(alb.true_peak - ref_album["true_peak"]) <= TP_TOL * ref_album["true_peak"]
    for name, layout in LAYOUTS.items():
        arena, descs, _ = al.pack(tr, layout)
        for mode in ("batch", "album") + (("dynamics",) if name == "guard-loud" else ()):
            got = _r128_call(an, tr, arena.ctypes.data, arena.nbytes, descs, mode)
            _r128_same(got, canon[mode], ids, (S, name, mode))


# ---- the device-resident route ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt", layout_cases.FORMATS)
def test_device_resident_route_equals_the_host_route(an, oracle, fmt):
    """pcm_on_device = 1 with a base that is itself only sample-aligned: the arena is uploaded k samples into a device
    buffer, so every track's absolute address moves with k.  rg_analyze_pcm_batch, rg_r128_analyze_pcm_batch and
    rg_find_peak_pcm give the bits of the host route over the same arena and of the canonical layout.  The R 128 resident
    route runs on the context's own stream: the upload is finished (synchronize) before the call."""
    import torch
    from mp3rgain_amd import replaygain

    capi, lib = _lib()
    dt = {"f32": np.float32, "s16": np.int16, "s32": np.int32}[fmt]
    bps = np.dtype(dt).itemsize
    layout = al.Layout("guard", "loud", "input", 5)
    _, tr1, _ = _rg1_set(oracle)
    _, tr2, _ = _r128_set()
    rg1 = [t for t in tr1 if t.channels[0].dtype == dt]
    r128 = [t for t in tr2 if t.channels[0].dtype == dt]
    assert len(rg1) >= 7 and len(r128) >= 7
    for tracks, which in ((rg1, "rg1"), (r128, "r128")):
        n = len(tracks)
        names = [str(i) for i in range(n)]
        c_arena, c_descs = replaygain.pack_tracks(tracks)
        arena, descs, _ = al.pack(tracks, layout)
        if which == "rg1":
            canon, canon_hist = _rg1_batch(an, c_arena.ctypes.data, c_arena.nbytes, c_descs, n, 0)
            want, want_hist = _rg1_batch(an, arena.ctypes.data, arena.nbytes, descs, n, 0)
            assert [_rg1_fields(r) for r in want] == [_rg1_fields(r) for r in canon] and np.array_equal(want_hist, canon_hist), fmt
        else:
            canon = _r128_call(an, tracks, c_arena.ctypes.data, c_arena.nbytes, c_descs, "batch", 0)
            want = _r128_call(an, tracks, arena.ctypes.data, arena.nbytes, descs, "batch", 0)
            _r128_same(want, canon, names, (fmt, "host"))
        for k in (0, 1, 3):
            sh = k * bps
            dev = torch.zeros(arena.nbytes + 16, dtype=torch.uint8, device="cuda:0")
            dev[sh:sh + arena.nbytes] = torch.from_numpy(arena).to("cuda:0")
            torch.cuda.synchronize()
            d_base = dev.data_ptr() + sh
            if which == "rg1":
                got, got_hist = _rg1_batch(an, d_base, arena.nbytes, descs, n, 1)
                assert [_rg1_fields(r) for r in got] == [_rg1_fields(r) for r in canon], (fmt, k)
                assert np.array_equal(got_hist, canon_hist), (fmt, k)
            else:
                got = _r128_call(an, tracks, d_base, arena.nbytes, descs, "batch", 1)
                _r128_same(got, canon, names, (fmt, k))
            for i, t in enumerate(tracks):
                if len(t.channels) != 3:
                    continue
                peak = oracle.find_peak(t.channels, dt)
                for base, on_device in ((arena.ctypes.data, 0), (d_base, 1)):
                    pk = capi.PeakResult()
                    an._check(lib.rg_find_peak_pcm(an.handle, C.byref(descs[i]), base, arena.nbytes, on_device, C.byref(pk)))
                    assert pk.peak == peak and pk.sample_rate == t.sample_rate, (fmt, k, on_device, pk.peak, peak)
            del dev


# ---- rg_find_peak_pcm -------------------------------------------------------------------------------------------------------
def test_find_peak_reads_every_channel_and_nothing_else(an, oracle):
    """Three quiet channels, loud guards directly before the first and behind the last: max |x| over all three, exactly."""
    import mp3rgain_amd as rg
    import torch

    capi, lib = _lib()
    for fmt in layout_cases.FORMATS:
        for frames, loud_ch in ((4097, None), (1, None), (777, 2), (778, 0)):
            ch = layout_cases.quiet(8000 + frames, frames, 3, fmt)
            if loud_ch is not None:
                layout_cases.full_scale(ch, loud_ch, (frames - 1,))
            want = oracle.find_peak(ch, ch[0].dtype)
            assert (want == 1.0) == (loud_ch is not None) and want > 0.0
            for layout in (LAYOUTS["guard-loud"], LAYOUTS["guard-nan"]):
                arena, descs, _ = al.pack([rg.PcmTrack(ch, 44100)], layout)
                dev = torch.from_numpy(arena).to("cuda:0")
                torch.cuda.synchronize()
                for base, on_device in ((arena.ctypes.data, 0), (dev.data_ptr(), 1)):
                    pk = capi.PeakResult()
                    an._check(lib.rg_find_peak_pcm(an.handle, descs, base, arena.nbytes, on_device, C.byref(pk)))
                    assert pk.peak == want and pk.peak_pcm == want * 32768.0, (fmt, frames, layout, on_device, pk.peak, want)


# ---- true peak with samples that are not finite --------------------------------------------------------------------------
def test_true_peak_with_nonfinite_samples_equals_the_checker(an):
    """The checker drops exactly the interpolator outputs a non-finite sample touches, as the kernel does: the value, not only
    its being finite and positive."""
    import mp3rgain_amd as rg
    from mp3rgain_amd import replaygain

    ch, rate = layout_cases.nonfinite_case()
    ref = r128ref.analyze(ch, rate, True)
    assert math.isfinite(ref["true_peak"]) and ref["true_peak"] > 0.0
    tr = [rg.PcmTrack(ch, rate)]
    packs = [replaygain.pack_tracks(tr)] + [al.pack(tr, LAYOUTS[name])[:2] for name in ("abut", "guard-loud", "guard-nan")]
    for arena, descs in packs:
        r = _r128_call(an, tr, arena.ctypes.data, arena.nbytes, descs, "batch")["out"][0]
        print(f"true peak {r.true_peak:.9f} (checker {ref['true_peak']:.9f}), sample peak {r.sample_peak}")
        assert r.flags == NONFINITE and math.isnan(r.loudness_lufs) and math.isnan(r.gain_db)
        assert r.sample_peak == ref["sample_peak"]
        assert abs(r.true_peak - ref["true_peak"]) <= TP_TOL * ref["true_peak"], (r.true_peak, ref["true_peak"])
