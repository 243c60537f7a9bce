"""BS.1770 channel weights on the GPU (mp3rgain_amd/csrc/rg_r128_surround.hip and the weighted route of rg_r128.hip) against
the float64 checker tests/r128surround_ref.py: EBU Tech 3341 case 6, every gating block of weighted parity signals within the
tolerance MEASURED on the checker (tests/golden/r128_measured.json), the exact identities the fold's definition gives (powers
of two, zero weights, weights of one), mixed batches in hostile arena layouts, albums, files with and without a channel mask,
a one-GPU node, the edge rules and the command line."""
import ctypes as C
import json
import math
import os
import struct
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import arena_layouts  # noqa: E402
import r128cases  # noqa: E402
import r128range_cases  # noqa: E402
import r128ref  # noqa: E402
import r128surround_ref as sref  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
FLAC6 = ROOT / "tests" / "golden" / "flac" / "s16_6ch_48k.flac"
TOL = 100.0 * r128cases.load_measured()["worst_relative_block_error"]
ST_TOL = 100.0 * r128range_cases.load_measured()["worst_relative_st_error"]
TP_TOL = 2e-6  # tests/test_gpu_r128.py: the f32 interpolator's rounding
LU = 4.343
W51 = [1.0, 1.0, 1.0, 0.0, 1.41, 1.41]
DYN_FIELDS = ("loudness_range_lu", "range_low_lufs", "range_high_lufs", "max_momentary_lufs", "max_short_term_lufs")


@pytest.fixture()
def an(_ctx):
    _ctx.set_kernel(0)
    for key in (1, 2, 4, 10, 13):
        _ctx.set_tuning(key, 0)
    _ctx.set_tuning(14, 1)
    _ctx.set_tuning_r128(1, 0)
    _ctx.set_tuning_r128(2, 0)
    _ctx.set_channel_mode_r128("pair")
    _ctx.set_decoder_command(None)
    yield _ctx
    _ctx.set_tuning_r128(1, 0)
    _ctx.set_tuning_r128(2, 0)
    _ctx.set_channel_mode_r128("pair")
    _ctx.set_tuning(13, 0)


def _track(chans, rate, weights=None):
    import mp3rgain_amd as rg

    return rg.PcmTrack(chans, rate, channel_weights=weights)


def _res_bytes(r):
    """A track's or an album's record as bytes (NaN compares equal to itself), its dynamics behind it."""
    b = struct.pack("<4d", r.loudness_lufs, r.gain_db, r.sample_peak, r.true_peak)
    b += struct.pack("<4I", getattr(r, "sample_rate", 0), r.blocks, r.blocks_gated, getattr(r, "flags", 0))
    d = r.dynamics
    if d is not None:
        b += b"".join(struct.pack("<d", getattr(d, k)) for k in DYN_FIELDS) + struct.pack("<2I", d.st_blocks, d.st_blocks_gated)
    return b


def _noise(rate, frames, nch, fmt, seed, amp=None):
    """`nch` channels of stationary noise, every channel at a level of its own."""
    rng = np.random.default_rng(seed)
    out = []
    for c in range(nch):
        a = (0.05 + 0.04 * c) if amp is None else amp[c]
        x = np.clip(a * rng.standard_normal(frames), -1.0, 1.0)
        if fmt == "f32":
            out.append(x.astype(np.float32))
        elif fmt == "s16":
            out.append(np.round(x * 32767.0).astype(np.int16))
        else:
            out.append(np.round(x * 2147483647.0).astype(np.int32))
    return out


# ---- (a) conformance: EBU Tech 3341 case 6 --------------------------------------------------------------------------------
def test_tech3341_case6(an):
    import mp3rgain_amd as rg

    rate = 48000
    chans = [c.astype(np.float32) for c in sref.tech3341_case6(rate)]
    w = rg.r128_layout_weights(5)
    assert w == [1.0, 1.0, 1.0, 1.41, 1.41]
    r = an.analyze_tracks_r128([_track(chans, rate, w)])[0]
    pair = an.analyze_tracks_r128([_track(chans, rate)])[0]
    an.set_channel_mode_r128("layout")
    by_mode = an.analyze_tracks_r128([_track(chans, rate)])[0]
    print(f"case 6: {r.loudness_lufs:.4f} LUFS with the layout's weights (expected -23.0 +- 0.1), {pair.loudness_lufs:.4f} as a pair")
    assert abs(r.loudness_lufs - (-23.0)) <= 0.1
    assert abs(r.gain_db - (-18.0 - r.loudness_lufs)) <= 1e-12
    assert abs(pair.loudness_lufs - (-28.0)) <= 0.1
    assert _res_bytes(by_mode) == _res_bytes(r)
    assert r.sample_peak == float(np.abs(chans[2]).max()) and pair.sample_peak == float(np.abs(chans[0]).max())


# ---- (b) parity per block --------------------------------------------------------------------------------------------------
_CACHE = {}


def _parity_set():
    """[(id, channels, rate, weights)] and the checker's results: 1.3 s + 5 frames = 13 hops = 10 blocks."""
    if not _CACHE:
        cases = []
        for kind, seed in (("noise", 510), ("music", 520)):
            for rate, fmt in ((8000, "s16"), (48000, "f32")):
                frames = 13 * r128cases.hop(rate) + 5
                cases.append((f"{kind}-{rate}-{fmt}-6ch", r128cases.make(kind, rate, frames, 6, fmt, seed), rate, W51))
        rate = 44100
        cases.append(("noise-44100-s32-8ch", r128cases.make("noise", rate, 13 * r128cases.hop(rate) + 5, 8, "s32", 530), rate,
                      sref.layout_weights(8)))
        _CACHE["set"] = (cases, [sref.analyze(ch, rate, w, True) for _, ch, rate, w in cases])
    return _CACHE["set"]


def test_parity_precondition_no_block_near_a_gate():
    cases, refs = _parity_set()
    for c, ref in zip(cases, refs):
        z = ref["z"]
        assert len(z) == 10, c[0]
        _, _, thr = r128ref.gate(z)
        for gate in (r128ref.ABS_GATE, thr):
            d = float(np.min(np.abs(z - gate) / gate))
            assert d > 10.0 * TOL, (c[0], gate, d)


@pytest.mark.parametrize("S", [0, 1, 4], ids=lambda s: f"S{s}")
def test_parity_per_block(an, S):
    cases, refs = _parity_set()
    an.set_tuning_r128(1, S)
    res, blocks = an.analyze_tracks_r128([_track(ch, rate, w) for _, ch, rate, w in cases], true_peak=True, return_blocks=True)
    for (cid, _, rate, _), r, z, ref in zip(cases, res, blocks, refs):
        zr = ref["z"]
        assert len(z) == len(zr) == r.blocks == ref["blocks"], cid
        above = zr >= r128ref.ABS_GATE
        err_above = float(np.max(np.abs(z[above] - zr[above]) / zr[above])) if np.any(above) else 0.0
        err_below = float(np.max(np.abs(z[~above] - zr[~above]))) / r128ref.ABS_GATE if np.any(~above) else 0.0
        print(f"{cid}: {r.loudness_lufs:.6f} LUFS (ref {ref['loudness_lufs']:.6f}), worst block error {err_above:.2e} relative above "
              f"the gate, {err_below:.2e} of the gate below it (bar {TOL:.2e}), true peak {r.true_peak:.6f} (ref {ref['true_peak']:.6f})")
        assert err_above <= TOL and err_below <= TOL, (cid, err_above, err_below)
        assert r.blocks_gated == ref["blocks_gated"], cid
        assert abs(r.loudness_lufs - ref["loudness_lufs"]) <= 4.343 * TOL + 1e-12, cid
        assert abs(r.gain_db - (-18.0 - r.loudness_lufs)) <= 1e-12, cid
        assert r.sample_peak == ref["sample_peak"], cid
        assert abs(r.true_peak - ref["true_peak"]) <= TP_TOL * ref["true_peak"], (cid, r.true_peak, ref["true_peak"])
        assert r.sample_rate == rate and r.flags == 0, cid


# ---- (c), (d), (e): what the fold's definition makes exact -----------------------------------------------------------------
def test_power_of_two_weights_scale_every_block_exactly(an):
    rate = 8000
    chans = _noise(rate, 33 * 800 + 7, 2, "f32", 601)
    plain, z1, s1 = an.analyze_tracks_r128([_track(chans, rate)], dynamics=True, return_blocks=True, return_short_term=True)
    four, z4, s4 = an.analyze_tracks_r128([_track(chans, rate, [4.0, 4.0])], dynamics=True, return_blocks=True, return_short_term=True)
    assert len(z1[0]) == 30 and len(s1[0]) == 4
    assert (4.0 * z1[0]).tobytes() == z4[0].tobytes() and (4.0 * s1[0]).tobytes() == s4[0].tobytes()
    assert abs(four[0].loudness_lufs - plain[0].loudness_lufs - 10.0 * math.log10(4.0)) <= 1e-12
    assert (four[0].blocks, four[0].blocks_gated, four[0].sample_peak) == (plain[0].blocks, plain[0].blocks_gated, plain[0].sample_peak)
    assert abs(four[0].dynamics.max_short_term_lufs - plain[0].dynamics.max_short_term_lufs - 10.0 * math.log10(4.0)) <= 1e-12


def test_zero_weight_leaves_the_pair_and_still_counts_for_peak_and_flag(an):
    rate = 8000
    chans = _noise(rate, 20 * 800 + 3, 3, "f32", 602, amp=(0.1, 0.12, 0.3))
    stereo, zs = an.analyze_tracks_r128([_track(chans[:2], rate)], true_peak=True, return_blocks=True)
    three, z3 = an.analyze_tracks_r128([_track(chans, rate, [1.0, 1.0, 0.0])], true_peak=True, return_blocks=True)
    assert zs[0].tobytes() == z3[0].tobytes() and len(z3[0]) == 17
    assert (three[0].loudness_lufs, three[0].blocks_gated) == (stereo[0].loudness_lufs, stereo[0].blocks_gated)
    pk2 = float(np.abs(chans[2]).max())
    assert pk2 > stereo[0].sample_peak and three[0].sample_peak == pk2
    assert three[0].true_peak >= pk2 * (1.0 - TP_TOL) and three[0].flags == 0
    bad = [c.copy() for c in chans]
    bad[2][5000] = np.nan
    r = an.analyze_tracks_r128([_track(bad, rate, [1.0, 1.0, 0.0]), _track(chans, rate, [1.0, 1.0, 0.0])], true_peak=True)
    assert r[0].flags == 1 and math.isnan(r[0].loudness_lufs) and math.isnan(r[0].gain_db) and r[0].sample_peak == pk2
    assert _res_bytes(r[1]) == _res_bytes(three[0])


def test_weights_of_one_take_the_existing_path(an):
    rate = 44100
    stereo = _noise(rate, 2 * rate + 11, 2, "s16", 603)
    mono = _noise(rate, 2 * rate + 11, 1, "f32", 604)
    plain = an.analyze_tracks_r128([_track(stereo, rate), _track(mono, rate)], true_peak=True, dynamics=True)
    ones = an.analyze_tracks_r128([_track(stereo, rate, [1.0, 1.0]), _track(mono, rate, [1.0])], true_peak=True, dynamics=True)
    assert [_res_bytes(r) for r in ones] == [_res_bytes(r) for r in plain]
    # entries beyond the channel count are ignored
    more = an.analyze_tracks_r128([_track(stereo, rate, [1.0, 1.0, 7.0, math.nan]), _track(mono, rate, [1.0, -3.0])], true_peak=True,
                                  dynamics=True)
    assert [_res_bytes(r) for r in more] == [_res_bytes(r) for r in plain]
    an.set_channel_mode_r128("layout")  # the layouts of one and two channels are weights of one
    layout = an.analyze_tracks_r128([_track(stereo, rate), _track(mono, rate)], true_peak=True, dynamics=True)
    assert [_res_bytes(r) for r in layout] == [_res_bytes(r) for r in plain]


# ---- (f) a mixed batch in hostile arenas -----------------------------------------------------------------------------------
def _raw(an, descs, n, arena, weights):
    """rg_r128_analyze_pcm_weighted without albums, everything asked for -> per track (record, dynamics, blocks, short-term)."""
    from mp3rgain_amd import _capi

    lib = _capi.load()
    zc = [int(lib.rg_r128_block_count(descs[i].sample_rate, descs[i].frames)) for i in range(n)]
    sc = [int(lib.rg_r128_short_term_count(descs[i].sample_rate, descs[i].frames)) for i in range(n)]
    z, st = np.zeros(max(1, sum(zc))), np.zeros(max(1, sum(sc)))
    out = (_capi.R128TrackResult * n)()
    dyn = (_capi.R128Dynamics * n)()
    an._check(lib.rg_r128_analyze_pcm_weighted(an.handle, descs, weights, n, None, 0, arena.ctypes.data, arena.nbytes, 0, 1, out, None,
                                               z.ctypes.data, dyn, None, st.ctypes.data))
    res, pz, ps = [], 0, 0
    for i in range(n):
        res.append((bytes(out[i]), bytes(dyn[i]), z[pz:pz + zc[i]].tobytes(), st[ps:ps + sc[i]].tobytes()))
        pz += zc[i]
        ps += sc[i]
    return res


def _weights_array(ws):
    from mp3rgain_amd import _capi

    arr = (_capi.R128ChannelWeights * max(1, len(ws)))()
    for i, w in enumerate(ws):
        for k, v in enumerate(w):
            arr[i].w[k] = v
    return arr


@pytest.mark.parametrize("layout", [arena_layouts.Layout("guard", "nan", "reversed"), arena_layouts.Layout("guard", "loud", "input", 3),
                                    arena_layouts.Layout("abut", "loud", "input")], ids=lambda l: f"{l.gap}-{l.guard}-{l.order}")
def test_mixed_batch_equals_solo_calls(an, layout):
    from mp3rgain_amd import replaygain

    rate = 8000
    tracks = [
        (_noise(rate, 31 * 800 + 13, 2, "f32", 701), [1.0, 1.0]),
        (_noise(rate, 33 * 800 + 1, 6, "s16", 702), W51),
        (_noise(rate, 30 * 800, 1, "s32", 703), [1.0]),
        (_noise(rate, 32 * 800 + 799, 6, "f32", 704), W51),
        (_noise(11025, 35 * 1103 + 2, 3, "f32", 705), [0.5, 2.0, 1.41]),
        (_noise(rate, 5 * 800, 6, "s16", 706), W51),
        (_noise(rate, 34 * 800 + 5, 2, "s16", 707), [1.0, 1.0]),
    ]
    rates = [rate, rate, rate, rate, 11025, rate, rate]
    an.set_tuning_r128(1, 3)  # the same hops per lane in the batch and alone
    solo = []
    for (ch, w), r in zip(tracks, rates):
        arena, descs = replaygain.pack_tracks([_track(ch, r)])
        solo.append(_raw(an, descs, 1, arena, _weights_array([w]))[0])
    order = list(np.random.default_rng(0xF00D).permutation(len(tracks)))  # descriptors shuffled
    pcm = [_track(tracks[i][0], rates[i]) for i in order]
    arena, descs, guards = arena_layouts.pack(pcm, layout)
    assert guards or layout.gap == "abut"
    got = _raw(an, descs, len(pcm), arena, _weights_array([tracks[i][1] for i in order]))
    for k, i in enumerate(order):
        assert got[k] == solo[i], (k, i)
    # the same batch by the context's mode: the 5.1 tracks get the layout's weights, one and two channels the plain path
    keep = [k for k, i in enumerate(order) if len(tracks[i][0]) != 3]
    pcm2 = [pcm[k] for k in keep]
    arena, descs, _ = arena_layouts.pack(pcm2, layout)
    an.set_channel_mode_r128("layout")
    by_mode = _raw(an, descs, len(pcm2), arena, None)
    assert by_mode == [solo[order[k]] for k in keep]
    an.set_channel_mode_r128("pair")
    pair = _raw(an, descs, len(pcm2), arena, None)
    plain = an.analyze_tracks_r128(pcm2, true_peak=True, dynamics=True)
    assert [struct.unpack("<d", p[0][:8])[0] for p in pair] == [r.loudness_lufs for r in plain]
    assert any(a[0] != b[0] for a, b in zip(pair, by_mode))


# ---- (g) albums --------------------------------------------------------------------------------------------------------------
def _album_set():
    rate = 8000
    a = [(_noise(rate, 36 * 800 + 9, 6, "s16", 801), rate, W51), (_noise(rate, 40 * 800, 2, "f32", 802, amp=(0.2, 0.15)), rate, None),
         (_noise(rate, 33 * 800 + 100, 6, "f32", 803, amp=(0.02, 0.02, 0.03, 0.5, 0.01, 0.015)), rate, W51)]
    b = [(_noise(rate, 35 * 800, 2, "s16", 804, amp=(0.05, 0.3)), rate, None), (_noise(rate, 45 * 800 + 3, 6, "f32", 805), rate, W51)]
    return [a, b]


def test_albums_equal_single_album_calls_and_the_checker(an):
    albums = _album_set()
    an.set_tuning_r128(1, 4)
    mk = lambda alb: [_track(ch, rate, w) for ch, rate, w in alb]  # noqa: E731
    many, zs, sts = an.analyze_albums_r128([mk(a) for a in albums], true_peak=True, dynamics=True, return_blocks=True, return_short_term=True)
    an.set_channel_mode_r128("layout")  # the single-album call proper: the same weights, by the context's mode
    plain = lambda alb: [_track(ch, rate) for ch, rate, _ in alb]  # noqa: E731
    singles = [an.analyze_album_r128(plain(alb), true_peak=True, dynamics=True, return_blocks=True, return_short_term=True) for alb in albums]
    an.set_channel_mode_r128("pair")
    for k, alb in enumerate(albums):
        one, z1, st1 = singles[k]
        again = an.analyze_album_r128(mk(alb), true_peak=True, dynamics=True)  # and by explicit weights
        assert _res_bytes(again) == _res_bytes(one) and [_res_bytes(t) for t in again.tracks] == [_res_bytes(t) for t in one.tracks], k
        assert _res_bytes(many[k]) == _res_bytes(one), k
        assert [_res_bytes(t) for t in many[k].tracks] == [_res_bytes(t) for t in one.tracks], k
        assert [z.tobytes() for z in zs[k]] == [z.tobytes() for z in z1] and [s.tobytes() for s in sts[k]] == [s.tobytes() for s in st1]
        _, ref = sref.analyze_album([(ch, rate, w if w is not None else [1.0] * len(ch)) for ch, rate, w in alb], True)
        z = np.concatenate(z1)
        _, _, thr = r128ref.gate(ref["z"])
        for gate in (r128ref.ABS_GATE, thr):  # the precondition, on the checker alone
            assert float(np.min(np.abs(ref["z"] - gate) / gate)) > 10.0 * TOL
        err = float(np.max(np.abs(z - ref["z"]) / ref["z"]))
        st = np.concatenate(st1)
        err_st = float(np.max(np.abs(st - ref["st"]) / ref["st"]))
        d = one.dynamics
        print(f"album {k}: {one.loudness_lufs:.6f} LUFS (ref {ref['loudness_lufs']:.6f}), LRA {d.loudness_range_lu:.6f} LU (ref "
              f"{ref['loudness_range_lu']:.6f}), worst block error {err:.2e} (bar {TOL:.2e}), short-term {err_st:.2e} (bar {ST_TOL:.2e})")
        assert err <= TOL and err_st <= ST_TOL
        assert abs(one.loudness_lufs - ref["loudness_lufs"]) <= LU * TOL + 1e-12
        assert (one.blocks, one.blocks_gated) == (ref["blocks"], ref["blocks_gated"])
        assert one.sample_peak == ref["sample_peak"] and abs(one.true_peak - ref["true_peak"]) <= TP_TOL * ref["true_peak"]
        assert (d.st_blocks, d.st_blocks_gated) == (ref["st_blocks"], ref["st_blocks_gated"])
        assert abs(d.loudness_range_lu - ref["loudness_range_lu"]) <= 2.0 * LU * ST_TOL
        for key in DYN_FIELDS[1:]:
            assert abs(getattr(d, key) - ref[key]) <= LU * ST_TOL, key
    # the LFE of album 0's last track is its loudest channel: it sets the peak and nothing else
    assert many[0].tracks[2].sample_peak == float(np.abs(albums[0][2][0][3]).max())


# ---- (h) files ---------------------------------------------------------------------------------------------------------------
def _wav_extensible(channels, rate, mask):
    """A 16-bit WAVE_FORMAT_EXTENSIBLE stream with the given dwChannelMask."""
    nch = len(channels)
    body = np.stack(channels, axis=1).astype("<i2").tobytes()
    guid = struct.pack("<H", 1) + bytes.fromhex("000000001000800000aa00389b71")
    fmt = struct.pack("<HHIIHHHHI", 0xFFFE, nch, rate, rate * nch * 2, nch * 2, 16, 22, 16, mask) + guid
    assert len(fmt) == 40
    chunks = b"fmt " + struct.pack("<I", len(fmt)) + fmt + b"data" + struct.pack("<I", len(body)) + body
    return b"RIFF" + struct.pack("<I", 4 + len(chunks)) + b"WAVE" + chunks


@pytest.fixture(scope="module")
def surround_files(tmp_path_factory):
    """[(path, decoded channels, rate, channel mask)]"""
    from mp3rgain_amd import flacdec

    d = tmp_path_factory.mktemp("r128surround")
    rate = 8000
    chans = _noise(rate, 32 * 800 + 17, 6, "s16", 901, amp=(0.05, 0.06, 0.04, 0.4, 0.12, 0.1))
    files = []
    for mask in (0x3F, 0x60F, 0x633):  # 5.1 with backs, 5.1 with sides, six channels without an LFE
        p = d / f"six_{mask:x}.wav"
        p.write_bytes(_wav_extensible(chans, rate, mask))
        files.append((p, chans, rate, mask))
    frate, bps, fp, _ = flacdec.decode(FLAC6.read_bytes())
    assert bps == 16 and len(fp) == 6
    files.append((FLAC6, [c.astype(np.int16) for c in fp], frate, 0))
    return files


def test_files_use_the_containers_mask(an, surround_files):
    import mp3rgain_amd as rg

    assert rg.r128_layout_weights(6, 0x633) == [1.0, 1.0, 1.0, 1.0, 1.41, 1.41]
    an.set_tuning_r128(1, 4)
    paths = [f[0] for f in surround_files]
    pair_pcm = an.analyze_tracks_r128([_track(ch, rate) for _, ch, rate, _ in surround_files], true_peak=True, dynamics=True)
    want = an.analyze_tracks_r128([_track(ch, rate, rg.r128_layout_weights(len(ch), mask)) for _, ch, rate, mask in surround_files],
                                  true_peak=True, dynamics=True)
    pair = an.analyze_track_files_r128(paths, true_peak=True, dynamics=True)
    assert [_res_bytes(r) for r in pair] == [_res_bytes(r) for r in pair_pcm]
    an.set_channel_mode_r128("layout")
    got = an.analyze_track_files_r128(paths, true_peak=True, dynamics=True)
    for f, g, w, p in zip(surround_files, got, want, pair):
        print(f"{f[0].name}: {g.loudness_lufs:.4f} LUFS by layout, {p.loudness_lufs:.4f} as a pair")
    assert [_res_bytes(r) for r in got] == [_res_bytes(r) for r in want]
    assert got[2].loudness_lufs > got[0].loudness_lufs + 3.0  # mask 0x633 counts the channel that 0x3F calls the LFE
    assert all(_res_bytes(a) != _res_bytes(b) for a, b in zip(got, pair))
    # the album routes: one album of files, and the same album among many
    album = an.analyze_album_files_r128(paths[:3], true_peak=True, dynamics=True)
    album_pcm = an.analyze_album_r128([_track(ch, rate, rg.r128_layout_weights(len(ch), mask)) for _, ch, rate, mask in surround_files[:3]],
                                      true_peak=True, dynamics=True)
    assert _res_bytes(album) == _res_bytes(album_pcm)
    many = an.analyze_albums_files_r128([paths[:3], [paths[3]]], true_peak=True, dynamics=True)
    assert _res_bytes(many[0]) == _res_bytes(album) and _res_bytes(many[1].tracks[0]) == _res_bytes(want[3])
    an.set_channel_mode_r128("pair")
    again = an.analyze_track_files_r128(paths, true_peak=True, dynamics=True)
    assert [_res_bytes(r) for r in again] == [_res_bytes(r) for r in pair]


def test_files_through_a_one_gpu_node(an, surround_files):
    import mp3rgain_amd as rg

    paths = [f[0] for f in surround_files]
    an.set_tuning_r128(1, 4)
    pair = an.analyze_track_files_r128(paths, true_peak=True, dynamics=True)
    an.set_channel_mode_r128("layout")
    layout = an.analyze_track_files_r128(paths, true_peak=True, dynamics=True)
    album = an.analyze_album_files_r128(paths, true_peak=True, dynamics=True)
    with rg.Node([0]) as node:
        node.analyzer(0).set_tuning_r128(1, 4)
        got = node.analyze_track_files_r128(paths, true_peak=True, dynamics=True)
        assert [_res_bytes(r) for r in got] == [_res_bytes(r) for r in pair]
        node.set_channel_mode_r128("layout")
        got = node.analyze_track_files_r128(paths, true_peak=True, dynamics=True)
        assert [_res_bytes(r) for r in got] == [_res_bytes(r) for r in layout]
        albums = node.analyze_albums_files_r128([paths], true_peak=True, dynamics=True)
        assert _res_bytes(albums[0]) == _res_bytes(album)
        node.set_channel_mode_r128("pair")
        got = node.analyze_track_files_r128(paths, true_peak=True, dynamics=True)
        assert [_res_bytes(r) for r in got] == [_res_bytes(r) for r in pair]


# ---- (i) edge rules ------------------------------------------------------------------------------------------------------------
def test_edge_rules(an):
    import mp3rgain_amd as rg
    from mp3rgain_amd import _capi, replaygain

    lib = _capi.load()
    rate = 8000
    six = _noise(rate, 20 * 800, 6, "f32", 1001)

    def refused(tracks, weights):
        arena, descs = replaygain.pack_tracks(tracks)
        n = len(tracks)
        out = (_capi.R128TrackResult * n)()
        C.memset(out, 0xA5, C.sizeof(out))
        z = np.full(64, -7.0)
        rc = lib.rg_r128_analyze_pcm_weighted(an.handle, descs, weights, n, None, 0, arena.ctypes.data, arena.nbytes, 0, 0, out, None,
                                              z.ctypes.data, None, None, None)
        assert rc == _capi.RG_ERR_INVALID_ARG, rc
        assert bytes(out) == b"\xa5" * C.sizeof(out) and np.all(z == -7.0)  # outputs untouched
        return lib.rg_last_error(an.handle).decode()

    nine = [_track(six[:2], rate), _track([six[0]] * 9, rate)]
    assert "track 1" in refused(nine, _weights_array([[1.0, 1.0], [1.0] * 8]))
    assert "track 0" in refused([_track(six, rate)], _weights_array([[1.0, 1.0, -0.5, 0.0, 1.0, 1.0]]))
    assert "track 1" in refused([_track(six, rate), _track(six, rate)], _weights_array([W51, [1.0, math.nan, 1.0, 0.0, 1.0, 1.0]]))
    refused([_track(six, rate)], _weights_array([[1.0, math.inf, 1.0, 0.0, 1.0, 1.0]]))
    an.set_channel_mode_r128("layout")  # the layout rule has no nine channels either
    assert "track 1" in refused(nine, None)
    with pytest.raises(rg.ReplayGainError):
        an.analyze_tracks_r128(nine)
    an.set_channel_mode_r128("pair")
    assert len(an.analyze_tracks_r128(nine)) == 2  # as a pair it is what it always was
    with pytest.raises(rg.ReplayGainError):
        an.set_channel_mode_r128(2)
    with pytest.raises(rg.ReplayGainError):
        an.set_channel_mode_r128(-1)

    # all weights zero: every hop energy is 0
    r, z = an.analyze_tracks_r128([_track(six, rate, [0.0] * 6)], true_peak=True, dynamics=True, return_blocks=True)
    assert r[0].loudness_lufs == -math.inf and r[0].gain_db == 0.0 and (r[0].blocks, r[0].blocks_gated) == (17, 0)
    assert not z[0].any() and len(z[0]) == 17 and r[0].flags == 0
    assert r[0].sample_peak == max(float(np.abs(c).max()) for c in six)
    assert r[0].dynamics.max_momentary_lufs == -math.inf and r[0].dynamics.loudness_range_lu == 0.0
    # no frames, and fewer than four hops
    empty = [np.zeros(0, dtype=np.float32)] * 6
    short = [c[:3 * 800 + 799] for c in six]
    r = an.analyze_tracks_r128([_track(empty, rate, W51), _track(short, rate, W51), _track(six, rate, W51)], true_peak=True, dynamics=True)
    assert (r[0].blocks, r[0].sample_peak, r[0].true_peak, r[0].loudness_lufs, r[0].gain_db) == (0, 0.0, 0.0, -math.inf, 0.0)
    assert (r[1].blocks, r[1].loudness_lufs, r[1].gain_db) == (0, -math.inf, 0.0)
    assert r[1].sample_peak == max(float(np.abs(c).max()) for c in short)
    assert r[1].dynamics.st_blocks == 0 and r[1].dynamics.max_momentary_lufs == -math.inf
    alone = an.analyze_tracks_r128([_track(six, rate, W51)], true_peak=True, dynamics=True)
    assert _res_bytes(r[2]) == _res_bytes(alone[0])
    want = sref.analyze(six, rate, W51)
    assert abs(r[2].loudness_lufs - want["loudness_lufs"]) <= LU * TOL + 1e-12
    # weights = NULL in PAIR mode: the bits of the plain calls
    arena, descs = replaygain.pack_tracks([_track(six, rate), _track(short, rate)])
    plain = an.analyze_tracks_r128([_track(six, rate), _track(short, rate)], true_peak=True, dynamics=True)
    raw = _raw(an, descs, 2, arena, None)
    assert [struct.unpack("<4d", x[0][:32]) for x in raw] == [(p.loudness_lufs, p.gain_db, p.sample_peak, p.true_peak) for p in plain]


# ---- (j) the command line ------------------------------------------------------------------------------------------------------
def test_cli_surround(an, surround_files):
    path, chans, rate, mask = surround_files[0]
    stereo = path.parent / "stereo.wav"
    stereo.write_bytes(_wav_extensible(chans[:2], rate, 0x3))
    an.set_tuning_r128(1, 0)
    files = [path, FLAC6, stereo]
    pair = an.analyze_track_files_r128(files)
    an.set_channel_mode_r128("layout")
    layout = an.analyze_track_files_r128(files)
    album = an.analyze_album_files_r128(files)
    an.set_channel_mode_r128("pair")
    env = dict(os.environ, PYTHONPATH=str(ROOT), MP3RGAIN_AMD_DEVICES="0")

    def cli(*args):
        p = subprocess.run([sys.executable, "-m", "mp3rgain_amd", *[str(a) for a in args]], capture_output=True, text=True, env=env,
                           cwd=ROOT, timeout=600)
        return p.returncode, p.stdout, p.stderr

    rc, out, err = cli("--r128", "--surround", "-a", "-n", "-o", "json", *files)
    assert rc == 0, err
    d = json.loads(out)
    lufs = lambda v: -math.inf if v is None else v  # noqa: E731  (the golden FLAC has no whole block: JSON has no -inf)
    assert [lufs(f["loudness_lufs"]) for f in d["files"]] == [r.loudness_lufs for r in layout]
    assert d["album"]["loudness_lufs"] == album.loudness_lufs
    rc, out, err = cli("--r128", "-r", "-n", "-o", "json", *files)
    assert rc == 0, err
    got = [lufs(f["loudness_lufs"]) for f in json.loads(out)["files"]]
    assert got == [r.loudness_lufs for r in pair]
    assert got[2] == layout[2].loudness_lufs and got[0] != layout[0].loudness_lufs
    assert layout[1].sample_peak > pair[1].sample_peak  # the FLAC's loudest channels are not its first two
    rc, out, err = cli("--surround", "-r", "-n", path)
    assert rc == 1 and "--surround requires --r128" in err
