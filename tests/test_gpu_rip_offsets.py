"""The AccurateRip signatures at every drive offset on the GPU (include/mp3rgain_amd_rip.h, DRIVE OFFSETS): the kernel through its
seam (rg_rip_offsets_arena, route 1) on the shared discs in the arena layouts every PCM-reading kernel is held to, and
rg_rip_offset_signatures on files.  The oracle is the numpy restatement of the definition (tests/rip_offset_cases.py); no
tolerance anywhere.  tests/test_rip_offsets_cpu.py proves the same discs on the host routes."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import arena_layouts as al  # noqa: E402
import flacenc  # noqa: E402
import rip_cases as rc  # noqa: E402
import rip_offset_cases as oc  # noqa: E402
from wavutil import wav_bytes  # noqa: E402

pytestmark = pytest.mark.gpu

RG_ERR_REFUSED = -10
FULL = oc.RADIUS_MAX


@pytest.fixture()
def an(_ctx):
    _ctx.set_tuning(14, 1)
    _ctx.set_tuning(13, 0)
    _ctx.set_decoder_command(None)
    yield _ctx
    _ctx.set_tuning(14, 1)
    _ctx.set_tuning(13, 0)


def _check_discs(an, layout, radius):
    want = oc.restated(radius)
    for d in oc.discs():
        arena, descs, guards = al.pack(oc.tracks(d), layout)
        descs = list(descs)[:len(d.tracks)]
        v1, v2 = an.rip_offsets_arena(1, descs, d.flags, radius, arena)
        w1, w2 = want[d.name]
        assert v1.shape == w1.shape and v2.shape == w2.shape
        assert np.array_equal(v1, w1), (d.name, "arv1", np.argwhere(v1 != w1)[:4].tolist())
        assert np.array_equal(v2, w2), (d.name, "arv2", np.argwhere(v2 != w2)[:4].tolist())
        raw = v1.tobytes() + v2.tobytes()
        again = an.rip_offsets_arena(1, descs, d.flags, radius, arena)
        assert again[0].tobytes() + again[1].tobytes() == raw, d.name
        host = an.rip_offsets_arena(0, descs, d.flags, radius, arena)
        assert host[0].tobytes() + host[1].tobytes() == raw, d.name
        # one table at a time gives the same table
        assert an.rip_offsets_arena(1, descs, d.flags, radius, arena, (True, False))[0].tobytes() == v1.tobytes()
        assert an.rip_offsets_arena(1, descs, d.flags, radius, arena, (False, True))[1].tobytes() == v2.tobytes()
        if guards:
            other = arena.copy()
            for a, b in guards:
                other[a:b] ^= 0x5A
            o1, o2 = an.rip_offsets_arena(1, descs, d.flags, radius, other)
            assert o1.tobytes() + o2.tobytes() == raw, d.name


LAYOUTS = [al.Layout("abut", "loud", "input"), al.Layout("guard", "loud", "input"), al.Layout("guard", "loud", "reversed"),
           al.Layout("abut", "loud", "reversed")] + [al.Layout("guard", "loud", "input", s) for s in range(1, 7)]


@pytest.mark.parametrize("layout", LAYOUTS, ids=lambda l: f"{l.gap}-{l.order}-{l.shift}")
def test_kernel_matches_the_restatement_in_every_layout_at_radius_40(an, layout):
    """Every disc; what lies around the tracks (other tracks, INT_MIN / INT_MAX guards) reaches no result, rewriting the guards
    changes no byte, the same call twice gives the same bytes, and the definition on the host (route 0) gives them too."""
    _check_discs(an, layout, 40)


@pytest.mark.parametrize("layout", LAYOUTS[:3], ids=lambda l: f"{l.gap}-{l.order}")
def test_kernel_matches_the_restatement_at_the_full_radius(an, layout):
    _check_discs(an, layout, FULL)


@pytest.mark.parametrize("radius", [0, 1])
def test_kernel_at_the_smallest_radii(an, radius):
    _check_discs(an, al.Layout("guard", "loud", "input", 3), radius)


def test_kernel_on_aliased_tracks(an):
    """A disc whose tracks 0, 2 and 4 are one copy of the same PCM, and 1 and 3 another: the disc's words repeat, the arena's
    do not."""
    rng = np.random.default_rng(77)
    t, _ = oc.shape()
    a, b = rc.Track(list(rc._planes("random", t + 5, rng)), 44100), rc.Track(list(rc._planes("sparse", 3, rng)), 44100)
    trs = [a, b, a, b, a]
    arena, descs, _ = al.pack(trs, al.Layout("guard", "loud", "aliased"))
    descs = list(descs)[:5]
    assert descs[0].offset_bytes == descs[2].offset_bytes == descs[4].offset_bytes and descs[1].offset_bytes == descs[3].offset_bytes
    disc = oc.Disc("aliased", [(x.channels[0], x.channels[1]) for x in trs], [rc.FIRST, 0, 0, 0, rc.LAST])
    for radius in (40, FULL):
        w1, w2 = oc.restate(disc, radius)
        v1, v2 = an.rip_offsets_arena(1, descs, disc.flags, radius, arena)
        assert np.array_equal(v1, w1) and np.array_equal(v2, w2)


def test_kernel_seam_argument_errors(an):
    import mp3rgain_amd as rg
    from mp3rgain_amd import _capi

    arena = np.zeros(64, dtype=np.uint8)
    good = _capi.TrackDesc(0, 16, 44100, 2, _capi.FMT_S16_PLANAR)
    for descs, radius in (([_capi.TrackDesc(0, 17, 44100, 2, _capi.FMT_S16_PLANAR)], 1), ([good], -1), ([good], FULL + 1)):
        with pytest.raises(rg.ReplayGainError) as e:
            an.rip_offsets_arena(1, descs, [0], radius, arena)
        assert e.value.code == -1
    v1, v2 = an.rip_offsets_arena(1, [], [], 5, arena)
    assert v1.shape == (0, 11) and v2.shape == (0, 11)


# ---- rg_rip_offset_signatures on files ----------------------------------------------------------------------------------------
def _write(tmp_path, name, data):
    p = tmp_path / name
    p.write_bytes(data)
    return p


@pytest.fixture(scope="module")
def disc(tmp_path_factory):
    """Three tracks, each as WAV and as FLAC: [(pcm int16 [2][n], wav path, flac path)]."""
    tmp = tmp_path_factory.mktemp("offdisc")
    rng = np.random.default_rng(31)
    t, _ = oc.shape()
    out = []
    for k, n in enumerate((t + 2941, 3 * 1152 + 77, 2 * t + 588 * 3)):
        pcm = flacenc.test_pcm(rng, 2, n, 16)
        pcm[0, 100:140] = 0
        pcm[:, 500:510] = 0
        wav = _write(tmp, f"{k + 1:02d}.wav", wav_bytes([pcm[0], pcm[1]], 44100, "s16"))
        flac = _write(tmp, f"{k + 1:02d}.flac", flacenc.encode(pcm, 44100, 16, flacenc.Options(block_size=1152, stereo="mid_side")))
        out.append((pcm.astype(np.int16), wav, flac))
    return out


def test_files_wav_and_flac_on_both_decoder_routes_give_the_restatement(an, disc):
    wavs, flacs = [d[1] for d in disc], [d[2] for d in disc]
    want = oc.restate(oc.Disc("files", [(d[0][0], d[0][1]) for d in disc], [rc.FIRST, 0, rc.LAST]), FULL)
    rc_w, out_w, v1, v2 = an.rip_offset_signatures_raw(wavs)
    assert rc_w == 0 and np.array_equal(v1, want[0]) and np.array_equal(v2, want[1])
    assert out_w == an.rip_checksums_raw(wavs) and len(out_w) == 48 * 3
    tables = v1.tobytes() + v2.tobytes()
    for key14 in (1, 0):
        an.set_tuning(14, key14)
        for files in (flacs, [wavs[0], flacs[1], wavs[2]]):
            rc_f, out_f, f1, f2 = an.rip_offset_signatures_raw(files)
            assert rc_f == 0 and out_f == out_w and f1.tobytes() + f2.tobytes() == tables, (key14, files)
    an.set_tuning(14, 1)
    res = an.rip_offset_signatures(flacs, radius=40)
    assert res.radius == 40 and res.arv1.shape == (3, 81) and res.arv1.dtype == np.uint32
    assert np.array_equal(res.arv1, want[0][:, FULL - 40:FULL + 41]) and np.array_equal(res.arv2, want[1][:, FULL - 40:FULL + 41])
    assert [(r.arv1, r.arv2) for r in res.tracks] == [res.at(t, 0) for t in range(3)]
    assert [(r.first_track, r.last_track, r.error) for r in res.tracks] == [(True, False, None), (False, False, None), (False, True, None)]
    empty = an.rip_offset_signatures([], radius=3)
    assert empty.tracks == [] and empty.arv1.shape == (0, 7)


@pytest.mark.parametrize("shift", [6, -7])
def test_a_rip_read_at_another_offset_is_found_at_that_offset(an, tmp_path, shift):
    """Disc PCM D cut into rip A at the track boundaries, and rip B cut at the same boundaries from D read `shift` frames later:
    A's signatures at offset `shift` are B's checksums."""
    rng = np.random.default_rng(5)
    t, _ = oc.shape()
    bounds = np.cumsum([0, t + 3000, 2 * 588 + 5, 2 * t + 100])
    pad = 16
    whole = flacenc.test_pcm(rng, 2, int(bounds[-1]) + 2 * pad, 16).astype(np.int16)  # D with `pad` frames of lead-in and lead-out
    rips = {}
    for name, s in (("a", 0), ("b", shift)):
        files = []
        for k in range(3):
            cut = whole[:, pad + s + bounds[k]:pad + s + bounds[k + 1]]
            files.append(_write(tmp_path, f"{name}{k}.wav", wav_bytes([cut[0], cut[1]], 44100, "s16")))
        rips[name] = files
    a = an.rip_offset_signatures(rips["a"], disc=True, radius=40)
    b = an.rip_checksums(rips["b"], disc=True)
    for k in range(3):
        # the outer tracks' flagged ends stay inside rip A; the middle of the disc reads A's neighbours
        assert a.at(k, shift) == (b[k].arv1, b[k].arv2), k
        assert a.at(k, 0) != (b[k].arv1, b[k].arv2)
    assert [r.crc32 for r in a.tracks] == [r.crc32 for r in an.rip_checksums(rips["a"], disc=True)]


def test_a_file_that_takes_no_part_refuses_the_tables(an, tmp_path, disc):
    import mp3rgain_amd as rg

    rng = np.random.default_rng(32)
    mono = _write(tmp_path, "mono.wav", wav_bytes([flacenc.test_pcm(rng, 1, 4000, 16)[0]], 44100, "s16"))
    files = [disc[0][1], mono, disc[2][2]]
    code, out, v1, v2 = an.rip_offset_signatures_raw(files, radius=40)
    assert code == RG_ERR_REFUSED
    assert out == an.rip_checksums_raw(files) and out[48:52] != bytes(4) and out[0:4] == bytes(4)
    assert not v1.any() and not v2.any()
    with pytest.raises(rg.ReplayGainError) as e:
        an.rip_offset_signatures(files, radius=40)
    assert e.value.code == RG_ERR_REFUSED and str(mono) in str(e.value)


def test_a_disc_cut_into_groups_is_refused(an, disc):
    import mp3rgain_amd as rg

    flacs = [d[2] for d in disc]
    an.set_tuning(13, 24 * 30000)  # a file or two per group
    with pytest.raises(rg.ReplayGainError) as e:
        an.rip_offset_signatures(flacs, radius=40)
    assert e.value.code == RG_ERR_REFUSED and "groups" in str(e.value)
    code, out, v1, v2 = an.rip_offset_signatures_raw(flacs, radius=40)
    assert code == RG_ERR_REFUSED and not v1.any() and not v2.any()
    an.set_tuning(13, 0)
    assert an.rip_offset_signatures(flacs, radius=40).arv1.any()
