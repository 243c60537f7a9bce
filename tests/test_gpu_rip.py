"""The rip checksums on the GPU (include/mp3rgain_amd_rip.h): the two kernels through their seam (rg_rip_checksums_arena, route 1)
on the shared cases in the arena layouts every PCM-reading kernel is held to, and rg_rip_checksums on files.  The oracle is the
Python restatement of the definitions (tests/rip_cases.py: zlib.crc32, numpy, a plain loop); no tolerance anywhere.
tests/test_rip_cpu.py proves the same cases on the host routes."""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import arena_layouts as al  # noqa: E402
import flacenc  # noqa: E402
import rip_cases as rc  # noqa: E402
from wavutil import wav_bytes  # noqa: E402

from mp3rgain_amd import _capi, flacdec  # noqa: E402

pytestmark = pytest.mark.gpu

GOLD = Path(__file__).resolve().parent / "golden"
RG_ERR_IO, RG_ERR_FORMAT = -8, -9


@pytest.fixture()
def an(_ctx):
    _ctx.set_tuning(14, 1)
    _ctx.set_tuning(13, 0)
    _ctx.set_decoder_command(None)
    yield _ctx
    _ctx.set_tuning(14, 1)
    _ctx.set_tuning(13, 0)


def _raw(recs):
    return b"".join(bytes(r) for r in recs)


# ---- the kernels, through the seam --------------------------------------------------------------------------------------------
LAYOUTS = [al.Layout("abut", "loud", "input"), al.Layout("guard", "loud", "input"), al.Layout("guard", "loud", "reversed"),
           al.Layout("abut", "loud", "reversed")] + [al.Layout("guard", "loud", "input", s) for s in range(1, 7)]


@pytest.mark.parametrize("layout", LAYOUTS, ids=lambda l: f"{l.gap}-{l.order}-{l.shift}")
def test_kernels_match_the_restatement_in_every_layout(an, layout):
    """Every case in one launch, the flags cycling through the four combinations with the layout; what lies around the
    tracks (other tracks, INT_MIN / INT_MAX guards) reaches no result, rewriting the guards changes no byte, the same call
    twice gives the same bytes, and the kernels' arithmetic on the host (route 2) gives them too."""
    cases, wants = rc.cases(), rc.wants()
    arena, descs, guards = al.pack(rc.tracks(cases), layout)
    descs = list(descs)[:len(cases)]
    flags = [rc.ALL_FLAGS[(k + layout.shift + (layout.order == "reversed")) % 4] for k in range(len(cases))]
    out = an.rip_checksums_arena(1, descs, flags, arena)
    bad = [(cs.name, fl, rc.got(r), wants[(cs.name, fl)]) for cs, fl, r in zip(cases, flags, out) if rc.got(r) != wants[(cs.name, fl)]]
    assert not bad, f"{len(bad)} of {len(cases)} records differ from the restatement: {bad[:4]}"
    for cs, r in zip(cases, out):
        assert (r.status, r.frames, r.sample_rate, r.dropped_frames) == (0, len(cs.left), 44100, 0)
    raw = _raw(out)
    assert _raw(an.rip_checksums_arena(1, descs, flags, arena)) == raw
    assert _raw(an.rip_checksums_arena(2, descs, flags, arena)) == raw
    if guards:
        other = arena.copy()
        for a, b in guards:
            other[a:b] ^= 0x5A
        assert _raw(an.rip_checksums_arena(1, descs, flags, other)) == raw


def test_kernels_on_aliased_tracks_every_case_with_every_flag(an):
    """Four descriptors per case share one copy of its PCM and differ in their flags: all 4 x cases records in one launch."""
    cases, wants = rc.cases(), rc.wants()
    tracks = rc.tracks(cases)
    arena, descs, _ = al.pack(tracks * 4, al.Layout("guard", "loud", "aliased"))
    n = len(cases)
    descs = list(descs)[:4 * n]
    assert all(descs[k].offset_bytes == descs[k % n].offset_bytes for k in range(4 * n))
    flags = [rc.ALL_FLAGS[k // n] for k in range(4 * n)]
    out = an.rip_checksums_arena(1, descs, flags, arena)
    bad = [(cases[k % n].name, flags[k]) for k in range(4 * n) if rc.got(out[k]) != wants[(cases[k % n].name, flags[k])]]
    assert not bad, f"{len(bad)} of {4 * n} records differ from the restatement: {bad[:6]}"
    assert _raw(an.rip_checksums_arena(0, descs, flags, arena)) == _raw(out)


def test_kernels_refuse_a_track_outside_the_arena(an):
    import mp3rgain_amd as rg

    arena = np.zeros(64, dtype=np.uint8)
    for desc in (_capi.TrackDesc(0, 17, 44100, 2, _capi.FMT_S16_PLANAR), _capi.TrackDesc(2, 16, 44100, 2, _capi.FMT_S16_PLANAR)):
        with pytest.raises(rg.ReplayGainError) as e:
            an.rip_checksums_arena(1, [desc], [0], arena)
        assert e.value.code == -1 and "beyond the arena" in str(e.value)
    with pytest.raises(rg.ReplayGainError) as e:
        an.rip_checksums_arena(1, [_capi.TrackDesc(0, 16, 44100, 1, _capi.FMT_S16_PLANAR)], [0], arena)
    assert e.value.code == RG_ERR_FORMAT
    r = an.rip_checksums_arena(1, [_capi.TrackDesc(0, 16, 44100, 2, _capi.FMT_S16_PLANAR)], [3], arena)[0]
    assert rc.got(r) == rc.want(np.zeros(16, np.int16), np.zeros(16, np.int16), 3)
    assert an.rip_checksums_arena(1, [], [], arena) == []


# ---- rg_rip_checksums on files ------------------------------------------------------------------------------------------------
def _write(tmp_path, name, data):
    p = tmp_path / name
    p.write_bytes(data)
    return p


@pytest.fixture(scope="module")
def disc(tmp_path_factory):
    """Three tracks, each as WAV and as FLAC: [(pcm int16 [2][n], wav path, flac path)]."""
    tmp = tmp_path_factory.mktemp("disc")
    rng = np.random.default_rng(31)
    c, t, f = rc.shape()
    out = []
    for k, n in enumerate((t + 2941, 3 * 1152 + 77, 2 * t + 588 * 3)):
        pcm = flacenc.test_pcm(rng, 2, n, 16)
        pcm[0, 100:140] = 0  # some null samples, in one channel and in both
        pcm[:, 500:510] = 0
        wav = _write(tmp, f"{k + 1:02d}.wav", wav_bytes([pcm[0], pcm[1]], 44100, "s16"))
        flac = _write(tmp, f"{k + 1:02d}.flac", flacenc.encode(pcm, 44100, 16, flacenc.Options(block_size=1152, stereo="mid_side")))
        out.append((pcm.astype(np.int16), wav, flac))
    return out


def test_wav_and_flac_of_the_same_pcm_give_the_same_records_on_both_decoder_routes(an, disc):
    wavs, flacs = [d[1] for d in disc], [d[2] for d in disc]
    raw_wav = an.rip_checksums_raw(wavs)
    raw_flac = an.rip_checksums_raw(flacs)
    assert len(raw_wav) == 48 * 3 and raw_wav == raw_flac
    an.set_tuning(14, 0)
    assert an.rip_checksums_raw(flacs) == raw_flac and an.rip_checksums_raw([wavs[0], flacs[1], wavs[2]]) == raw_flac
    an.set_tuning(13, 24 * 30000)  # a file or two per group: the flags travel with their files
    assert an.rip_checksums_raw(flacs) == raw_flac
    an.set_tuning(14, 1)
    assert an.rip_checksums_raw([flacs[0], wavs[1], flacs[2]]) == raw_flac


def test_a_disc_of_three_files(an, disc):
    res = an.rip_checksums([d[2] for d in disc], disc=True)
    flags = [rc.FIRST, 0, rc.LAST]
    for (pcm, _, _), fl, r in zip(disc, flags, res):
        w = rc.want(pcm[0], pcm[1], fl)
        assert r.error is None and (r.crc32, r.crc32_nonnull, r.null_samples, r.arv1, r.arv2) == tuple(w)
        assert w.null_samples >= 60 and w.crc32 != w.crc32_nonnull and (w.arv1 != rc.want(pcm[0], pcm[1], 0).arv1) == bool(fl)
        assert (r.frames, r.sample_rate, r.dropped_frames, r.cd_rate, r.complete) == (pcm.shape[1], 44100, 0, True, True)
        assert r.cd_frames == (pcm.shape[1] % 588 == 0) and (r.first_track, r.last_track) == (bool(fl & 1), bool(fl & 2))
    # not a disc: no flag anywhere; and a disc of one track is first and last
    plain = an.rip_checksums([d[1] for d in disc], disc=False)
    assert [(r.arv1, r.arv2) for r in plain] == [rc.want(p[0], p[1], 0)[3:] for p, _, _ in disc]
    one = an.rip_checksums([disc[0][1]])[0]
    assert (one.arv1, one.arv2) == rc.want(disc[0][0][0], disc[0][0][1], 3)[3:] and one.first_track and one.last_track
    assert an.rip_checksums([]) == []


def test_failing_files_fail_alone(an, tmp_path, disc):
    rng = np.random.default_rng(32)
    good_wav, good_flac = disc[1][1], disc[1][2]
    mono = _write(tmp_path, "mono.wav", wav_bytes([flacenc.test_pcm(rng, 1, 4000, 16)[0]], 44100, "s16"))
    wide = _write(tmp_path, "wide.wav", wav_bytes(list(flacenc.test_pcm(rng, 2, 4000, 24)), 44100, "s24"))
    wide_flac = _write(tmp_path, "wide.flac", flacenc.encode(flacenc.test_pcm(rng, 2, 3000, 24), 48000, 24, flacenc.Options(block_size=576)))
    mono_flac = _write(tmp_path, "mono.flac", flacenc.encode(flacenc.test_pcm(rng, 1, 3000, 16), 44100, 16, flacenc.Options(block_size=576)))
    floaty = _write(tmp_path, "float.wav", wav_bytes([np.zeros(100, np.float32)] * 2, 44100, "f32"))
    mp3 = GOLD / "mp3" / "v1_44k_ms_mixed.mp3"
    missing = tmp_path / "missing.flac"
    files = [good_flac, mono, good_wav, wide, mp3, good_flac, missing, wide_flac, mono_flac, floaty, good_wav]
    an.set_decoder_command("false {}")  # a decoder command is set and must not be run
    try:
        res = an.rip_checksums(files, disc=False)
        raw = an.rip_checksums_raw(files, disc=False)
    finally:
        an.set_decoder_command(None)
    w = rc.want(disc[1][0][0], disc[1][0][1], 0)
    for k in (0, 2, 5, 10):
        r = res[k]
        assert r.error is None and (r.crc32, r.crc32_nonnull, r.null_samples, r.arv1, r.arv2) == tuple(w), k
    for k, code, text in ((1, RG_ERR_FORMAT, "1 channel"), (3, RG_ERR_FORMAT, "24-bit"), (4, RG_ERR_FORMAT, "MPEG"), (6, RG_ERR_IO, "Failed to open"),
                          (7, RG_ERR_FORMAT, "24 bits"), (8, RG_ERR_FORMAT, "1 channel"), (9, RG_ERR_FORMAT, "float")):
        r = res[k]
        assert r.error is not None and r.error.code == code and text in str(r.error) and str(files[k]) in str(r.error), (k, str(r.error))
        assert (r.crc32, r.crc32_nonnull, r.arv1, r.arv2, r.frames, r.null_samples, r.sample_rate, r.dropped_frames) == (0,) * 8
        assert not (r.cd_rate or r.cd_frames or r.complete)
        rec = _capi.RipRecord.from_buffer_copy(raw[48 * k:48 * k + 48])
        assert rec.status == code and raw[48 * k + 4:48 * k + 48] == bytes(44)  # zero apart from `status`


def test_a_damaged_flac_stream_gets_the_checksums_of_what_was_decoded(an, tmp_path):
    name, data, kept, dropped = next(v for v in flacenc.damaged_variants() if v[0] == "bitflip")
    _, _, host, hi = flacdec.decode(data)
    assert dropped == 1 and int(hi.dropped_frames) == 1 and np.array_equal(host, kept)
    p = _write(tmp_path, "damaged.flac", data)
    for key14 in (1, 0):
        an.set_tuning(14, key14)
        r = an.rip_checksums([p])[0]
        assert r.error is None and r.dropped_frames == 1 and not r.complete and r.frames == host.shape[1]
        assert (r.crc32, r.crc32_nonnull, r.null_samples, r.arv1, r.arv2) == tuple(rc.want(host[0], host[1], 3))
