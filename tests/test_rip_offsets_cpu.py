"""The host side of the AccurateRip signatures at every drive offset (include/mp3rgain_amd_rip.h, DRIVE OFFSETS), without a
GPU: the definition (rg_rip_offsets_arena route 0) and arv1's sliding recurrence (route 2) against the numpy restatement of
tests/rip_offset_cases.py, the closed form of an impulse, the argument errors, riplog.find_offset on constructed tables and
the command line's option errors."""
import io
import sys
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import arena_layouts as al  # noqa: E402
import rip_cases as rc  # noqa: E402
import rip_offset_cases as oc  # noqa: E402

from mp3rgain_amd import _capi, replaygain, riplog  # noqa: E402

LAYOUT = al.Layout("guard", "loud", "reversed", 2)


def _packed(disc):
    arena, descs, _ = al.pack(oc.tracks(disc), LAYOUT)
    return arena, list(descs)[:len(disc.tracks)]


@pytest.mark.parametrize("radius", [oc.RADIUS_MAX, 0, 1, 40])
def test_the_definition_on_the_host_equals_the_restatement(radius):
    want = oc.restated(radius)
    for d in oc.discs():
        arena, descs = _packed(d)
        v1, v2 = replaygain.rip_offsets_arena(None, 0, descs, d.flags, radius, arena)
        assert v1.shape == (len(d.tracks), 2 * radius + 1) and v1.dtype == np.uint32
        assert np.array_equal(v1, want[d.name][0]) and np.array_equal(v2, want[d.name][1]), d.name
        only2 = replaygain.rip_offsets_arena(None, 0, descs, d.flags, radius, arena, (False, True))
        assert only2[0] is None and np.array_equal(only2[1], v2)


def test_offset_zero_is_rip_checksums():
    for d in oc.discs():
        arena, descs = _packed(d)
        v1, v2 = replaygain.rip_offsets_arena(None, 0, descs, d.flags, 40, arena)
        recs = replaygain.rip_checksums_arena(None, 0, descs, d.flags, arena)
        assert [(int(a), int(b)) for a, b in zip(v1[:, 40], v2[:, 40])] == [(r.arv1, r.arv2) for r in recs], d.name


@pytest.mark.parametrize("radius", [oc.RADIUS_MAX, 40])
def test_the_sliding_recurrence_equals_the_definition_with_every_flag_on_every_track(radius):
    want = oc.restated(radius)
    for d in oc.discs():
        arena, descs = _packed(d)
        s1, none = replaygain.rip_offsets_arena(None, 2, descs, d.flags, radius, arena, (True, False))
        assert none is None and np.array_equal(s1, want[d.name][0]), d.name
    d = next(x for x in oc.discs() if x.name == "mixed_b")
    arena, descs = _packed(d)
    for shift in range(4):  # all four flag combinations on every track, the middle ones too
        flags = [rc.ALL_FLAGS[(t + shift) % 4] for t in range(len(d.tracks))]
        v1, _ = replaygain.rip_offsets_arena(None, 0, descs, flags, radius, arena, (True, False))
        s1, _ = replaygain.rip_offsets_arena(None, 2, descs, flags, radius, arena, (True, False))
        assert np.array_equal(s1, v1), flags
        if radius == 40:
            r1, _ = oc.restate(oc.Disc("flags", d.tracks, flags), radius)
            assert np.array_equal(v1, r1), flags


def test_an_impulse_gives_the_closed_form():
    """One non-zero word v at disc frame j: track t at offset o sees it at position i = j - B_t - o + 1, so arv1 = lo32(v i) and
    arv2 = lo32(v i) + hi32(v i) where that position counts, and 0 elsewhere."""
    lens = [3000, 2, 7000, 1, 4000]
    flags = [rc.FIRST, 0, rc.FIRST | rc.LAST, 0, rc.LAST]
    bases = np.concatenate([[0], np.cumsum(lens)])
    radius = oc.RADIUS_MAX
    for j, (l, r) in ((0, (-1, -1)), (3001, (0x1234, -32768)), (6500, (-2, 0x7FFF)), (int(bases[-1]) - 1, (1, 0))):
        tracks = [(np.zeros(n, np.int16), np.zeros(n, np.int16)) for n in lens]
        t_of = int(np.searchsorted(bases, j, side="right")) - 1
        tracks[t_of][0][j - bases[t_of]] = l
        tracks[t_of][1][j - bases[t_of]] = r
        v = (l & 0xFFFF) | ((r & 0xFFFF) << 16)
        disc = oc.Disc("impulse", tracks, flags)
        arena, descs = _packed(disc)
        v1, v2 = replaygain.rip_offsets_arena(None, 0, descs, flags, radius, arena)
        for t, n in enumerate(lens):
            lo, hi = rc.ar_range(n, flags[t])
            i = j - int(bases[t]) - np.arange(-radius, radius + 1, dtype=np.int64) + 1
            counts = (i >= max(lo, 1)) & (i <= hi)
            p = np.where(counts, i, 0).astype(np.uint64) * np.uint64(v)
            assert np.array_equal(v1[t], (p & oc.M32).astype(np.uint32)), (j, t)
            assert np.array_equal(v2[t], (((p & oc.M32) + (p >> np.uint64(32))) & oc.M32).astype(np.uint32)), (j, t)


def test_argument_errors():
    arena = np.zeros(64, dtype=np.uint8)
    good = _capi.TrackDesc(0, 16, 44100, 2, _capi.FMT_S16_PLANAR)

    def fails(code, text, route, descs, radius, want=(True, True), flags=None):
        with pytest.raises(replaygain.ReplayGainError) as e:
            replaygain.rip_offsets_arena(None, route, descs, flags, radius, arena, want)
        assert e.value.code == code and text in str(e.value), str(e.value)

    fails(-1, "radius", 0, [good], -1)
    fails(-1, "radius", 0, [good], _capi.RIP_OFFSET_MAX + 1)
    fails(-1, "radius", 2, [good], 5000, (True, False))
    fails(-1, "route", 3, [good], 1)
    fails(-1, "route", -1, [good], 1)
    fails(-1, "arv1 only", 2, [good], 1, (True, True))
    fails(-1, "at most 1024", 0, [good] * (_capi.RIP_DISC_MAX_TRACKS + 1), 1)
    fails(-1, "beyond the arena", 0, [_capi.TrackDesc(0, 17, 44100, 2, _capi.FMT_S16_PLANAR)], 1)
    fails(-1, "beyond the arena", 0, [good, _capi.TrackDesc(2, 16, 44100, 2, _capi.FMT_S16_PLANAR)], 1)
    fails(-1, "sample-aligned", 0, [_capi.TrackDesc(1, 4, 44100, 2, _capi.FMT_S16_PLANAR)], 1)
    fails(-9, "channel", 0, [_capi.TrackDesc(0, 16, 44100, 1, _capi.FMT_S16_PLANAR)], 1)
    fails(-9, "16-bit planar", 2, [_capi.TrackDesc(0, 4, 44100, 2, _capi.FMT_F32_PLANAR)], 1, (True, False))
    L = _capi.load()  # route 1 has no host twin to fall back to: without a context it is an error
    assert L.rg_rip_offsets_arena(None, 1, 0, None, None, 1, None, 0, None, None) == -1
    v1, v2 = replaygain.rip_offsets_arena(None, 0, [], None, 7, arena)  # n = 0 is RG_OK
    assert v1.shape == (0, 15) and v2.shape == (0, 15)
    v1, v2 = replaygain.rip_offsets_arena(None, 0, [good] * _capi.RIP_DISC_MAX_TRACKS, None, 1, arena)  # 1024 aliased tracks of zeros
    assert v1.shape == (1024, 3) and not v1.any() and not v2.any()
    assert replaygain.rip_offsets_arena(None, 0, [good], [3], 2, arena, (False, False)) == (None, None)
    assert replaygain.rip_offsets_kernel_shape() == (4096, 256)


# ---- riplog.find_offset ----------------------------------------------------------------------------------------------------------
def _table(n, radius, seed=1):
    rng = np.random.default_rng(seed)
    # distinct values everywhere, so that only constructed coincidences match
    vals = rng.permutation(np.arange(1, 2 * n * (2 * radius + 1) + 1, dtype=np.uint32) * np.uint32(7919)).reshape(2, n, 2 * radius + 1)
    return SimpleNamespace(radius=radius, arv1=vals[0].copy(), arv2=vals[1].copy())


def _sections(tab, o, which=(True, True)):
    r = tab.radius
    return [riplog.LogTrack(t + 1, arv1=int(tab.arv1[t][o + r]) if which[0] else None, arv2=int(tab.arv2[t][o + r]) if which[1] else None)
            for t in range(len(tab.arv1))]


def test_find_offset_finds_the_common_offset():
    tab = _table(4, 30)
    for o in (6, -7, 0, 30, -30):
        s = riplog.find_offset(_sections(tab, o), tab)
        assert (s.offset, s.tracks, s.signatures) == (o, 4, 8) and f"{o:+d}" in s.text
    s = riplog.find_offset(_sections(tab, 5, (False, True)), tab)
    assert (s.offset, s.tracks, s.signatures) == (5, 4, 4)
    secs = _sections(tab, -3)
    secs[1] = riplog.LogTrack(2, copy_crc=0x12345678)  # a section without AccurateRip values takes no part
    s = riplog.find_offset(secs, tab)
    assert (s.offset, s.tracks, s.signatures) == (-3, 3, 6)
    assert riplog.find_offset(secs + [riplog.LogTrack(5, arv1=1)], tab).offset == -3  # a section beyond the table's tracks


def test_find_offset_takes_the_smallest_and_on_a_tie_the_negative_offset():
    tab = _table(2, 20)
    r = tab.radius
    for t in range(2):  # the same pair of values at -4, +4 and +9
        for o in (4, 9):
            tab.arv1[t][o + r] = tab.arv1[t][-4 + r]
            tab.arv2[t][o + r] = tab.arv2[t][-4 + r]
    assert riplog.find_offset(_sections(tab, 9), tab).offset == -4
    tab.arv2[1][-4 + r] ^= 1  # -4 drops out for one signature: +4 is the smallest left
    assert riplog.find_offset(_sections(tab, 9), tab).offset == 4


def test_find_offset_with_a_zero_track_nothing_logged_and_a_conflict():
    tab = _table(3, 10)
    tab.arv1[1][:] = 0  # digital silence matches everywhere and constrains nothing
    tab.arv2[1][:] = 0
    s = riplog.find_offset(_sections(tab, -2), tab)
    assert (s.offset, s.tracks, s.signatures) == (-2, 3, 6)
    allzero = SimpleNamespace(radius=10, arv1=np.zeros((2, 21), np.uint32), arv2=np.zeros((2, 21), np.uint32))
    assert riplog.find_offset(_sections(allzero, 3), allzero).offset == 0
    nothing = riplog.find_offset([riplog.LogTrack(1, crc32=5), riplog.LogTrack(2), riplog.LogTrack(3)], tab)
    assert (nothing.offset, nothing.tracks, nothing.signatures) == (None, 0, 0) and nothing.text == "nothing to compare"
    assert riplog.find_offset([], tab).text == "nothing to compare"
    tab = _table(3, 10, seed=2)
    secs = _sections(tab, 3)
    secs[2] = _sections(tab, -5)[2]  # the tracks disagree
    s = riplog.find_offset(secs, tab)
    assert s.offset is None and s.signatures == 6 and "no common offset" in s.text
    secs = _sections(tab, 3)
    secs[0].arv2 ^= 0x10  # the versions disagree
    assert riplog.find_offset(secs, tab).offset is None


def test_compare_at_an_offset():
    sec = riplog.LogTrack(1, copy_crc=1, crc32=2, arv1=10, arv2=20)
    v = riplog.compare_at(sec, 6, 10, 20)
    assert v.ok and v.offset == 6 and v.text == "match at offset +6; CRC-32 not comparable at offset +6"
    assert [(n, ok) for n, _, _, ok in v.checks] == [("Copy CRC", None), ("CRC32 hash", None), ("AccurateRip v1", True), ("AccurateRip v2", True)]
    assert v.check_text(None) == "not comparable at offset +6" and v.check_text(True) == "match at offset +6"
    v = riplog.compare_at(sec, -7, 10, 21)
    assert not v.ok and v.text.startswith("mismatch: AccurateRip v2")
    assert riplog.compare_at(riplog.LogTrack(1, arv1=10), -7, 10, 0).text == "match at offset -7"
    same = riplog.compare(sec, SimpleNamespace(crc32=2, crc32_nonnull=1, arv1=10, arv2=20))  # offset 0: as before
    assert same.ok and same.text == "match" and same.offset == 0


# ---- the command line's option errors ----------------------------------------------------------------------------------------------
def test_rip_offsets_option_errors():
    from mp3rgain_amd import cli

    def run(*args):
        out, err = io.StringIO(), io.StringIO()
        return cli.main(list(args), out, err), out.getvalue(), err.getvalue()

    code, _, err = run("--rip-offsets", "a.wav")
    assert code != 0 and "--rip-offsets requires --rip" in err
    code, _, err = run("--rip", "--rip-offsets", "a.wav")
    assert code != 0 and "--rip-offsets requires --rip-log" in err
    code, _, err = run("--rip-offsets", "--rip-log", "x.log", "a.wav")
    assert code != 0 and "requires --rip" in err
    code, out, _ = run("-h")
    assert "--rip-offsets" in out
