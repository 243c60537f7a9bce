"""Many albums in one call (rg_analyze_albums, rg_analyze_albums_node): every album's result equals rg_analyze_album on that
album field for field, every file's result equals the per-album call's, under every route the file layer takes (parts on
and off, one loader thread, groups small enough that albums straddle them); the albums against the CPU oracle's fold of its
own track histograms; a failing file ends its album only, with analyze_album_files' code and text; the node keeps albums
whole; malformed album boundaries are refused."""
import ctypes as C
import os
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import wavutil  # noqa: E402
from wavutil import planar_for_oracle, wav_bytes  # noqa: E402

import mp3rgain_amd as rg  # noqa: E402
from mp3rgain_amd import _capi  # noqa: E402

pytestmark = pytest.mark.gpu
GOLDEN = Path(__file__).resolve().parent / "golden"
_signal = wavutil.test_signal  # (not imported under its own name: pytest would collect it)


@pytest.fixture()
def an(_ctx):
    _ctx.set_kernel(0)
    for key in (1, 2, 4, 7, 10, 11, 12, 13):
        _ctx.set_tuning(key, 0)
    _ctx.set_tuning(14, 1)
    _ctx.set_decoder_command(None)
    yield _ctx
    for key in (7, 10, 11, 12, 13):
        _ctx.set_tuning(key, 0)


@pytest.fixture(scope="module")
def mixed(tmp_path_factory):
    """MP3 goldens, undamaged FLAC fixtures at supported rates, synthesized WAVs at several rates, mono and stereo."""
    d = tmp_path_factory.mktemp("albums_mixed")
    files = sorted((GOLDEN / "mp3").glob("*.mp3")) + sorted((GOLDEN / "fixtures").glob("test_*.mp3"))
    files += [f for f in sorted((GOLDEN / "flac").glob("*.flac")) if not f.name.startswith("damaged_") and "192k" not in f.name]
    for k, (rate, nch, kind) in enumerate([(44100, 2, "s16"), (48000, 1, "f32"), (22050, 2, "s24"), (96000, 2, "s16"),
                                           (8000, 1, "u8"), (32000, 2, "s32"), (88200, 1, "s16"), (16000, 2, "f32")]):
        frames = int(rate * (0.4 + 0.15 * k))
        f = d / f"w{k}_{rate}_{nch}.wav"
        f.write_bytes(wav_bytes(_signal(kind, rate, frames, nch, 100 + k), rate, kind))
        files.append(f)
    return files


def _partition(files, seed, max_album=7, empty=True):
    rng = np.random.default_rng(seed)
    order = list(rng.permutation(len(files)))
    albums = []
    while order:
        k = int(rng.integers(1, max_album + 1))
        albums.append([files[i] for i in order[:k]])
        order = order[k:]
    if empty:
        albums.insert(int(rng.integers(0, len(albums) + 1)), [])
        albums.append([])
    return albums


def _same_as_per_album(an, albums, got):
    assert len(got) == len(albums)
    for files, g in zip(albums, got):
        try:
            want = an.analyze_album_files(files)
        except rg.ReplayGainError as e:
            assert isinstance(g, rg.ReplayGainError), files
            assert (g.code, str(g)) == (e.code, str(e))
            continue
        assert isinstance(g, rg.AlbumGainResult), (files, g)
        assert (g.album_loudness_db, g.album_gain_db, g.album_peak) == (want.album_loudness_db, want.album_gain_db, want.album_peak)
        assert g.album_gain_steps() == want.album_gain_steps()
        assert g.tracks == want.tracks


ROUTES = {
    "default": {},
    "parts_off": {10: 1},
    "parts_on": {10: 2},
    "parts_every_chunk": {10: 2, 11: 1, 12: 65536},
    "one_loader": {7: 1},
    "small_groups": {13: 3 << 20},
    "small_groups_parts": {13: 3 << 20, 10: 2, 11: 1},
}


@pytest.mark.parametrize("route", list(ROUTES))
def test_albums_equal_per_album_calls(an, mixed, route):
    for key, value in ROUTES[route].items():
        an.set_tuning(key, value)
    for seed in (1, 2):
        albums = _partition(mixed, seed)
        _same_as_per_album(an, albums, an.analyze_albums_files(albums))
    # MPEG streams only: groups the loader pipeline takes whole, where the parts (when on) stay the route to the end
    albums = _partition([f for f in mixed if f.suffix == ".mp3"], 3)
    _same_as_per_album(an, albums, an.analyze_albums_files(albums))


def test_albums_raw_results_and_empty_album(an, mixed):
    """The C call's per-album record, album status and per-file status; an empty album is what rg_analyze_album gives for n = 0."""
    lib = _capi.load()
    albums = [[], mixed[:3], [], mixed[3:4], []]
    flat = [os.fsencode(str(f)) for a in albums for f in a]
    first = [0]
    for a in albums:
        first.append(first[-1] + len(a))
    n, na = len(flat), len(albums)
    paths = (C.c_char_p * n)(*flat)
    fa = (C.c_size_t * (na + 1))(*first)
    out, st = (_capi.TrackResult * n)(), (C.c_int32 * n)()
    alb, ast = (_capi.AlbumResult * na)(), (C.c_int32 * na)()
    assert lib.rg_analyze_albums(an._ctx, paths, n, fa, na, -1, out, st, alb, ast) == 0
    assert list(st) == [0] * n and list(ast) == [0] * na
    empty = _capi.AlbumResult()
    none = (_capi.TrackResult * 1)()
    assert lib.rg_analyze_album(an._ctx, (C.c_char_p * 1)(), 0, -1, none, C.byref(empty)) == 0
    for a in (0, 2, 4):
        assert bytes(alb[a]) == bytes(empty)
    for a in (1, 3):
        one = _capi.AlbumResult()
        k = first[a + 1] - first[a]
        tr = (_capi.TrackResult * k)()
        assert lib.rg_analyze_album(an._ctx, (C.c_char_p * k)(*flat[first[a]:first[a + 1]]), k, -1, tr, C.byref(one)) == 0
        assert bytes(alb[a]) == bytes(one)
        assert [bytes(out[i]) for i in range(first[a], first[a + 1])] == [bytes(t) for t in tr]


def test_albums_against_the_oracle(an, oracle, tmp_path):
    """200 albums of 1-6 short synthesized tracks: loudness, gain and peak equal the oracle's fold of its own track histograms."""
    rng = np.random.default_rng(77)
    rates = (44100, 48000, 32000, 22050, 16000, 96000)
    albums, wants = [], []
    k = 0
    for a in range(200):
        files, hists, peaks = [], [], []
        for t in range(int(rng.integers(1, 7))):
            rate = int(rates[int(rng.integers(0, len(rates)))])
            nch = int(rng.integers(1, 3))
            frames = int(rate * rng.uniform(0.12, 0.5))
            sig = _signal("s16", rate, frames, nch, 5000 + k)
            f = tmp_path / f"a{a:03d}_{t}.wav"
            f.write_bytes(wav_bytes(sig, rate, "s16"))
            pl = planar_for_oracle(sig, "s16")
            res, hist = oracle.analyze_pcm(pl[0], pl[1] if nch == 2 else None, rate)
            files.append(f)
            hists.append(hist)
            peaks.append(res["peak"])
            k += 1
        albums.append(files)
        wants.append(oracle.album_from_hists(hists, peaks)[0])
    an.set_tuning(13, 4 << 20)  # several groups: albums straddle them
    got = an.analyze_albums_files(albums)
    for g, w in zip(got, wants):
        assert isinstance(g, rg.AlbumGainResult)
        assert (g.album_loudness_db, g.album_gain_db, g.album_peak) == (w["album_loudness_db"], w["album_gain_db"], w["album_peak"])


def _raw_wav(tag, bits, body, rate=44100, nch=2):
    """A RIFF/WAVE stream of any format tag: one the library parses but does not lay out (64-bit float, mu-law, ...)."""
    import struct

    align = nch * bits // 8
    fmt = struct.pack("<HHIIHH", tag, nch, rate, rate * align, align, bits)
    chunks = b"fmt " + struct.pack("<I", len(fmt)) + fmt + b"data" + struct.pack("<I", len(body)) + body
    return b"RIFF" + struct.pack("<I", 4 + len(chunks)) + b"WAVE" + chunks


def test_failing_file_ends_its_album_only(an, mixed, tmp_path):
    missing = tmp_path / "missing.mp3"
    junk = tmp_path / "junk.mp3"
    junk.write_bytes(b"not an audio stream\n" * 250)
    bad_rate = tmp_path / "bad_rate.wav"
    bad_rate.write_bytes(wav_bytes(_signal("s16", 44000, 30000, 2, 9), 44000, "s16"))
    f64 = tmp_path / "float64.wav"  # parses, passes every per-file check, but no de-interleave reads it
    f64.write_bytes(_raw_wav(3, 64, (0.25 * np.sin(np.arange(2 * 20000) / 9.0)).astype("<f8").tobytes()))
    mulaw = tmp_path / "mulaw.wav"
    mulaw.write_bytes(_raw_wav(7, 8, bytes(range(256)) * 100, rate=8000, nch=1))
    albums = _partition(mixed, 11, max_album=5, empty=False)
    assert len(albums) >= 8
    albums[1].insert(1, missing)
    albums[3].append(junk)
    albums[4].insert(0, bad_rate)
    albums[4].append(junk)  # a later failure does not replace the first
    albums[5].insert(1, f64)
    albums[7].append(mulaw)
    got = an.analyze_albums_files(albums)
    codes = {1: -8, 3: -9, 4: -2, 5: -9, 7: -9}
    assert str(got[5]) == f"Failed to probe format: {f64}" and str(got[7]) == f"Failed to probe format: {mulaw}"
    assert all(isinstance(g, rg.AlbumGainResult) for a, g in enumerate(got) if a not in codes)
    for a, code in codes.items():
        assert isinstance(got[a], rg.ReplayGainError) and got[a].code == code
    _same_as_per_album(an, albums, got)
    # the good files of a failed album still have their track results
    lib = _capi.load()
    flat = [f for a in albums for f in a]
    n = len(flat)
    first = np.cumsum([0] + [len(a) for a in albums])
    out, st = (_capi.TrackResult * n)(), (C.c_int32 * n)()
    alb, ast = (_capi.AlbumResult * len(albums))(), (C.c_int32 * len(albums))()
    assert lib.rg_analyze_albums(an._ctx, (C.c_char_p * n)(*[os.fsencode(str(f)) for f in flat]), n,
                                 (C.c_size_t * (len(albums) + 1))(*[int(x) for x in first]), len(albums), -1, out, st, alb, ast) == 0
    for i, f in enumerate(flat):  # every file as analyze_track_file takes it on its own
        try:
            want = an.analyze_track_file(f)
        except rg.ReplayGainError as e:
            assert (st[i], lib.rg_tracks_error(an._ctx, i).decode()) == (e.code, str(e))
            continue
        assert st[i] == 0 and rg.replaygain._to_result(out[i], out[i].file_type) == want


def test_node_keeps_albums_whole(an, mixed):
    albums = _partition(mixed, 21)
    single = an.analyze_albums_files(albums)
    with rg.Node([0, 0]) as node:
        node.set_tuning(14, 1)
        got = node.analyze_albums_files(albums)
        own = node.last_partition(sum(len(a) for a in albums))
    assert len(got) == len(single)
    for g, s in zip(got, single):
        if isinstance(s, rg.ReplayGainError):
            assert (g.code, str(g)) == (s.code, str(s))
        else:
            assert g == s
    k = 0
    for a in albums:
        assert len(set(own[k:k + len(a)])) <= 1
        k += len(a)
    assert set(own) == {0, 1}


@pytest.mark.parametrize("first, n_albums", [(None, 1), ([1, 2], 1), ([0, 1], 1), ([0, 2, 1, 2], 3)])
def test_malformed_album_first_is_refused(an, mixed, first, n_albums):
    lib = _capi.load()
    paths = (C.c_char_p * 2)(*[os.fsencode(str(f)) for f in mixed[:2]])
    fa = (C.c_size_t * len(first))(*first) if first is not None else None
    out, st = (_capi.TrackResult * 2)(), (C.c_int32 * 2)()
    alb, ast = (_capi.AlbumResult * 3)(), (C.c_int32 * 3)()
    assert lib.rg_analyze_albums(an._ctx, paths, 2, fa, n_albums, -1, out, st, alb, ast) == _capi.RG_ERR_INVALID_ARG
    assert lib.rg_last_error(an._ctx).decode().startswith("rg_analyze_albums: ")
