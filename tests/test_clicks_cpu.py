"""The click scan on the host (include/mp3rgain_amd_clicks.h): the serial twin (rg_clicks_arena route 0) and the kernels' tile and
fold code on one lane (route 2) on the shared cases (tests/clicks_cases.py), byte for byte against each other, records and event
lists, and field for field against the Python restatement, in the arena layouts every PCM-reading kernel is held to; the
refusals and their texts; and both routes under AddressSanitizer + UndefinedBehaviorSanitizer in a stand-alone driver with its
own main (tests/san/clicks_driver.cpp with rg_clicks_host.cpp only), run as a child process.  No GPU, nothing loaded into Python
under a sanitizer."""
import ctypes as C
import shutil
import struct
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))
import arena_layouts as al  # noqa: E402
import clicks_cases as cc  # noqa: E402

import mp3rgain_amd as rg  # noqa: E402
from mp3rgain_amd import _capi  # noqa: E402

RG_ERR_INVALID_ARG, RG_ERR_FORMAT = -1, -9
S16, S32, F32 = _capi.FMT_S16_PLANAR, _capi.FMT_S32_PLANAR, _capi.FMT_F32_PLANAR
LAYOUTS = [al.Layout("abut", "loud", "input"), al.Layout("abut", "loud", "reversed"), al.Layout("guard", "nan", "reversed", 1)] + \
          [al.Layout("guard", "loud", "input", s) for s in (0, 2, 4, 5, 6)]
SHORT_SAMPLES = 1400  # what a layout run keeps of a group


def _raw(recs):
    return b"".join(bytes(r) for r in recs)


def _run(route, tracks, o, layout=al.Layout("guard", "loud", "input", 3)):
    arena, descs, _ = al.pack(tracks, layout)
    return rg.clicks_arena(None, route, list(descs)[:len(tracks)], arena, **o._asdict())


def _rows(rows, k, K):
    return rows[k * K:(k + 1) * K] if K else []


@pytest.mark.parametrize("group", cc.groups(), ids=lambda g: g.name)
def test_host_routes_match_each_other_and_the_restatement(group):
    tracks, want, K = list(group.tracks), cc.wants(group.name), group.opts.max_events
    serial, s_rows = _run(0, tracks, group.opts)
    folded, f_rows = _run(2, tracks, group.opts)
    bad = [(tr.name, d) for k, (tr, r) in enumerate(zip(tracks, serial)) for d in [cc.differences(cc.got(r, _rows(s_rows, k, K)), want[tr.name])] if d]
    assert not bad, f"{len(bad)} of {len(tracks)} records of the serial twin differ from the restatement: {bad[:3]}"
    diff = [(tr.name, cc.differences(cc.got(a, _rows(f_rows, k, K)), cc.got(b, _rows(s_rows, k, K)) | {"ch": cc.got(b, [])["ch"], "list": cc.got(b, _rows(s_rows, k, K))["list"]}))
            for k, (tr, a, b) in enumerate(zip(tracks, folded, serial)) if bytes(a) != bytes(b)]
    assert _raw(folded) == _raw(serial), diff[:3]
    assert bytes(f_rows) == bytes(s_rows)


@pytest.mark.parametrize("layout", LAYOUTS, ids=lambda l: f"{l.gap}-{l.guard}-{l.order}-{l.shift}")
def test_host_routes_in_every_layout(layout):
    """What lies around a plane (other tracks, full-scale or NaN guards) reaches no record and no event."""
    for group in cc.groups():
        tracks = [tr for tr in group.tracks if len(tr.channels[0]) <= SHORT_SAMPLES]
        if len(tracks) < 3:
            continue
        want, K = cc.wants(group.name), group.opts.max_events
        serial, s_rows = _run(0, tracks, group.opts, layout)
        folded, f_rows = _run(2, tracks, group.opts, layout)
        assert _raw(folded) == _raw(serial) and bytes(f_rows) == bytes(s_rows), group.name
        bad = [tr.name for k, (tr, r) in enumerate(zip(tracks, serial)) if cc.differences(cc.got(r, _rows(s_rows, k, K)), want[tr.name])]
        assert not bad, (group.name, bad[:5])


def test_the_case_list_covers_what_it_claims():
    by = {(g.name, tr.name): (g, tr) for g in cc.groups() for tr in g.tracks}
    names = {g.opts: g.name for g in cc.groups()}
    dflt, small, big = names[cc.Opts()], names[cc.Opts(block_samples=256, order=2)], names[cc.Opts(block_samples=4096, order=12)]
    wide = names[cc.Opts(block_samples=4096, order=12, gap=255, max_width=4095)]
    assert {tr.channels[0].dtype for _, tr in by.values()} == {np.dtype(np.int16), np.dtype(np.int32), np.dtype(np.float32)}
    assert {len(tr.channels) for _, tr in by.values()} >= {1, 2, 8}
    assert [rg.clicks_kernel_shape(b)[:3] for b in (256, 512, 1024, 2048, 4096)] == [(11776, 46, 256), (11264, 22, 256), (10240, 10, 256), (8192, 4, 256),
                                                                                    (4096, 1, 256)]
    assert rg.clicks_kernel_shape(1024)[3] <= 160 * 1024
    T = cc.tile_samples(4096)
    for tag in ("s16", "s32", "f32"):
        for name, B, P in ((dflt, 1024, 8), (small, 256, 2), (big, 4096, 12)):
            for N in (0, 1, P - 1, P, P + 1, 4 * P - 1, 4 * P, B - 1, B, B + 1, 2 * B + 1, 3 * B, B + 4 * P - 1):
                assert (name, f"{tag}_noise_n{N}") in by
        for N in (T - 1, T, T + 1, 2 * T + 1):
            assert (big, f"{tag}_noise_n{N}") in by
        # the constructed places: one event at `gap`, two at `gap` + 1, whatever cut lies between
        for name in (dflt, small, big):
            for where in ("block", "cut"):
                one, two = cc.wants(name)[f"{tag}_gap_{where}"]["ch"][0], cc.wants(name)[f"{tag}_gap+1_{where}"]["ch"][0]
                g = by[(name, f"{tag}_gap_{where}")][0].opts.gap
                assert (one["flagged"], one["clicks"], one["widest"]) == (6, 1, g + 5) and (two["flagged"], two["clicks"], two["widest"]) == (6, 2, 3), (name, where)
        w = cc.wants(wide)[f"{tag}_tile_cut_gap"]
        assert [c["clicks"] for c in w["ch"]] == [1, 2] and w["ch"][0]["widest"] == 255 + 5
        w = cc.wants(wide)[f"{tag}_spans_a_tile"]
        assert (w["ch"][0]["bursts"], w["ch"][0]["clicks"], w["ch"][0]["widest"]) == (1, 0, 200 * ((T + 699) // 200) + 3) and w["ch"][1]["clicks"] == 1
        assert w["ch"][0]["widest"] > T + 400  # from the tile before, through a whole tile, into the tile behind
        assert w["list"][0]["kind"] == _capi.CK_KIND_BURST and w["list"][0]["start"] == T - 400
        # widths on either side of max_width
        a, b = cc.wants(dflt)[f"{tag}_width32"]["ch"][0], cc.wants(dflt)[f"{tag}_width33"]["ch"][0]
        assert (a["clicks"], a["bursts"], a["widest"], b["clicks"], b["bursts"], b["widest"]) == (1, 0, 32, 0, 1, 33)
        # exactly K events and K + 1; K = 0 lists nothing and says so
        for opts, K in ((cc.Opts(), 16), (cc.Opts(max_events=0), 0), (cc.Opts(max_events=3), 3)):
            for k in (16, 17):
                w = cc.wants(names[opts])[f"{tag}_events{k}"]
                assert w["events"] == k + 1 and w["listed"] == min(k + 1, K) and bool(w["flags"] & _capi.CK_TRUNCATED) == (k + 1 > K)
        w = cc.wants(dflt)[f"{tag}_events16"]
        assert [(e["start"], e["channel"]) for e in w["list"][:3]] == [(100, 0), (165, 1), (230, 0)]
        # several channels at the same sample: by (start, channel); the clean channel has nothing
        w = cc.wants(dflt)[f"{tag}_eight_channels"]
        assert [(e["channel"]) for e in w["list"][:7]] == [0, 1, 2, 4, 5, 6, 7] and w["ch"][3]["flagged"] == 0
        assert len({e["start"] for e in w["list"][:2]}) == 1
        # silence between music: the all-zero block falls back; the click planted behind the silence is found (so are the hard cuts
        # into and out of the silence, which are discontinuities of their own)
        w = cc.wants(dflt)[f"{tag}_zeros_between_music"]
        assert w["ch"][0]["fallback_blocks"] >= 1 and any(abs(e["start"] - (4 * 1024 + 10)) <= 9 for e in w["list"])
    w, w1 = cc.wants(dflt)["s16_file_events16"], cc.wants(dflt)["s16_file_events17"]
    assert (w["events"], w["listed"], len(w["list"]), w["flags"] & _capi.CK_TRUNCATED) == (16, 16, 16, 0) and w["list"][15]["channel"] == 1
    assert (w1["events"], w1["listed"], len(w1["list"]), w1["flags"] & _capi.CK_TRUNCATED) == (17, 16, 16, _capi.CK_TRUNCATED) and w1["list"][15]["channel"] == 0
    for where in ("first", "middle", "last"):
        assert cc.wants(dflt)[f"f32_nonfinite_{where}"]["nonfinite"] == 2
    w = cc.wants(dflt)["f32_all_nan"]
    assert w["nonfinite"] == 300 and w["flags"] == _capi.CK_COMPLETE | _capi.CK_SILENT | _capi.CK_NONFINITE
    assert "s16_two_tiles" in cc.wants(dflt) and "s16_two_tiles" in cc.wants(small)


def test_options_and_refusals():
    arena = np.zeros(64, dtype=np.uint8)
    ok = _capi.TrackDesc(0, 4, 44100, 2, S16)
    for route in (0, 2):
        for desc, opts, code, text in ((_capi.TrackDesc(0, 17, 44100, 2, S16), {}, RG_ERR_INVALID_ARG, "beyond the arena"),
                                       (_capi.TrackDesc(1, 4, 44100, 2, S16), {}, RG_ERR_INVALID_ARG, "sample-aligned"),
                                       (_capi.TrackDesc(2, 4, 44100, 2, S32), {}, RG_ERR_INVALID_ARG, "sample-aligned"),
                                       (_capi.TrackDesc(0, 1, 44100, 9, S16), {}, RG_ERR_FORMAT, "9 channel(s), the click scan takes 1 to 8"),
                                       (_capi.TrackDesc(0, 1, 44100, 0, S16), {}, RG_ERR_FORMAT, "0 channel"),
                                       (_capi.TrackDesc(0, 1, 44100, 2, 7), {}, RG_ERR_FORMAT, "format 7"),
                                       (ok, {"block_samples": 1000}, RG_ERR_INVALID_ARG, "clicks: block_samples 1000 is not 256, 512, 1024, 2048 or 4096"),
                                       (ok, {"block_samples": 8192}, RG_ERR_INVALID_ARG, "block_samples 8192"),
                                       (ok, {"order": 7}, RG_ERR_INVALID_ARG, "clicks: order 7 is not an even number in 2 .. 12"),
                                       (ok, {"order": 0}, RG_ERR_INVALID_ARG, "order 0"),
                                       (ok, {"order": 14}, RG_ERR_INVALID_ARG, "order 14"),
                                       (ok, {"ratio_permille": 999}, RG_ERR_INVALID_ARG, "clicks: ratio_permille 999 is not in 1000 .. 1000000"),
                                       (ok, {"ratio_permille": 1000001}, RG_ERR_INVALID_ARG, "ratio_permille 1000001"),
                                       (ok, {"floor": 0}, RG_ERR_INVALID_ARG, "clicks: floor 0 is not in 1 .. 32767"),
                                       (ok, {"floor": 32768}, RG_ERR_INVALID_ARG, "floor 32768"),
                                       (ok, {"gap": 0}, RG_ERR_INVALID_ARG, "clicks: gap 0 is not in 1 .. 255"),
                                       (ok, {"gap": 256}, RG_ERR_INVALID_ARG, "gap 256"),
                                       (ok, {"max_width": 0}, RG_ERR_INVALID_ARG, "clicks: max_width 0 is not in 1 .. 4095"),
                                       (ok, {"max_width": 4096}, RG_ERR_INVALID_ARG, "max_width 4096")):
            with pytest.raises(rg.ReplayGainError) as e:
                rg.clicks_arena(None, route, [desc], arena, **opts)
            assert e.value.code == code and text in str(e.value), (route, str(e.value))
        recs, rows = rg.clicks_arena(None, route, [_capi.TrackDesc(0, 4, 44100, 8, S16)], arena)
        r = recs[0]
        assert (r.status, r.channels, r.block_samples, r.order, r.ratio_permille, r.floor, r.gap, r.max_width, r.max_events) == (
            0, 8, 1024, 8, _capi.CK_DEFAULT_RATIO_PERMILLE, 4, 16, 32, 16)
        assert r.flags == _capi.CK_COMPLETE | _capi.CK_SILENT and r.ch[7].first_click == 4 and r.ch[7].fallback_blocks == 1 and len(rows) == 16
        recs, rows = rg.clicks_arena(None, route, [_capi.TrackDesc(0, 0, 44100, 2, S16)], arena, max_events=256, gap=255, max_width=4095, floor=32767,
                                     ratio_permille=1000000, block_samples=4096, order=12)
        assert (recs[0].frames, recs[0].flags, recs[0].max_events, len(rows)) == (0, _capi.CK_COMPLETE | _capi.CK_SILENT, 256, 256)
        assert rg.clicks_arena(None, route, [], arena)[0] == []
    # max_events beyond 256 is refused by the library (the Python wrapper sizes its rows by the clamped value)
    o = _capi.ClicksOpts(1024, 8, 15000, 4, 16, 32, 257)
    out, rows = (_capi.ClicksRecord * 1)(), (_capi.ClicksEvent * 300)()
    d = (_capi.TrackDesc * 1)(ok)
    assert _capi.load().rg_clicks_arena(None, 0, 1, d, C.byref(o), arena.ctypes.data, arena.size, out, rows) == RG_ERR_INVALID_ARG
    assert b"clicks: max_events 257 is not in 0 .. 256" in _capi.load().rg_last_error(None)
    with pytest.raises(rg.ReplayGainError) as e:
        rg.clicks_arena(None, 3, [ok], arena)
    assert e.value.code == RG_ERR_INVALID_ARG
    assert _capi.load().rg_clicks_arena(None, 1, 0, None, None, None, 0, None, None) == RG_ERR_INVALID_ARG  # the kernels need a context
    with pytest.raises(rg.ReplayGainError):
        rg.clicks_kernel_shape(1000)
    assert (C.sizeof(_capi.ClicksRecord), C.sizeof(_capi.ClicksOpts), C.sizeof(_capi.ClicksChannel), C.sizeof(_capi.ClicksEvent)) == (400, 28, 40, 20)


def test_records_become_objects_and_options_move_the_flags():
    rng = np.random.default_rng(5)
    x = cc.tonal(rng, 3000)
    x[1500] += 9000
    arena = np.concatenate([x, x]).astype(np.int16).view(np.uint8)
    d = [_capi.TrackDesc(0, 3000, 44100, 2, S16)]
    recs, rows = rg.clicks_arena(None, 0, d, arena)
    c = rg.clicks_from_record(recs[0], rows)
    assert (c.frames, c.channels, c.clicks, c.bursts, c.listed, len(c.events), c.complete, c.truncated, c.error) == (3000, 2, 2, 0, 2, 2, True, False, None)
    assert c.first_click[1] == 0 and abs(c.first_click[0] - 1500) <= 9 and c.strongest_click[0] == c.ch[0].strongest_permille > 20000
    assert [(e.channel, e.kind) for e in c.events] == [(0, "click"), (1, "click")] and c.events[0].start == c.ch[0].first_click
    quiet = rg.clicks_from_record(*[v[0] if k == 0 else v for k, v in enumerate(rg.clicks_arena(None, 0, d, arena, ratio_permille=1000000))])
    assert quiet.clicks == 0 and quiet.events == [] and quiet.first_click is None and quiet.strongest_click is None
    narrow = rg.clicks_arena(None, 2, d, arena, max_width=1)[0][0]
    assert narrow.flags & _capi.CK_BURSTS and not narrow.flags & _capi.CK_CLICKS


# ---- the host routes under the sanitizers ------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    tmp = tmp_path_factory.mktemp("san")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    # does this toolchain have the sanitizers' runtimes at all?  A trivial program of the test's own says so; after that a
    # failing build of the project's sources is a failure, whatever its diagnostics mention
    probe = tmp / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    r = subprocess.run(["g++"] + san + [str(probe), "-o", str(tmp / "probe")], capture_output=True, text=True)
    if r.returncode != 0 or subprocess.run([str(tmp / "probe")], capture_output=True).returncode != 0:
        pytest.skip("this toolchain has no sanitizer runtime")
    out = tmp / "clicks_driver"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off"] + san + [f"-I{ROOT / 'include'}", str(ROOT / "tests" / "san" / "clicks_driver.cpp"),
                                                                           str(ROOT / "mp3rgain_amd" / "csrc" / "rg_clicks_host.cpp"), "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return out


def test_host_routes_under_asan_ubsan(driver, tmp_path):
    """Every case's arena through both host routes of a sanitized build: clean, the two routes' bytes equal, and the records the
    restatement's."""
    chosen = [(g, tr) for g in cc.groups() for tr in g.tracks]
    files = []
    for k, (g, tr) in enumerate(chosen):
        p = tmp_path / f"{k:03d}.bin"
        dt = tr.channels[0].dtype
        p.write_bytes(struct.pack("<Q10I", len(tr.channels[0]), len(tr.channels), al.FMT[dt], tr.sample_rate, *g.opts)
                      + b"".join(np.ascontiguousarray(ch, dt.newbyteorder("<")).tobytes() for ch in tr.channels))
        files.append(str(p))
    r = subprocess.run([str(driver)] + files, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    assert r.stderr == ""
    lines = [ln.split(" ") for ln in r.stdout.split("\n")[:-1]]
    assert len(lines) == 2 * len(chosen)
    for k, (g, tr) in enumerate(chosen):
        serial, folded = lines[2 * k], lines[2 * k + 1]
        assert serial[:2] == [files[k], "0"] and folded[:2] == [files[k], "2"] and serial[2:] == folded[2:], tr.name
        rec = _capi.ClicksRecord.from_buffer_copy(bytes.fromhex(serial[2]))
        K = g.opts.max_events
        row = (_capi.ClicksEvent * max(1, K)).from_buffer_copy(bytes.fromhex(serial[3]).ljust(20 * max(1, K), b"\0"))
        assert not cc.differences(cc.got(rec, list(row)[:K]), cc.wants(g.name)[tr.name]), tr.name
