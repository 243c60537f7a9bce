"""The lossy ancestry scan on the host (include/mp3rgain_amd_ancestry.h): the serial twin (rg_ancestry_arena route 0) and the
kernels' cutting into phases and tiles (route 2) on the shared cases (tests/ancestry_cases.py), byte for byte against each
other, counts included; route 0 against the float64 reference built from oracle/mp3_encoder.py: the same r*, flags and
grid_offset on every case, and counts within TOLERANCE_FACTOR times the worst difference tools/ancestry_refcheck.py recorded
in tests/golden/ancestry_measured.json (route 0 against numpy, never the kernels against themselves).  No GPU."""
import ctypes as C
import json
import math
import re
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import ancestry_cases as ac  # noqa: E402

import mp3rgain_amd as rg  # noqa: E402
from mp3rgain_amd import _capi  # noqa: E402

RG_ERR_INVALID_ARG, RG_ERR_FORMAT = -1, -9
S16, S32, F32 = _capi.FMT_S16_PLANAR, _capi.FMT_S32_PLANAR, _capi.FMT_F32_PLANAR
ROOT = Path(__file__).resolve().parent.parent
MEASURED = json.loads(ac.MEASURED.read_text())


def _route(case, route):
    arena, descs = ac.pack_one(case)
    recs, cnt = rg.ancestry_arena(None, route, descs, arena, case.segments, case.granules)
    return recs[0], cnt[0]


@pytest.mark.parametrize("case", ac.cases(), ids=lambda c: c.name)
def test_host_routes_match_each_other_and_the_reference(case):
    serial, scnt = _route(case, 0)
    folded, fcnt = _route(case, 2)
    assert bytes(folded) == bytes(serial) and np.array_equal(fcnt, scnt), np.argwhere(fcnt != scnt)[:4].tolist()
    ref = ac.reference(case.name)
    assert (serial.status, serial.segments, serial.granules, serial.views, serial.frames) == (0, ref["S"], ref["G"], len(ref["views"]), len(case.channels[0]))
    assert serial.flags == ref["flags"] and serial.grid_offset == ref["grid_offset"], (serial.flags, ref["flags"], serial.grid_offset, ref["grid_offset"])
    assert serial.best_view == (_capi.ANC_NO_VIEW if ref["best_view"] is None else ref["best_view"])
    tol_s = ac.TOLERANCE_FACTOR * MEASURED["worst_small_error"]
    tol_a = ac.TOLERANCE_FACTOR * MEASURED["worst_active_error"]
    for v, (w, (small, active)) in enumerate(zip(ref["views"], ref["counts"])):
        got = serial.view[v]
        print(case.name, v, "z", got.z, w["z"], "iso", got.iso, w["iso"], "r*", got.offset, w["offset"])
        assert (got.kind, got.nonfinite, bool(got.flagged)) == (w["kind"], w["nonfinite"], w["flagged"])
        if w["active_total"]:
            assert got.offset == w["offset"]
        s32, a32 = scnt[v, 0].astype(np.int64), scnt[v, 1].astype(np.int64)
        assert (np.abs(a32 - active) <= tol_a * np.maximum(active, a32)).all()
        assert (np.abs(s32 - small) <= tol_s * np.maximum(active, a32)).all()
        # the finish itself, restated on the twin's own counts: the same numbers
        mine = ac.finish_view(s32, a32, *ac.thresholds())
        for f in ("ratio", "second", "p0", "z", "iso"):
            a, b = getattr(got, f), mine[f]
            assert a == b or abs(a - b) <= 1e-12 * max(abs(a), abs(b)), (f, a, b)
        assert (got.small, got.active, got.active_total, got.offset) == (mine["small"], mine["active"], mine["active_total"], mine["offset"])
    assert not scnt[len(ref["views"]):].any()


def test_verdicts_of_the_case_list():
    """Coded and expected found: flagged at the offset the construction gives; a stream coded mid/side is flagged in its mid or
    side view and carries RG_ANC_MIDSIDE; never coded: unflagged; the finely coded cases are present and UNFLAGGED (the stated
    limit).  No coded case lies within 10 % of a threshold."""
    z_min, iso_min = ac.thresholds()
    kinds = {k: [c for c in ac.cases() if c.kind == k] for k in ("found", "miss", "clean", "shape")}
    assert len(kinds["found"]) >= 20 and len(kinds["clean"]) >= 10 and {c.name for c in kinds["miss"]} == {"cut_fine_k2000", "mp3_320_mono_k2000_s16"}
    assert {c.offset for c in kinds["found"]} >= {ac.grid_after(k) for k in (0, 1, 31, 32, 575, 2000)} and ac.grid_after(0) == 481
    for c in kinds["found"] + kinds["miss"]:
        r, _ = _route(c, 0)
        ref = ac.reference(c.name)
        strongest = max(ref["views"], key=lambda w: w["z"])
        assert not (0.9 * z_min <= strongest["z"] <= 1.1 * z_min) and not (0.9 * iso_min <= strongest["iso"] <= 1.1 * iso_min), c.name
        if c.kind == "miss":
            assert not r.flags & _capi.ANC_MP3_GRID and r.best_view == _capi.ANC_NO_VIEW, c.name
            continue
        assert r.flags & _capi.ANC_MP3_GRID and r.grid_offset == c.offset and r.z >= z_min and r.iso >= iso_min, (c.name, r.grid_offset, r.z, r.iso)
        if c.midside:
            assert r.flags & _capi.ANC_MIDSIDE and r.view[r.best_view].kind in (_capi.ANC_VIEW_MID, _capi.ANC_VIEW_SIDE), c.name
            assert any(r.view[v].flagged and r.view[v].offset == c.offset for v in (2, 3)), c.name
    for c in kinds["clean"]:
        r, _ = _route(c, 0)
        assert not r.flags & (_capi.ANC_MP3_GRID | _capi.ANC_MIDSIDE) and (r.grid_offset, r.z, r.iso) == (0, 0.0, 0.0), c.name
        assert not any(r.view[v].flagged for v in range(r.views)), c.name


def test_the_recorded_thresholds_are_the_headers():
    """tests/golden/ancestry_measured.json holds both sides; the header's defaults are their geometric means, and the sides do
    not overlap."""
    m = MEASURED
    assert m["never_coded_max_z"] < m["coded_min_z"] and m["never_coded_max_iso"] < m["coded_min_iso"]
    z_min, iso_min = ac.thresholds()
    text = (ROOT / "include" / "mp3rgain_amd_ancestry.h").read_text()
    hz = float(re.search(r"#define RG_ANC_Z_MIN\s+([0-9.]+)", text).group(1))
    hi = float(re.search(r"#define RG_ANC_ISO_MIN\s+([0-9.]+)", text).group(1))
    hf = float(re.search(r"#define RG_ANC_ACTIVE_FLOOR\s+([0-9.]+)f", text).group(1))
    assert hz == round(z_min, 2) == m["z_min"] == _capi.ANC_Z_MIN and hi == round(iso_min, 3) == m["iso_min"] == _capi.ANC_ISO_MIN
    assert abs(hf - 1.0 / 216.0) < 1e-8 and hf == _capi.ANC_ACTIVE_FLOOR and abs(m["active_floor"] - 1.0 / 216.0) < 1e-15
    for k in ("7.3931", "48.8816", "1.0559", "2.6564"):
        assert k in text
    assert all(str(v) in text for v in (m["never_coded_max_z"], m["coded_min_z"], m["never_coded_max_iso"], m["coded_min_iso"]))


def test_short_silent_and_nonfinite_records():
    x = ac.to_s16(ac.music(3 * 576, 9))
    r = rg.ancestry_arena(None, 0, [_capi.TrackDesc(0, 3 * 576 - 1, 44100, 1, S16)], x.view(np.uint8))[0][0]
    assert r.flags == _capi.ANC_COMPLETE | _capi.ANC_SHORT | _capi.ANC_SILENT and (r.segments, r.granules, r.views, r.best_view) == (0, 0, 1, _capi.ANC_NO_VIEW)
    r = rg.ancestry_arena(None, 2, [_capi.TrackDesc(0, 0, 44100, 2, S16)], x.view(np.uint8))[0][0]
    assert r.flags == _capi.ANC_COMPLETE | _capi.ANC_SHORT | _capi.ANC_SILENT and r.views == 4
    r, cnt = rg.ancestry_arena(None, 0, [_capi.TrackDesc(0, 3 * 576, 44100, 1, S16)], x.view(np.uint8))
    assert r[0].flags == _capi.ANC_COMPLETE and (r[0].segments, r[0].granules) == (1, 1) and cnt[0, 0, 1].max() == 576
    z = np.zeros(2 * 4 * 576, np.int16)
    z[5] = 1  # one LSB: below the floor everywhere
    r = rg.ancestry_arena(None, 0, [_capi.TrackDesc(0, 4 * 576, 44100, 2, S16)], z.view(np.uint8))[0][0]
    assert r.flags == _capi.ANC_COMPLETE | _capi.ANC_SILENT and r.view[0].active_total == 0 and r.view[0].z == 0.0
    f = (ac.music(2 * 3 * 576, 10) / 32768.0).astype(np.float32)
    f[[3, 3 * 576 + 1, 3 * 576 + 2]] = [np.nan, np.inf, -np.inf]
    for route in (0, 2):
        r = rg.ancestry_arena(None, route, [_capi.TrackDesc(0, 3 * 576, 44100, 2, F32)], f.view(np.uint8))[0][0]
        assert r.flags == _capi.ANC_COMPLETE | _capi.ANC_NONFINITE and [r.view[v].nonfinite for v in range(4)] == [1, 2, 0, 0]
        assert [r.view[v].kind for v in range(4)] == [0, 1, _capi.ANC_VIEW_MID, _capi.ANC_VIEW_SIDE]


def test_the_floor_is_sixteen_times_the_rounding_noise():
    """The mean noise gain of the 576 analysis functionals, recomputed here in float64 from the encoder's own chain: 1/288."""
    import mp3_encoder as E

    rng = np.random.default_rng(3)
    n = 576 * 40
    spec = E.mdct_granules(E.polyphase_analysis(rng.standard_normal(n)), [0] * (n // 576))[2:]
    gain = float((spec * spec).mean())
    assert abs(gain * 288.0 - 1.0) < 0.02
    assert abs(16.0 * (1.0 / 12.0) / 288.0 - ac.ACTIVE_FLOOR) < 1e-15


def test_options_and_refusals():
    arena = np.zeros(64, dtype=np.uint8)
    ok = _capi.TrackDesc(0, 4, 44100, 2, S16)
    for route in (0, 2):
        for desc, opts, code, text in ((_capi.TrackDesc(0, 17, 44100, 2, S16), {}, RG_ERR_INVALID_ARG, "beyond the arena"),
                                       (_capi.TrackDesc(1, 4, 44100, 2, S16), {}, RG_ERR_INVALID_ARG, "sample-aligned"),
                                       (_capi.TrackDesc(2, 4, 44100, 2, S32), {}, RG_ERR_INVALID_ARG, "sample-aligned"),
                                       (_capi.TrackDesc(0, 1, 44100, 9, S16), {}, RG_ERR_FORMAT, "9 channel"),
                                       (_capi.TrackDesc(0, 1, 44100, 0, S16), {}, RG_ERR_FORMAT, "0 channel"),
                                       (_capi.TrackDesc(0, 1, 44100, 1, 7), {}, RG_ERR_FORMAT, "format 7"),
                                       (ok, dict(segments=1, granules=0), RG_ERR_INVALID_ARG, "granules"),
                                       (ok, dict(z_min=-1.0), RG_ERR_INVALID_ARG, "z_min"),
                                       (ok, dict(iso_min=math.inf), RG_ERR_INVALID_ARG, "iso_min"),
                                       (ok, dict(active_floor=math.nan), RG_ERR_INVALID_ARG, "active_floor")):
            with pytest.raises(rg.ReplayGainError) as e:
                rg.ancestry_arena(None, route, [desc], arena, **opts)
            assert e.value.code == code and text in str(e.value), (route, str(e.value))
        assert rg.ancestry_arena(None, route, [], arena)[0] == []
        assert rg.ancestry_arena(None, route, [ok], arena, segments=0, granules=0)[0][0].flags & _capi.ANC_SHORT  # granules is ignored
    L = _capi.load()
    bad = _capi.AncestryOpts(1, 1, 0.0, 0.0, 0.0, 5)
    d = (_capi.TrackDesc * 1)(ok)
    out = (_capi.AncestryRecord * 1)()
    assert L.rg_ancestry_arena(None, 0, 1, d, C.byref(bad), arena.ctypes.data, arena.size, out, None) == RG_ERR_INVALID_ARG
    with pytest.raises(rg.ReplayGainError) as e:
        rg.ancestry_arena(None, 3, [ok], arena)
    assert e.value.code == RG_ERR_INVALID_ARG
    assert L.rg_ancestry_arena(None, 1, 0, None, None, None, 0, None, None) == RG_ERR_INVALID_ARG  # the kernels need a context
    assert C.sizeof(_capi.AncestryRecord) == 872 and C.sizeof(_capi.AncestryView) == 80 and C.sizeof(_capi.AncestryOpts) == 32
    phases, tile, lanes, lds = rg.ancestry_kernel_shape()
    assert (phases, lanes) == (32, 256) and tile >= 1 and lds <= 160 * 1024


def test_records_as_python_objects():
    case = next(c for c in ac.cases() if c.name == "mp3_64_ms_k2000_s16")
    r, _ = _route(case, 0)
    a = rg.ancestry_from_record(r)
    assert a.mp3_grid and a.midside and a.complete and not a.short and not a.silent and a.error is None
    assert a.grid_offset == case.offset and a.views[a.best_view].name in ("mid", "side") and [v.name for v in a.views] == ["ch0", "ch1", "mid", "side"]
    assert a.summary == f"mp3 grid at +{case.offset} (z {a.z:.1f}, x{a.iso:.2f}, mid/side)" and a.verdicts == ["mp3-grid", "mid/side"]
    clean = rg.ancestry_from_record(_route(next(c for c in ac.cases() if c.name == "clean_white"), 0)[0])
    assert clean.summary == "no grid found" and clean.verdicts == ["ok"] and clean.best_view is None
