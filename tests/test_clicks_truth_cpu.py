"""The click scan against planted truth, on the serial host twin (rg_clicks_arena route 0), no GPU: a 3 s mix of tones over a noise
floor of 2^-13 of full scale with single-sample impulses of 1/4 of full scale at ten stated places per channel, two of them in
the same frame of both channels.  At the header's defaults (only the list is made long enough for all twenty events) every
planted impulse is a listed click that starts within order + 1 samples of its place, there are ten clicks per channel and nothing
else, and the copy without the impulses reads no clicks.  The default ratio itself is held to what tools/clicks_refcheck.py
recorded in tests/golden/clicks_measured.json: strictly between the largest undamaged click strength and the smallest strength of
the defect classes the header claims."""
import json
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))

import mp3rgain_amd as rg  # noqa: E402
from mp3rgain_amd import _capi  # noqa: E402

RATE, N = 44100, 3 * 44100
LEFT = (5000, 17321, 29888, 41003, 55555, 66000, 78901, 90123, 104729, 120011)
RIGHT = (7001, 17321, 31000, 44444, 55555, 69001, 80808, 93939, 108000, 125000)  # 17321 and 55555: the same frame in both channels


def _mix(seed):
    rng = np.random.default_rng(seed)
    t = np.arange(N) / RATE
    return 7000.0 * np.sin(2 * np.pi * 220.0 * t) + 4000.0 * np.sin(2 * np.pi * 1318.5 * t + 0.3) + 2000.0 * np.sin(2 * np.pi * 3520.0 * t + 1.1) + \
        4.0 * rng.standard_normal(N)  # 4 LSB: 2^-13 of full scale


def _scan(chans, **kw):
    arena, descs = rg.replaygain.pack_tracks([rg.PcmTrack([np.clip(np.rint(c), -32768, 32767).astype(np.int16) for c in chans], RATE)])
    recs, rows = rg.clicks_arena(None, 0, list(descs)[:1], arena, max_events=32, **kw)
    return rg.clicks_from_record(recs[0], rows)


def test_planted_impulses_are_clicks_and_the_clean_copy_has_none():
    clean = [_mix(101), _mix(102)]
    planted = [c.copy() for c in clean]
    for c, places in enumerate((LEFT, RIGHT)):
        for k, p in enumerate(places):
            planted[c][p] += 8192.0 * (1 if k % 2 == 0 else -1)
    r = _scan(planted)
    P = r.order
    assert (r.ratio_permille, r.block_samples, P, r.gap, r.max_width) == (_capi.CK_DEFAULT_RATIO_PERMILLE, 1024, 8, 16, 32)
    print("planted strengths", sorted(e.strength_permille for e in r.events), "listed", r.listed)
    assert [c.clicks for c in r.ch] == [10, 10] and [c.bursts for c in r.ch] == [0, 0] and r.listed == 20 and not r.truncated
    for c, places in enumerate((LEFT, RIGHT)):
        for p in places:
            near = [e for e in r.events if e.channel == c and e.kind == "click" and abs(e.start - p) <= P + 1]
            assert len(near) == 1, (c, p)
    same = [e for e in r.events if e.start in (17321, 55555)]
    assert [(e.start, e.channel) for e in same] == [(17321, 0), (17321, 1), (55555, 0), (55555, 1)]
    c = _scan(clean)
    print("clean medians", [ch.median_max for ch in c.ch], "strongest clean sample at the probe ratio",
          max(ch.strongest_permille for ch in _scan(clean, ratio_permille=4000).ch))
    assert c.clicks == 0 and c.bursts == 0 and c.events == [] and not c.flags & (_capi.CK_CLICKS | _capi.CK_BURSTS)


def test_the_default_lies_between_the_recorded_sides():
    m = json.loads((ROOT / "tests" / "golden" / "clicks_measured.json").read_text())
    assert m["ratio_permille"] == _capi.CK_DEFAULT_RATIO_PERMILLE
    clean = {k: v for k, v in m["undamaged_max_by_kind"].items() if k not in m["not_clean_kinds"]}
    assert m["claimed"] and m["not_clean_kinds"] == ["drums"] and m["undamaged_max"] == max(clean.values())
    # the undamaged figure of a kind is its strongest click at ANY ratio of the ladder, never below its reading at the probe ratio
    for f in m["cases"]["undamaged"].values():
        assert f["strongest_click"] >= f["at_probe"]["strongest_click"] and f["highest_ratio_with_a_click"] <= f["strongest_click"]
    # at the recorded default the kinds counted clean read no clicks, the kind that is not is a false positive with its numbers ...
    for name, f in m["at_default"].items():
        assert (f["clicks"] == 0) == (f["kind"] not in m["not_clean_kinds"]), name
    assert set(m["false_positives_at_default"]) == {"drums"} and "47 clicks and 21 bursts" in (ROOT / "include" / "mp3rgain_amd_clicks.h").read_text()
    assert m["false_positives_at_default"]["drums"]["clicks"] == 47 and m["false_positives_at_default"]["drums"]["bursts"] == 21
    # ... and every planted defect of every claimed class is found
    assert set(m["claimed_at_default"]) == set(m["claimed"]) and all(f["found"] == f["planted"] == 10 for f in m["claimed_at_default"].values())
    assert all(m["cases"]["damaged"][name]["smallest"] >= m["margin"] * m["undamaged_max"] for name in m["claimed"])
    assert m["claimed_min"] == min(m["cases"]["damaged"][name]["smallest"] for name in m["claimed"])
    assert all(m["cases"]["damaged"][name]["found"] == m["cases"]["damaged"][name]["planted"] for name in m["claimed"])
    assert m["undamaged_max"] < m["ratio_permille"] < m["claimed_min"]
    header = (ROOT / "include" / "mp3rgain_amd_clicks.h").read_text()
    assert f"#define RG_CK_DEFAULT_RATIO_PERMILLE {m['ratio_permille']}u" in header and f"ratio_permille {m['ratio_permille']}" in header
    assert "SYNTHETIC MATERIAL ONLY" in header and "Not found" in header and "FALSE POSITIVES" in header
