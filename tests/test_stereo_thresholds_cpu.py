"""The two measured thresholds of the stereo scan (include/mp3rgain_amd_stereo.h: delay_permille, phase_permille) against their
record (tests/golden/stereo_measured.json, written by tools/stereo_refcheck.py --record): the two classes of each do not overlap,
the shipped defaults are the geometric means and lie between them, every delayed copy read its delay, and a small subset of the
tool's cases re-run here on the serial host twin stays inside the recorded bounds.  No GPU."""
import importlib.util
import json
import math
import re
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))

from mp3rgain_amd import _capi  # noqa: E402

MEASURED = json.loads((ROOT / "tests" / "golden" / "stereo_measured.json").read_text())


def _tool():
    spec = importlib.util.spec_from_file_location("stereo_refcheck", ROOT / "tools" / "stereo_refcheck.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_the_classes_do_not_overlap_and_the_defaults_lie_between_them():
    m = MEASURED
    assert m["not_found"] == [] and m["delayed_misread"] == []
    assert 0.0 < m["never_delayed_max"] < m["delay_permille"] / 1000.0 < m["delayed_min"] <= 1.0
    assert 0.0 < m["never_inverted_max"] < m["phase_permille"] / 1000.0 < m["inverted_min"] <= 1.0
    assert m["delay_permille"] == round(1000.0 * math.sqrt(m["never_delayed_max"] * m["delayed_min"]))
    assert m["phase_permille"] == round(1000.0 * math.sqrt(m["never_inverted_max"] * m["inverted_min"]))
    assert (_capi.ST_DEFAULT_DELAY_PERMILLE, _capi.ST_DEFAULT_PHASE_PERMILLE) == (m["delay_permille"], m["phase_permille"])
    hdr = (ROOT / "include" / "mp3rgain_amd_stereo.h").read_text()
    assert int(re.search(r"#define RG_ST_DEFAULT_DELAY_PERMILLE (\d+)u", hdr).group(1)) == m["delay_permille"]
    assert int(re.search(r"#define RG_ST_DEFAULT_PHASE_PERMILLE (\d+)u", hdr).group(1)) == m["phase_permille"]


def test_the_record_holds_every_case_the_header_names():
    m = MEASURED
    assert m["radius"] == 64 and len(m["cases"]["never"]) >= 13
    forms = ("s16", "f32", "dithered", "mp3_128", "mp3_320")
    assert set(m["cases"]["inverted"]) == set(forms)
    assert set(m["cases"]["delayed"]) == {f"d{d}_{form}" for d in (1, -1, 2, -2, 17, -17, 64, -64) for form in forms}
    for name, f in m["cases"]["delayed"].items():
        assert f["lag"] == f["d"] and f["beats_zero"] and f["lag_correlation"] >= m["delayed_min"], name
    # what keeps a panned tone unflagged is that nothing beats lag 0, not the threshold
    tones = [f for k, f in m["cases"]["never"].items() if k.startswith("panned_tone")]
    assert len(tones) == 4 and all(f["lag"] == 0 and not f["beats_zero"] and f["off_zero_max"] > 0.99 for f in tones)
    assert m["never_delayed_off_zero_max"] > m["delay_permille"] / 1000.0


def test_a_subset_re_run_on_the_host_twin_stays_inside_the_recorded_bounds():
    tool = _tool()
    m = MEASURED
    n = 30000
    rng = np.random.default_rng(0x57E1)
    x = tool.music(n, 7)
    lo_delay, hi_phase = m["delay_permille"] / 1000.0, m["phase_permille"] / 1000.0
    for d in (1, -2, 17, -64):
        for form, chans in tool.treatments(x, tool.delayed(x, d), rng, mp3=False).items():
            f = tool.figures(chans)
            assert f["lag"] == d and f["beats_zero"] and f["lag_correlation"] >= m["delayed_min"] > lo_delay, (d, form, f)
    for form, chans in tool.treatments(x, -x, rng, mp3=False).items():
        f = tool.figures(chans)
        assert -f["correlation"] >= m["inverted_min"] - 1e-6 and (not f["beats_zero"] or f["lag_correlation"] < lo_delay), (form, f)
    a, b = tool.music(n, 21), tool.music(n, 22)
    for g in (0.5, math.sqrt(2.0)):
        f = tool.figures([tool.to_s16(0.4 * (a + g * b)), tool.to_s16(0.4 * (a - g * b))])
        assert -f["correlation"] < hi_phase and (not f["beats_zero"] or f["lag_correlation"] < lo_delay), (g, f)
    t = np.arange(n) / tool.RATE
    tone = 20000.0 * np.sin(2 * np.pi * 997.0 * t)
    f = tool.figures([tool.to_s16(tone), tool.to_s16(0.3 * tone)])
    assert f["lag"] == 0 and not f["beats_zero"]
