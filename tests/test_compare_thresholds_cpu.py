"""The two measured thresholds of the null test (include/mp3rgain_amd_compare.h: lock_permille, requant_millilsb2) against their
record (tests/golden/compare_measured.json, written by tools/compare_refcheck.py --record): the two classes of each do not
overlap, the shipped defaults are the geometric means and lie between them, every same-recording pair read its lag, and a reduced
re-run of the tool's material (a quarter of the length, no MP3 encode) on the serial host twin stays inside the recorded sides.
No GPU."""
import importlib.util
import json
import math
import re
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))

from mp3rgain_amd import _capi  # noqa: E402

MEASURED = json.loads((ROOT / "tests" / "golden" / "compare_measured.json").read_text())


def _tool():
    spec = importlib.util.spec_from_file_location("compare_refcheck", ROOT / "tools" / "compare_refcheck.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_the_classes_do_not_overlap_and_the_defaults_are_the_geometric_means():
    m = MEASURED
    assert m["not_found"] == [] and m["same_misread"] == []
    assert 0.0 < m["unrelated_max"] < m["lock_permille"] / 1000.0 < m["same_min"] <= 1.0
    assert 0.0 < m["master_max"] < m["requant_millilsb2"] / 1000.0 < m["other_min"]
    assert m["lock_permille"] == round(1000.0 * math.sqrt(m["unrelated_max"] * m["same_min"]))
    assert m["requant_millilsb2"] == round(1000.0 * math.sqrt(m["master_max"] * m["other_min"]))
    assert (_capi.CMP_DEFAULT_LOCK_PERMILLE, _capi.CMP_DEFAULT_REQUANT_MILLILSB2) == (m["lock_permille"], m["requant_millilsb2"])
    hdr = (ROOT / "include" / "mp3rgain_amd_compare.h").read_text()
    assert int(re.search(r"#define RG_CMP_DEFAULT_LOCK_PERMILLE (\d+)u", hdr).group(1)) == m["lock_permille"]
    assert int(re.search(r"#define RG_CMP_DEFAULT_REQUANT_MILLILSB2 (\d+)u", hdr).group(1)) == m["requant_millilsb2"]


def test_the_record_holds_every_case_the_header_names():
    c = MEASURED["cases"]
    assert len(c["unrelated"]) >= 9 and sum(k.startswith("synth_") for k in c["unrelated"]) == 6
    assert set(c["same"]) == {f"offset{d}" for d in (1, -1, 17, -17, 588, -588, 1023, -1023)} | {"f32_copy", "s24_copy", "gain-6", "inverted"}
    assert set(c["master"]) == {f"gain{db}_{how}" for db in ("-6", "-3", "+1") for how in ("rounded", "dithered")} | {"s24_truncated", "s24_dithered", "f32_to_s16"}
    assert set(c["other"]) == {"remaster", "mp3_64", "mp3_128", "mp3_320"}
    for d in (1, -1, 17, -17, 588, -588, 1023, -1023):
        assert c["same"][f"offset{d}"]["lag"] == d and c["same"][f"offset{d}"]["identical"]
    assert c["same"]["inverted"]["polarity"] == -1 and abs(c["same"]["gain-6"]["gain_db"] - 6.0) < 0.01
    assert all(f["lag"] == MEASURED["mp3_delay"] for k, f in c["other"].items() if k.startswith("mp3"))
    # the 320 kb/s stream is the near side of the residual threshold, and the coders order as their bitrates do
    assert c["other"]["mp3_320"]["residual_lsb2"] == MEASURED["other_min"] < c["other"]["mp3_128"]["residual_lsb2"] < c["other"]["mp3_64"]["residual_lsb2"]
    assert all(f["lock"] >= MEASURED["same_min"] for kind in ("same", "other", "master") for f in c[kind].values())


def test_a_reduced_re_run_on_the_host_twin_stays_inside_the_recorded_sides():
    tool = _tool()
    m = tool.measure(mp3=False, frames=tool.FRAMES // 4)
    lock, requant = MEASURED["lock_permille"] / 1000.0, MEASURED["requant_millilsb2"] / 1000.0
    assert m["same_misread"] == []
    for kind in ("same", "master", "other"):
        for name, f in m["cases"][kind].items():
            assert f["lock"] > lock, (kind, name, f)
    for name, f in m["cases"]["master"].items():
        assert f["residual_lsb2"] < requant and f["residual_lsb2"] <= 1.05 * MEASURED["master_max"], (name, f)
    assert m["cases"]["other"]["remaster"]["residual_lsb2"] > requant
    # unrelated material of the reduced length: below the threshold (a shorter file correlates by chance a little more)
    for s, t in ((7, 8), (21, 22)):
        f = tool.figures(tool.to_s16(tool.music(tool.FRAMES // 4, s)), tool.to_s16(tool.music(tool.FRAMES // 4, t)))
        assert f["lock"] < lock, (s, t, f)
