"""`--clicks` of the command line (mp3rgain_amd/cli.py) on the GPU: tiny synthetic files through rg_clicks, the readings they were
made for, the numbers against the restatement (tests/clicks_cases.py), the three output forms, exit status 0 and 1 with a missing
file."""
import io
import json
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import clicks_cases as cc  # noqa: E402
import flacenc  # noqa: E402
from wavutil import wav_bytes  # noqa: E402

pytestmark = pytest.mark.gpu


def _run(*args):
    from mp3rgain_amd import cli

    out, err = io.StringIO(), io.StringIO()
    code = cli.main([str(a) for a in args], out, err)
    return code, out.getvalue(), err.getvalue()


def test_clicks_on_files_text_tsv_json(tmp_path):
    rate = 8000
    rng = np.random.default_rng(93)
    a, b = cc.tonal(rng, 6000), cc.tonal(rng, 6000)
    t0, t1 = a.copy(), b.copy()
    t0[2000] += 9000
    t1[4000] -= 9000
    made = {"clean.wav": [a, b], "ticks.wav": [t0, t1], "one.wav": [t0]}
    made = {name: [v.astype(np.int16) for v in chans] for name, chans in made.items()}
    files = []
    for name, chans in made.items():
        (tmp_path / name).write_bytes(wav_bytes(chans, rate, "s16"))
        files.append(tmp_path / name)
    pcm = np.stack([t0[:5000], b[:5000]]).astype(np.int64)
    flac = tmp_path / "b.flac"
    flac.write_bytes(flacenc.encode(pcm, 44100, 16, flacenc.Options(block_size=1152)))
    want = {name: cc.want_track(cc.Tr(name, chans, rate), cc.Opts()) for name, chans in made.items()}
    wf = cc.want_track(cc.Tr("b", [pcm[c].astype(np.int16) for c in range(2)], 44100), cc.Opts())
    w = want["ticks.wav"]
    assert [c["clicks"] for c in w["ch"]] == [1, 1] and w["listed"] == 2 and want["clean.wav"]["events"] == 0
    code, out, err = _run("--clicks", *files, flac)
    lines = out.splitlines()
    assert code == 0 and err == "" and lines[0].startswith("mp3rgain click scan of 4 file(s)")
    assert lines[2] == "no clicks  clean.wav"
    assert lines[3].startswith("2 clicks (first at 0:00.250 left, strongest x") and lines[3].endswith("  ticks.wav")
    e0, e1 = w["list"]
    assert lines[4] == f"    click at 0:00.250 left, {e0['width']} samples, x{e0['strength_permille'] / 1000.0:.1f}"
    assert lines[5] == f"    click at 0:00.500 right, {e1['width']} samples, x{e1['strength_permille'] / 1000.0:.1f}"
    assert lines[6].startswith("1 click (first at 0:00.250, strongest x") and lines[6].endswith("  one.wav")
    assert lines[8].startswith("1 click (first at 0:00.045 left, ") and lines[8].endswith("  b.flac") and len(lines) == 10
    code, out, _ = _run("--clicks", "-o", "tsv", "--click-list", "1", "--click-ratio", "20", "--click-order", "4", "--click-block", "512", tmp_path / "ticks.wav")
    rows = [line.split("\t") for line in out.splitlines()]
    near = cc.want_track(cc.Tr("ticks", made["ticks.wav"], rate), cc.Opts(block_samples=512, order=4, ratio_permille=20000, max_events=1))
    assert code == 0 and len(rows) == 2 and rows[0][:3] == ["ticks.wav", str(sum(c["clicks"] for c in near["ch"])), str(sum(c["bursts"] for c in near["ch"]))]
    assert rows[0][9:11] == [str(near["events"]), "1"] and rows[0][14] == "20.000"
    assert rows[1] == ["ticks.wav", "click", str(near["list"][0]["start"]), str(near["list"][0]["width"]), "0", str(near["list"][0]["peak_at"]),
                       f"{near['list'][0]['strength_permille'] / 1000.0:.3f}"]
    code, out, _ = _run("--clicks", "-o", "json", tmp_path / "ticks.wav", tmp_path / "missing.wav", flac)
    d = json.loads(out)
    assert code == 1 and d["summary"] == {"total_files": 3, "successful": 2, "failed": 1}
    assert d["files"][1]["status"] == "error" and "Failed to open" in d["files"][1]["error"]
    for got, ww in ((d["files"][0], w), (d["files"][2], wf)):
        for f in cc.RECORD_FIELDS:
            if f not in ("status", "events"):
                assert got[f] == ww[f], f
        assert got["events_total"] == ww["events"]
        assert [{f: c[f] for f in cc.CHANNEL_FIELDS} for c in got["channel_records"]] == ww["ch"]
        kinds = {"click": 1, "burst": 2}
        assert [dict({f: e[f] for f in cc.EVENT_FIELDS if f != "kind"}, kind=kinds[e["kind"]]) for e in got["events"]] == ww["list"]
    assert d["files"][0]["clicks"] == 2 and d["files"][2]["block_samples"] == 1024
