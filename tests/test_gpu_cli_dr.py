"""`--dr` of the command line (mp3rgain_amd/cli.py) on the GPU: files through rg_dynamic_range, the numbers against the
restatement (tests/dr_cases.py), the three output forms, the album line, exit status 0 and 1 with a missing file."""
import io
import json
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import dr_cases as dc  # noqa: E402
import flacenc  # noqa: E402
from wavutil import wav_bytes  # noqa: E402

pytestmark = pytest.mark.gpu


def _run(*args):
    from mp3rgain_amd import cli

    out, err = io.StringIO(), io.StringIO()
    code = cli.main([str(a) for a in args], out, err)
    return code, out.getvalue(), err.getvalue()


def test_dr_on_files_text_tsv_json(tmp_path):
    rate = 8000  # 3-second blocks of 24 000 frames: 7 blocks in 20 s
    t = np.arange(20 * rate)
    env = np.where((t // (3 * rate)) % 2 == 0, 1.0, 0.25)
    left = np.rint(30000.0 * env * np.sin(2.0 * np.pi * 441.0 * t / rate)).astype(np.int16)
    right = np.rint(30000.0 * np.sin(2.0 * np.pi * 441.0 * t / rate)).astype(np.int16)
    wav = tmp_path / "a.wav"
    wav.write_bytes(wav_bytes([left, right], rate, "s16"))
    rng = np.random.default_rng(91)
    quiet = flacenc.test_pcm(rng, 2, 5000, 16) >> 2
    flac = tmp_path / "b.flac"
    flac.write_bytes(flacenc.encode(quiet << 8, 44100, 24, flacenc.Options(block_size=1152)))
    w = dc.want_track(dc.Tr("a", [left, right], rate))
    wq = dc.want_track(dc.Tr("b", [(quiet[c].astype(np.int64) << 16).astype(np.int32) for c in range(2)], 44100))
    album = int(round((w["dr"] + wq["dr"]) / 2))
    code, out, err = _run("--dr", wav, flac)
    lines = out.splitlines()
    assert code == 0 and err == "" and lines[0].startswith("mp3rgain dynamic range of 2 file(s)")
    assert lines[2] == f"DR{w['dr']:<3d} {w['peak_db']:8.2f} dB peak {w['rms_db']:8.2f} dB RMS   a.wav"
    assert lines[3] == f"    ch 0: DR {w['ch'][0]['dr']:.2f}  peak {w['ch'][0]['peak_db']:.2f} dB  RMS {w['ch'][0]['rms_db']:.2f} dB  blocks 1 of 7"
    assert lines[5].startswith(f"DR{wq['dr']:<3d} ") and lines[5].endswith("b.flac  [short]") and lines[-1] == f"album DR{album}"
    code, out, _ = _run("--dr", "-o", "tsv", "--dr-top", "1000", wav)
    rows = [line.split("\t") for line in out.splitlines()]
    w1000 = dc.want_track(dc.Tr("a", [left, right], rate), None, 1000)
    assert code == 0 and len(rows) == 3 and rows[0][:4] == ["a.wav", "ok", str(w1000["dr"]), f"{w1000['dr_mean']:.2f}"] and rows[1][8:10] == ["7", "7"]
    code, out, _ = _run("--dr", "-o", "json", wav, tmp_path / "missing.wav", flac)
    d = json.loads(out)
    assert code == 1 and d["summary"] == {"total_files": 3, "successful": 2, "failed": 1} and d["album_dr"] == album
    assert d["files"][1]["status"] == "error" and "Failed to open" in d["files"][1]["error"]
    for k, c in enumerate(d["files"][0]["channels"]):
        for f in dc.RAW_FIELDS:
            assert c[f] == w["ch"][k][f], (k, f)
    assert d["files"][0]["dr"] == w["dr"] and abs(d["files"][0]["dr_mean"] - w["dr_mean"]) <= 1e-12 * abs(w["dr_mean"])
    assert d["files"][2]["verdicts"] == ["short"] and d["files"][2]["block_frames"] == 132300
