"""`--stereo` of the command line (mp3rgain_amd/cli.py) on the GPU: synthetic files through rg_stereo, the verdicts they were
made for, the numbers against the restatement (tests/stereo_cases.py), the three output forms, exit status 0 and 1 with a missing
file."""
import io
import json
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import flacenc  # noqa: E402
import stereo_cases as sc  # noqa: E402
from wavutil import wav_bytes  # noqa: E402

pytestmark = pytest.mark.gpu


def _run(*args):
    from mp3rgain_amd import cli

    out, err = io.StringIO(), io.StringIO()
    code = cli.main([str(a) for a in args], out, err)
    return code, out.getvalue(), err.getvalue()


def test_stereo_on_files_text_tsv_json(tmp_path):
    rate = 8000
    rng = np.random.default_rng(93)
    a = rng.integers(-12000, 12000, size=6000).astype(np.int16)
    b = rng.integers(-12000, 12000, size=6000).astype(np.int16)
    made = {"wide.wav": [(a + b // 2).astype(np.int16), (a - b // 2).astype(np.int16)], "dual.wav": [a, a.copy()], "flipped.wav": [a, (-a).astype(np.int16)],
            "late.wav": [a, sc.delayed(a, 3)], "one.wav": [a]}
    files = []
    for name, chans in made.items():
        (tmp_path / name).write_bytes(wav_bytes(chans, rate, "s16"))
        files.append(tmp_path / name)
    pcm = flacenc.test_pcm(rng, 2, 5000, 16)
    flac = tmp_path / "b.flac"
    flac.write_bytes(flacenc.encode(pcm, 44100, 16, flacenc.Options(block_size=1152)))
    want = {name: sc.want_track(sc.Tr(name, chans, rate)) for name, chans in made.items()}
    wf = sc.want_track(sc.Tr("b", [pcm[c].astype(np.int16) for c in range(2)], 44100))
    code, out, err = _run("--stereo", *files, flac)
    lines = out.splitlines()
    w, late = want["wide.wav"], want["late.wav"]
    assert code == 0 and err == "" and lines[0].startswith("mp3rgain stereo image of 6 file(s)")
    assert lines[2] == f"stereo  (correlation {w['correlation']:.2f}, side {w['side_db']:+.1f} dB, balance {w['balance_db']:+.1f} dB)  wide.wav"
    assert lines[3] == "dual mono  dual.wav" and lines[4] == "right channel is the inverted left  flipped.wav  [out of phase]"
    assert lines[5] == f"right channel late by 3 samples (correlation {late['lag_correlation']:.3f} there, {late['correlation']:.2f} in place)  late.wav"
    assert lines[6] == "mono file  one.wav" and lines[7].endswith("  b.flac")
    code, out, _ = _run("--stereo", "-o", "tsv", "--stereo-radius", "2", tmp_path / "late.wav")
    rows = [line.split("\t") for line in out.splitlines()]
    near = sc.want_track(sc.Tr("late", made["late.wav"], rate), 2)
    assert code == 0 and len(rows) == 1 and rows[0][:2] == ["late.wav", "stereo"] and rows[0][5] == str(near["lag"]) and rows[0][12] == "2"
    code, out, _ = _run("--stereo", "-o", "json", tmp_path / "late.wav", tmp_path / "missing.wav", flac)
    d = json.loads(out)
    assert code == 1 and d["summary"] == {"total_files": 3, "successful": 2, "failed": 1}
    assert d["files"][1]["status"] == "error" and "Failed to open" in d["files"][1]["error"]
    for got, w in ((d["files"][0], late), (d["files"][2], wf)):
        for f in sc.EXACT_FIELDS:
            if f != "status":
                assert got[f] == w[f], f
        for f in sc.FINISH_FIELDS:
            assert abs(got[f] - w[f]) <= sc.FINISH_RTOL * abs(w[f]), f
    assert d["files"][0]["verdicts"] == ["delayed"] and d["files"][2]["block_frames"] == 44100
