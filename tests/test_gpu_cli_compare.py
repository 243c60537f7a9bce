"""`python -m mp3rgain_amd --compare` end to end on the GPU: three generated WAV files of a few seconds -- a reference, the same
samples behind 588 frames of silence, a -3 dB re-dithered copy -- through the fingerprint hint in text and through a given hint in
JSON, and a missing file."""
import io
import json
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
from wavutil import wav_bytes  # noqa: E402

from mp3rgain_amd import cli  # noqa: E402

pytestmark = pytest.mark.gpu

N, RATE = 150000, 44100


def _run(*args):
    out, err = io.StringIO(), io.StringIO()
    code = cli.main([str(a) for a in args], out, err)
    return code, out.getvalue(), err.getvalue()


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("cli_compare")
    rng = np.random.default_rng(17)
    x = []
    for _ in range(2):
        v = np.cumsum(rng.standard_normal(N + 64))
        v = v[64:] - np.convolve(v, np.ones(64) / 64.0, "valid")[:N]
        x.append(np.rint(v / np.abs(v).max() * 20000.0).astype(np.int16))
    made = {"ref": x, "late": [np.concatenate([np.zeros(588, np.int16), c]) for c in x],
            "gain": [np.rint(c * 10 ** (-3.0 / 20) + rng.triangular(-1, 0, 1, size=N)).astype(np.int16) for c in x]}
    for name, chans in made.items():
        (tmp / f"{name}.wav").write_bytes(wav_bytes(chans, RATE, "s16"))
    return tmp


def test_compare_in_text_and_json(files):
    code, out, err = _run("--compare", files / "ref.wav", files / "late.wav", files / "gain.wav")
    assert code == 0 and err == "", err
    lines = out.strip().split("\n")
    assert lines[0].startswith("mp3rgain null test of 2 file(s) against ref.wav")
    assert lines[2] == "identical samples, starts 588 samples later  late.wav"
    assert lines[3].startswith("same master  (gain +3.00 dB, residual 0.") and lines[3].endswith("  gain.wav")
    code, out, err = _run("--compare", "--compare-hint", "600", "--compare-radius", "64", "-o", "json", files / "ref.wav", files / "late.wav", files / "missing.wav")
    doc = json.loads(out)
    assert code == 1 and [f["status"] for f in doc["files"]] == ["success", "error"] and "missing.wav" in doc["files"][1]["error"]
    r = doc["files"][0]
    assert (r["lag"], r["hint"], r["radius"], r["b_head"], r["overlap"], r["first_diff"], r["null_db"]) == (588, 600, 64, 588, N, None, None)
    assert r["verdicts"] == ["identical", "shifted", "lengths differ"] and r["reading"] == "identical samples, starts 588 samples later" and r["complete"]
    code, out, _ = _run("--compare", "-o", "tsv", files / "gain.wav", files / "ref.wav")
    row = out.strip().split("\t")
    assert code == 0 and row[:4] == ["ref.wav", "same master", "0", "1"] and abs(float(row[5]) + 3.0) < 0.01
