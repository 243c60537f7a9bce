"""`python -m mp3rgain_amd --r128 -o` on a golden MP3 and a golden FLAC prints the gain the checker (tests/r128ref.py) gives
for the PCM of the library's own host decoders; JSON carries loudness_lufs; without --r128 the ReplayGain 1.0 line is printed."""
import json
import math
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import r128ref  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
MP3 = ROOT / "tests" / "golden" / "mp3" / "dense_44k_joint_128.mp3"
FLAC = ROOT / "tests" / "golden" / "flac" / "s16_mono_8k.flac"
TOL = 100.0 * json.loads((ROOT / "tests" / "golden" / "r128_measured.json").read_text())["worst_relative_block_error"]


def _cli(*args):
    env = dict(os.environ, PYTHONPATH=str(ROOT))
    p = subprocess.run([sys.executable, "-m", "mp3rgain_amd", *[str(a) for a in args]], capture_output=True, text=True, env=env,
                       cwd=ROOT, timeout=600)
    return p.returncode, p.stdout, p.stderr


def _refs():
    from mp3rgain_amd import flacdec, mp3dec

    pcm, info = mp3dec.decode(MP3.read_bytes())
    a = r128ref.analyze([pcm[c] for c in range(int(info.channels))], int(info.sample_rate), True)
    rate, bps, fp, _ = flacdec.decode(FLAC.read_bytes())
    assert bps == 16
    b = r128ref.analyze([c.astype(np.int16) for c in fp], rate, True)
    return a, b


def test_tsv_gain_is_the_checkers(_ctx):
    a, b = _refs()
    rc, out, err = _cli("--r128", "-o", MP3, FLAC)
    assert rc == 0, err
    lines = out.splitlines()
    assert lines[0] == "File\tMP3 gain\tdB gain\tMax Amplitude\tMax global_gain\tMin global_gain"
    for line, ref, f in zip(lines[1:], (a, b), (MP3, FLAC)):
        cols = line.split("\t")
        print(line, "| checker gain", ref["gain_db"], "peak", ref["sample_peak"])
        assert cols[0] == f.name
        assert abs(float(cols[2]) - ref["gain_db"]) <= 4.343 * TOL + 1e-12 + 5e-7  # printed with six decimals
        assert int(cols[1]) == round(float(cols[2]) / 1.5)
        assert abs(float(cols[3]) - ref["sample_peak"] * 32768.0) <= 5e-7 * 32768.0
    rc, out, _ = _cli("--r128", "--true-peak", "-o", MP3)
    assert rc == 0
    assert abs(float(out.splitlines()[1].split("\t")[3]) / 32768.0 - a["true_peak"]) <= 2e-6 * a["true_peak"] + 5e-7
    # without the switch: the ReplayGain 1.0 analysis, another gain
    rc, out1, _ = _cli("-o", MP3)
    assert rc == 0 and abs(float(out1.splitlines()[1].split("\t")[2]) - a["gain_db"]) > 1e-3


def test_json_and_album(_ctx):
    a, b = _refs()
    rc, out, err = _cli("--r128", "-r", "-n", "-o", "json", MP3)
    assert rc == 0, err
    f = json.loads(out)["files"][0]
    assert abs(f["loudness_lufs"] - a["loudness_lufs"]) <= 4.343 * TOL + 1e-12 and f["loudness_db"] == f["loudness_lufs"]
    assert f["peak"] == a["sample_peak"]
    rc, out, err = _cli("--r128", "-a", "-n", "-o", "json", MP3, FLAC)
    assert rc == 0, err
    d = json.loads(out)
    pcm_tracks = _album_inputs()
    _, ref_album = r128ref.analyze_album(pcm_tracks)
    assert abs(d["album"]["loudness_lufs"] - ref_album["loudness_lufs"]) <= 4.343 * TOL + 1e-12
    assert abs(d["album"]["gain_db"] - (-18.0 - d["album"]["loudness_lufs"])) <= 1e-12
    assert d["album"]["peak"] == ref_album["sample_peak"]
    rc, out, _ = _cli("-r", "-n", "-o", "json", MP3)
    assert rc == 0 and "loudness_lufs" not in json.loads(out)["files"][0]
    rc, out, _ = _cli("--r128", "-r", "-n", MP3)
    assert rc == 0 and "Target: -18 LUFS (ReplayGain 2.0, EBU R 128)" in out


def _album_inputs():
    from mp3rgain_amd import flacdec, mp3dec

    pcm, info = mp3dec.decode(MP3.read_bytes())
    rate, _, fp, _ = flacdec.decode(FLAC.read_bytes())
    return [([pcm[c] for c in range(int(info.channels))], int(info.sample_rate)), ([c.astype(np.int16) for c in fp], rate)]
