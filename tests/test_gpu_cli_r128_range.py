"""`python -m mp3rgain_amd --r128 --range` on WAV and FLAC files the test writes (long enough to have short-term blocks): the
text output and the JSON output carry the loudness range and the momentary / short-term maxima the checker
(tests/r128range_ref.py) gives, per file and per album; without --range none of it appears; TSV is what it was."""
import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import flacenc as fe  # noqa: E402
import r128range_cases as cases  # noqa: E402
import r128range_ref as ref  # noqa: E402
from wavutil import wav_bytes  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = Path(__file__).resolve().parent.parent
TOL = 100.0 * cases.load_measured()["worst_relative_st_error"]
KEYS = ("loudness_range_lu", "max_momentary_lufs", "max_short_term_lufs")


def _cli(*args):
    env = dict(os.environ, PYTHONPATH=str(ROOT))
    p = subprocess.run([sys.executable, "-m", "mp3rgain_amd", *[str(a) for a in args]], capture_output=True, text=True, env=env,
                       cwd=ROOT, timeout=600)
    return p.returncode, p.stdout, p.stderr


@pytest.fixture(scope="module")
def album(tmp_path_factory):
    d = tmp_path_factory.mktemp("r128range")
    tr = cases.album_tracks()[:2]  # a float WAV at 48 kHz and a 16-bit FLAC at 44.1 kHz
    files = []
    for i, (ch, rate, container, kind) in enumerate(tr):
        f = d / f"t{i}.{container}"
        f.write_bytes(wav_bytes(ch, rate, kind) if container == "wav" else fe.encode(np.stack([c.astype(np.int64) for c in ch]), rate, 16))
        files.append(f)
    return files, ref.analyze_album([(ch, rate) for ch, rate, _, _ in tr])


def _check(got, want):
    assert abs(got["loudness_range_lu"] - want["loudness_range_lu"]) <= 2 * 4.343 * TOL
    assert abs(got["max_momentary_lufs"] - want["max_momentary_lufs"]) <= 4.343 * TOL
    assert abs(got["max_short_term_lufs"] - want["max_short_term_lufs"]) <= 4.343 * TOL


def test_json_carries_the_range_fields(_ctx, album):
    files, (ref_tracks, ref_album) = album
    rc, out, err = _cli("--r128", "--range", "-r", "-n", "-o", "json", *files)
    assert rc == 0, err
    for f, want in zip(json.loads(out)["files"], ref_tracks):
        print(f["file"], {k: f[k] for k in KEYS})
        _check(f, want)
        assert "loudness_lufs" in f
    rc, out, err = _cli("--r128", "--range", "-a", "-n", "-o", "json", *files)
    assert rc == 0, err
    d = json.loads(out)
    print("album", {k: d["album"][k] for k in KEYS})
    _check(d["album"], ref_album)
    for f, want in zip(d["files"], ref_tracks):
        _check(f, want)
    # without --range: none of the fields, for the files or for the album
    for args in (("-r",), ("-a",)):
        rc, out, err = _cli("--r128", *args, "-n", "-o", "json", *files)
        assert rc == 0, err
        d = json.loads(out)
        assert not any(k in f for f in d["files"] for k in KEYS) and not any(k in d.get("album", {}) for k in KEYS)
        assert all("loudness_lufs" in f for f in d["files"])
    # --range without --r128 is the ReplayGain 1.0 analysis, as --true-peak without it
    rc, out, err = _cli("--range", "-r", "-n", "-o", "json", files[0])
    assert rc == 0, err
    f = json.loads(out)["files"][0]
    assert not any(k in f for k in KEYS) and "loudness_lufs" not in f


def test_text_prints_the_range_lines(_ctx, album):
    files, (ref_tracks, ref_album) = album
    rc, out, err = _cli("--r128", "--range", "-r", "-n", *files)
    assert rc == 0, err
    lines = [line.strip() for line in out.splitlines() if "Loudness range:" in line]
    assert len(lines) == 2
    for line, want in zip(lines, ref_tracks):
        assert line == (f"Loudness range: {want['loudness_range_lu']:.1f} LU, Max momentary: {want['max_momentary_lufs']:.1f} LUFS, "
                        f"Max short-term: {want['max_short_term_lufs']:.1f} LUFS"), line
    rc, out, err = _cli("--r128", "--range", "-a", "-n", *files)
    assert rc == 0, err
    want = (f"  Album Loudness range: {ref_album['loudness_range_lu']:.1f} LU, Max momentary: {ref_album['max_momentary_lufs']:.1f} LUFS, "
            f"Max short-term: {ref_album['max_short_term_lufs']:.1f} LUFS")
    assert want in out.splitlines(), out
    assert sum("Loudness range:" in line for line in out.splitlines()) == 3  # the album's and one per file
    for args in (("-r",), ("-a",)):
        rc, out, err = _cli("--r128", *args, "-n", *files)
        assert rc == 0 and "Loudness range" not in out and "Max momentary" not in out
    # TSV stays as it is
    rc, with_range, _ = _cli("--r128", "--range", "-o", *files)
    rc2, without, _ = _cli("--r128", "-o", *files)
    assert rc == rc2 == 0 and with_range == without and with_range.startswith("File\tMP3 gain\tdB gain")
