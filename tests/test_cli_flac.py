"""The command line and FLAC: -R collects .flac files, FLAC is recognised by its bytes, applying gain leaves a FLAC file
untouched with an "analysed only" error, and the printed -r / -a numbers are the library's (GPU)."""
import io
import json
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import flacenc as fe  # noqa: E402

from mp3rgain_amd import cli  # noqa: E402


def run(*args):
    out, err = io.StringIO(), io.StringIO()
    rc = cli.main([str(a) for a in args], out, err)
    return rc, out.getvalue(), err.getvalue()


def _flac(path, seed=0, tag=False):
    data = fe.encode(fe.test_pcm(np.random.default_rng(seed), 2, 44100 * 2, 16), 44100, 16)
    path.write_bytes((fe.id3v2_tag(50) if tag else b"") + data)
    return path


def test_recursive_collects_flac(tmp_path):
    (tmp_path / "d").mkdir()
    a = _flac(tmp_path / "d" / "a.flac")
    b = _flac(tmp_path / "B.FLAC", 1)
    (tmp_path / "d" / "x.txt").write_text("no")
    got = cli.expand_files_recursive([tmp_path])
    assert a in got and b in got and all(p.suffix.lower() != ".txt" for p in got)


def test_flac_recognised_by_bytes(tmp_path):
    assert cli._is_flac(_flac(tmp_path / "a.flac"))
    assert cli._is_flac(_flac(tmp_path / "no_suffix", tag=True))
    (tmp_path / "fake.flac").write_bytes(b"RIFF\0\0\0\0WAVE")
    assert not cli._is_flac(tmp_path / "fake.flac")


@pytest.mark.gpu
def test_apply_gain_leaves_flac_untouched(tmp_path, _ctx):
    f = _flac(tmp_path / "a.flac")
    before = f.read_bytes()
    rc, out, err = run("-r", "-o", "json", f)
    assert f.read_bytes() == before
    doc = json.loads(out)
    entry = doc["files"][0]
    assert entry["status"] == "error" and "FLAC input is analysed only" in entry["error"]


@pytest.mark.gpu
def test_track_and_album_numbers(tmp_path, _ctx, oracle):
    files = [_flac(tmp_path / f"t{i}.flac", i) for i in range(2)]
    hists, per = [], []
    for i in range(2):
        pcm = fe.test_pcm(np.random.default_rng(i), 2, 44100 * 2, 16)
        want, h = oracle.analyze_pcm(pcm[0].astype(np.int16), pcm[1].astype(np.int16), 44100)
        per.append(want)
        hists.append(h)
    alb, _ = oracle.album_from_hists(hists, [w["peak"] for w in per])
    rc, out, _ = run("-o", "json", "-n", "-a", *files)
    d = json.loads(out)
    assert d["album"]["loudness_db"] == alb["album_loudness_db"] and d["album"]["gain_db"] == alb["album_gain_db"]
    assert [r["loudness_db"] for r in d["files"]] == [w["loudness_db"] for w in per]
    rc, out, _ = run("-o", "json", "-n", "-r", *files)
    assert [r["loudness_db"] for r in json.loads(out)["files"]] == [w["loudness_db"] for w in per]
