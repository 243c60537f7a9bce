"""`--duplicates --dup-any-rate` of the command line (mp3rgain_amd/cli.py) on the GPU: one piece rendered at three rates as WAV and
FLAC and an unrelated one through rg_same_recording_xrate: one group, each member with its own sample rate, the closing line,
the three output forms; without --dup-any-rate the same files form no group."""
import io
import json
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import flacenc  # noqa: E402
import resample_cases as rc  # noqa: E402
from wavutil import wav_bytes  # noqa: E402

pytestmark = pytest.mark.gpu


def _run(*args):
    from mp3rgain_amd import cli

    out, err = io.StringIO(), io.StringIO()
    code = cli.main([str(a) for a in args], out, err)
    return code, out.getvalue(), err.getvalue()


def test_duplicates_across_rates_text_tsv_json(tmp_path):
    files = []
    for name, rate, seed in (("cd.wav", 44100, 1), ("dl48.flac", 48000, 1), ("dl96.wav", 96000, 1), ("other.wav", 44100, 2)):
        x = rc.piece(rate, 5.0, seed=seed)
        p = tmp_path / name
        p.write_bytes(flacenc.encode(np.stack([x]).astype(np.int64), rate, 16, flacenc.Options(block_size=4096)) if name.endswith(".flac")
                      else wav_bytes([x], rate, "s16"))
        files.append(p)
    code, out, err = _run("--duplicates", "--dup-any-rate", *files)
    lines = out.splitlines()
    assert code == 0 and err == "" and lines[-1] == "4 files, 1 groups of duplicates"
    assert "group 1: 3 files" in lines
    k = lines.index("group 1: 3 files")
    assert lines[k + 1].split() == ["cd.wav", "44100", "Hz"]
    assert lines[k + 2].split()[:5] == ["dl48.flac", "48000", "Hz", "+0.000", "s"] and lines[k + 3].split()[:5] == ["dl96.wav", "96000", "Hz", "+0.000", "s"]
    code, out, _ = _run("--duplicates", *files)  # without the option nothing changes: no pair of these can be compared and match
    assert code == 0 and out.splitlines()[-1] == "4 files, 0 groups of duplicates" and " Hz" not in out
    code, out, _ = _run("--duplicates", "--dup-any-rate", "--dup-radius", "2.0", "--dup-ber", "250", "-o", "tsv", *files)
    rows = [line.split("\t") for line in out.splitlines()]
    assert code == 0 and [r[:2] for r in rows[:4]] == [["cd.wav", "0"], ["dl48.flac", "0"], ["dl96.wav", "0"], ["other.wav", "3"]]
    assert [r[6] for r in rows[:4]] == ["44100", "48000", "96000", "44100"]
    assert [r[:4] for r in rows[4:]] == [["pair", "cd.wav", "dl48.flac", "0.000"], ["pair", "cd.wav", "dl96.wav", "0.000"], ["pair", "dl48.flac", "dl96.wav", "0.000"]]
    code, out, _ = _run("--duplicates", "--dup-any-rate", "-o", "json", files[0], files[1], tmp_path / "missing.wav")
    d = json.loads(out)
    assert code == 1 and d["summary"] == {"total_files": 3, "successful": 2, "failed": 1} and d["groups"] == [[str(files[0]), str(files[1])]]
    assert d["pairs"][0]["lag_seconds"] == 0.0 and [f.get("sample_rate") for f in d["files"]] == [44100, 48000, None]


def test_dup_any_rate_requires_duplicates():
    from mp3rgain_amd import cli

    with pytest.raises(cli.CliError):
        cli.parse_args(["--dup-any-rate", "a.wav"], io.StringIO(), io.StringIO())
