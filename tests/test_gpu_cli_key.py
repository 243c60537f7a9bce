"""`--key` of the command line (mp3rgain_amd/cli.py) on the GPU: two files through rg_key, the reading the construction gives, the
three output forms, exit status 0 and 1 with a missing file."""
import io
import json
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import flacenc  # noqa: E402
import key_cases as kc  # noqa: E402
from wavutil import wav_bytes  # noqa: E402

pytestmark = pytest.mark.gpu


def _run(*args):
    from mp3rgain_amd import cli

    out, err = io.StringIO(), io.StringIO()
    code = cli.main([str(a) for a in args], out, err)
    return code, out.getvalue(), err.getvalue()


def test_key_on_files_text_tsv_json(tmp_path):
    from mp3rgain_amd import cli
    from mp3rgain_amd import replaygain as rgmod

    a = kc.fc.as_format(kc.progression(0, 44100, 16) * 29000.0, "s16")   # C major
    b = kc.fc.as_format(kc.progression(21, 48000, 16) * 29000.0, "s16")  # A minor
    wav = tmp_path / "c.wav"
    wav.write_bytes(wav_bytes([a, a], 44100, "s16"))
    flac = tmp_path / "am.flac"
    flac.write_bytes(flacenc.encode(np.stack([b]).astype(np.int64), 48000, 16, flacenc.Options(block_size=4096)))
    code, out, err = _run("--key", wav, flac)
    lines = out.splitlines()
    assert code == 0 and err == "" and lines[0].startswith("mp3rgain key of 2 file(s)") and len(lines) == 4
    want = []
    for planes, rate in (([a, a], 44100), ([b], 48000)):  # the kernels' arithmetic on the host, on the same PCM
        arena, descs = kc.pack([kc.Case("x", planes, rate)])
        want.append(rgmod.key_from_record(rgmod.key_arena(None, 2, descs, arena, bands=False)[0][0]))
    assert lines[2:] == [f"{cli.key_line(want[0])}  c.wav", f"{cli.key_line(want[1])}  am.flac"]
    assert lines[2].startswith("C major  (8B, correlation 0.") and lines[3].startswith("A minor  (8A, correlation 0.")
    code, out, _ = _run("--key", "--key-segment", "32", "-o", "tsv", wav, flac)
    rows = [line.split("\t") for line in out.splitlines()]
    assert code == 0 and [r[:4] for r in rows] == [["c.wav", "C major", "8B", "1d"], ["am.flac", "A minor", "8A", "1m"]]
    assert rows[0][7] == "ok" and rows[0][8] == "0" and rows[0][10] == str(want[0].rows // 32) and rows[0][11:] == [str(len(a)), "44100", "0"]
    code, out, _ = _run("--key", "-o", "json", flac, tmp_path / "missing.wav")
    d = json.loads(out)
    assert code == 1 and d["summary"] == {"total_files": 2, "successful": 1, "failed": 1}
    assert d["files"][1]["status"] == "error" and "Failed to open" in d["files"][1]["error"]
    f = d["files"][0]
    assert (f["key"], f["key_number"], f["correlation"], f["verdicts"], f["complete"]) == ("A minor", 21, want[1].correlation, ["ok"], True)
