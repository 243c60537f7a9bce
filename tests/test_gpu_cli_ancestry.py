"""`--ancestry` of the command line (mp3rgain_amd/cli.py) on the GPU: files through rg_ancestry, the grid offset the
construction gives, the three output forms, exit status 0 and 1 with a missing file."""
import io
import json
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import ancestry_cases as ac  # noqa: E402
import flacenc  # noqa: E402
from wavutil import wav_bytes  # noqa: E402

pytestmark = pytest.mark.gpu


def _run(*args):
    from mp3rgain_amd import cli

    out, err = io.StringIO(), io.StringIO()
    code = cli.main([str(a) for a in args], out, err)
    return code, out.getvalue(), err.getvalue()


def test_ancestry_on_files_text_tsv_json(tmp_path):
    dec = ac.real_stream(64, 2, True, False)
    planes = [ac.to_s16(p[32:] * 32768.0) for p in dec]
    flac = tmp_path / "a.flac"
    flac.write_bytes(flacenc.encode(np.stack(planes).astype(np.int64), 44100, 16, flacenc.Options(block_size=1152)))
    wav = tmp_path / "b.wav"
    wav.write_bytes(wav_bytes([ac.to_s16(ac.music(12000, 60))], 44100, "s16"))
    want = ac.grid_after(32)
    code, out, err = _run("--ancestry", flac, wav)
    lines = out.splitlines()
    assert code == 0 and err == "" and lines[0].startswith("mp3rgain ancestry scan of 2 file(s)")
    assert lines[2].startswith(f"mp3 grid at +{want} (z ") and lines[2].endswith(", mid/side)   a.flac")
    assert [ln.split(":")[0].strip() for ln in lines[3:7]] == ["ch0", "ch1", "mid", "side"] and lines[7] == "no grid found   b.wav" and len(lines) == 9
    code, out, _ = _run("--ancestry", "-o", "tsv", "--ancestry-segments", "2", "--ancestry-granules", "3", flac)
    rows = [line.split("\t") for line in out.splitlines()]
    assert code == 0 and len(rows) == 5 and rows[0][:3] == ["a.flac", "mp3-grid,mid/side", str(want)] and rows[0][8:11] == ["2", "2", "3"]
    code, out, _ = _run("--ancestry", "-o", "json", flac, tmp_path / "missing.wav", wav)
    d = json.loads(out)
    assert code == 1 and d["summary"] == {"total_files": 3, "successful": 2, "failed": 1}
    assert d["files"][1]["status"] == "error" and "Failed to open" in d["files"][1]["error"]
    a, b = d["files"][0], d["files"][2]
    assert (a["mp3_grid"], a["grid_offset"], a["midside"], a["segments"], len(a["views"])) == (True, want, True, 1, 4) and a["best_view"] in ("mid", "side")
    assert (b["mp3_grid"], b["grid_offset"], b["verdicts"], len(b["views"])) == (False, None, ["ok"], 1)
