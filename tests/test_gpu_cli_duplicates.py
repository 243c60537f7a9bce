"""`--duplicates` of the command line (mp3rgain_amd/cli.py) on the GPU: files through rg_same_recording, the group and the lag
the construction gives, the three output forms, exit status 0 and 1 with a missing file."""
import io
import json
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import fingerprint_cases as fc  # noqa: E402
import flacenc  # noqa: E402
from wavutil import wav_bytes  # noqa: E402

pytestmark = pytest.mark.gpu

N = fc.L + 300 * fc.H


def _run(*args):
    from mp3rgain_amd import cli

    out, err = io.StringIO(), io.StringIO()
    code = cli.main([str(a) for a in args], out, err)
    return code, out.getvalue(), err.getvalue()


def test_duplicates_on_files_text_tsv_json(tmp_path):
    x, y = fc.noise(N + 4 * fc.H, 710), fc.noise(N, 711)
    flac = tmp_path / "a.flac"
    flac.write_bytes(flacenc.encode(np.stack([fc.as_format(x[:N], "s16")]).astype(np.int64), 44100, 16, flacenc.Options(block_size=4096)))
    wav = tmp_path / "b.wav"
    wav.write_bytes(wav_bytes([fc.as_format(y, "s16")], 44100, "s16"))
    late = tmp_path / "c.wav"  # the first, four codes earlier and at half the level
    late.write_bytes(wav_bytes([fc.as_format(x[4 * fc.H:4 * fc.H + N] * 0.5, "s16")], 44100, "s16"))
    code, out, err = _run("--duplicates", flac, wav, late)
    lines = out.splitlines()
    assert code == 0 and err == "" and lines[0].startswith("mp3rgain duplicate search among 3 file(s)")
    assert lines[2:4] == ["group 1: 2 files", "    a.flac"] and lines[4].startswith(f"    c.wav   {-4 * 512 / 44100:+.3f} s   0.") and lines[4].endswith("% of bits differ")
    assert lines[5:] == ["", "3 files, 1 groups of duplicates"]
    # 3 codes: the right offset is out of reach, and one code beside it more than 1 per mille of the bits differ
    code, out, _ = _run("--duplicates", "-o", "tsv", "--dup-radius", "0.03", "--dup-ber", "1", flac, wav, late)
    rows = [line.split("\t") for line in out.splitlines()]
    assert code == 0 and [r[:5] for r in rows] == [["a.flac", "0", "ok", "300", "0"], ["b.wav", "1", "ok", "300", "0"], ["c.wav", "2", "ok", "300", "0"]]
    code, out, _ = _run("--duplicates", "-o", "json", flac, tmp_path / "missing.wav", late)
    d = json.loads(out)
    assert code == 1 and d["summary"] == {"total_files": 3, "successful": 2, "failed": 1}
    assert d["files"][1]["status"] == "error" and "Failed to open" in d["files"][1]["error"]
    assert (d["files"][0]["group"], d["files"][2]["group"], d["files"][2]["matches"]) == (0, 0, 1)
    assert [(p["i"], p["j"], p["lag_codes"]) for p in d["pairs"]] == [(0, 2, -4)] and d["groups"] == [[str(flac), str(late)]]
