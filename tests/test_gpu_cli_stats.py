"""`--stats` of the command line (mp3rgain_amd/cli.py) on the GPU: files through rg_pcm_stats, the numbers against the numpy
restatement (tests/pcm_stats_cases.py), exit status 0 with findings and 1 with a missing file."""
import io
import json
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import flacenc  # noqa: E402
import pcm_stats_cases as pc  # noqa: E402
from wavutil import wav_bytes  # noqa: E402

pytestmark = pytest.mark.gpu


def _run(*args):
    from mp3rgain_amd import cli

    out, err = io.StringIO(), io.StringIO()
    code = cli.main([str(a) for a in args], out, err)
    return code, out.getvalue(), err.getvalue()


def test_stats_on_files_text_tsv_json(tmp_path):
    rng = np.random.default_rng(61)
    n = 20000
    pcm = flacenc.test_pcm(rng, 2, n, 16).astype(np.int16)
    pcm[0, 4410:4420] = 32767
    pcm[1, 9000:9200] = 0
    pcm[:, :20] = 0
    wav = tmp_path / "a.wav"
    wav.write_bytes(wav_bytes([pcm[0], pcm[1]], 44100, "s16"))
    quiet = flacenc.test_pcm(rng, 2, 5000, 16) >> 2
    flac = tmp_path / "b.flac"
    flac.write_bytes(flacenc.encode(quiet << 8, 44100, 24, flacenc.Options(block_size=1152)))
    w = pc.want_track(pc.Tr("a", [pcm[0], pcm[1]], 44100, 16), 3, 64)
    code, out, err = _run("--stats", wav, flac)
    assert code == 0 and err == ""
    assert "a.wav - clipped, dropout  [16 of 16 bits, silence 20 + 0 frames]" in out and "clipped 10 in 1 run(s) first at 0:00.100" in out
    assert "dropouts 1 (longest 200)" in out and "b.flac - padded  [16 of 24 bits" in out
    code, out, _ = _run("--stats", "-o", "tsv", "--zero-run", "201", wav)
    rows = [line.split("\t") for line in out.splitlines()]
    assert code == 0 and rows[0][:3] == ["a.wav", "clipped", str(n)] and rows[2][10:] == ["0", "200"]
    code, out, _ = _run("--stats", "-o", "json", wav, tmp_path / "missing.wav", flac)
    d = json.loads(out)
    assert code == 1 and d["summary"] == {"total_files": 3, "successful": 2, "failed": 1}
    assert d["files"][1]["status"] == "error" and "Failed to open" in d["files"][1]["error"]
    for k, c in enumerate(d["files"][0]["channels"]):
        for f in ("min", "max", "sum", "clipped", "clip_runs", "longest_clip_run", "zeros", "lead_zeros", "trail_zeros", "zero_runs", "longest_zero_run"):
            assert c[f] == w["ch"][k][f], (k, f)
    assert d["files"][2]["verdicts"] == ["padded"] and d["files"][2]["effective_bits"] == 16
