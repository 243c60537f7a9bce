"""`--tempo` of the command line (mp3rgain_amd/cli.py) on the GPU: two files through rg_tempo, the reading the construction gives,
the three output forms, exit status 0 and 1 with a missing file."""
import io
import json
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import flacenc  # noqa: E402
import tempo_cases as tc  # noqa: E402
from wavutil import wav_bytes  # noqa: E402

pytestmark = pytest.mark.gpu


def _run(*args):
    from mp3rgain_amd import cli

    out, err = io.StringIO(), io.StringIO()
    code = cli.main([str(a) for a in args], out, err)
    return code, out.getvalue(), err.getvalue()


def test_tempo_on_files_text_tsv_json(tmp_path):
    from mp3rgain_amd import cli
    from mp3rgain_amd import replaygain as rgmod

    a = tc.fc.as_format(tc.click_track(128, 44100, 30) * 29000.0, "s16")
    b = tc.fc.as_format(tc.drum_pattern(90.5, 48000, 30) * 29000.0, "s16")
    flac = tmp_path / "a.flac"
    flac.write_bytes(flacenc.encode(np.stack([a]).astype(np.int64), 44100, 16, flacenc.Options(block_size=4096)))
    wav = tmp_path / "b.wav"
    wav.write_bytes(wav_bytes([b, b], 48000, "s16"))
    code, out, err = _run("--tempo", flac, wav)
    lines = out.splitlines()
    assert code == 0 and err == "" and lines[0].startswith("mp3rgain tempo of 2 file(s)") and len(lines) == 4
    want = []
    for planes, rate in (([a], 44100), ([b, b], 48000)):  # the kernels' arithmetic on the host, on the same PCM
        arena, descs = tc.pack([tc.Case("x", planes, rate)])
        want.append(rgmod.tempo_from_record(rgmod.tempo_arena(None, 2, descs, arena, bands=False)[0][0]))
    assert lines[2:] == [f"{cli.tempo_line(want[0])}  a.flac", f"{cli.tempo_line(want[1])}  b.wav"]
    assert abs(want[0].bpm - 128) < 0.5 and abs(want[1].bpm - 90.5) < 0.5 and lines[2].startswith("12") and " BPM  (confidence 0." in lines[2]
    code, out, _ = _run("--tempo", "--tempo-min", "100", "-o", "tsv", flac, wav)
    rows = [line.split("\t") for line in out.splitlines()]
    assert code == 0 and [r[0] for r in rows] == ["a.flac", "b.wav"] and abs(float(rows[0][1]) - 128) < 0.5 and abs(float(rows[1][1]) - 181) < 1.0
    assert rows[0][5] == "ok" and rows[0][9:] == [str(len(a)), "44100", "0"]
    code, out, _ = _run("--tempo", "-o", "json", flac, tmp_path / "missing.wav")
    d = json.loads(out)
    assert code == 1 and d["summary"] == {"total_files": 2, "successful": 1, "failed": 1}
    assert d["files"][1]["status"] == "error" and "Failed to open" in d["files"][1]["error"]
    f = d["files"][0]
    assert (f["bpm"], f["period16"], f["verdicts"], f["complete"]) == (want[0].bpm, want[0].period16, ["ok"], True)
