"""`--spectrum` of the command line (mp3rgain_amd/cli.py) on the GPU: files through rg_spectrum, text, TSV and JSON, exit status 0
with findings and 1 with a missing file."""
import io
import json
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import flacenc  # noqa: E402
import spectrum_cases as sc  # noqa: E402
from wavutil import wav_bytes  # noqa: E402

pytestmark = pytest.mark.gpu


def _run(*args):
    from mp3rgain_amd import cli

    out, err = io.StringIO(), io.StringIO()
    code = cli.main([str(a) for a in args], out, err)
    return code, out.getvalue(), err.getvalue()


def test_spectrum_on_files_text_tsv_json(tmp_path):
    cut, _ = sc.verdict_signal("white-16k")
    up, _ = sc.verdict_signal("pink-up96k")
    white, _ = sc.verdict_signal("white")
    wav = tmp_path / "a.wav"
    wav.write_bytes(wav_bytes([sc.as_s16(white)], 44100, "s16"))
    flac = tmp_path / "b.flac"
    flac.write_bytes(flacenc.encode(np.stack([sc.as_s16(cut), sc.as_s16(cut)]).astype(np.int64), 44100, 16))
    hires = tmp_path / "c.flac"
    hires.write_bytes(flacenc.encode((sc.as_s24(up) >> 8)[None, :].astype(np.int64), 96000, 24))
    code, out, err = _run("--spectrum", wav, flac, hires)
    assert code == 0 and err == ""
    lines = out.splitlines()
    assert "a.wav - ok  [44100 Hz]" in lines and "    no cutoff below Nyquist" in lines
    # the numbers in the words are the restatement's (the f32 edge may differ from the float64 one in the digits not printed)
    e, k, _ = sc.want_plane(sc.as_s16(cut))
    cutoff, edge, _ = sc.verdict_of_energy(e, k, 44100)
    assert abs(cutoff - 16200.0) <= 172.3
    assert "b.flac - bandlimited  [44100 Hz]" in lines and f"    cut off at {cutoff / 1000:.1f} kHz, edge {edge:.0f} dB" in lines
    e, k, _ = sc.want_plane(sc.as_s24(up))
    cutoff, _, _ = sc.verdict_of_energy(e, k, 96000)
    assert "c.flac - bandlimited, upsampled  [96000 Hz]" in lines and f"    96 kHz file with nothing above {cutoff / 1000:.1f} kHz" in lines
    code, out, _ = _run("--spectrum", "-o", "tsv", "--edge-db", "80", flac)
    rows = [line.split("\t") for line in out.splitlines()]
    assert code == 0 and rows[0][:4] == ["b.flac", "ok", "22050.0", "0.0"] and rows[1][:3] == ["b.flac", "ch", "0"] and len(rows) == 3
    code, out, _ = _run("--spectrum", "-o", "json", wav, tmp_path / "missing.wav", flac)
    d = json.loads(out)
    assert code == 1 and d["summary"] == {"total_files": 3, "successful": 2, "failed": 1}
    assert d["files"][1]["status"] == "error" and "Failed to open" in d["files"][1]["error"]
    want, analysed, _ = sc.want_plane(sc.as_s16(cut))
    c = d["files"][2]["channels"][1]
    assert (c["cutoff_hz"], c["bandlimited"]) == (sc.verdict_of_energy(want, analysed, 44100)[0], True) and c["analysed_frames"] == analysed
    lv = 10.0 * np.log10(want / want.max())
    assert len(c["levels_db"]) == 256 and np.abs(np.array(c["levels_db"]) - lv).max() < 0.02
