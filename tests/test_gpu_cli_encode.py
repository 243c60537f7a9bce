"""`--encode` of the command line on the GPU: the files it writes and its text, JSON, TSV and exit status."""
import io
import json
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import wavutil  # noqa: E402
from wavutil import wav_bytes  # noqa: E402

from mp3rgain_amd import cli, flacdec  # noqa: E402

pytestmark = pytest.mark.gpu


def _run(*args):
    out, err = io.StringIO(), io.StringIO()
    code = cli.main([str(a) for a in args], out, err)
    return code, out.getvalue(), err.getvalue()


def test_encode_command(tmp_path):
    chans = wavutil.test_signal("s16", 44100, 12345, 2, 5)
    src = tmp_path / "one.wav"
    src.write_bytes(wav_bytes(chans, 44100, "s16"))
    flt = tmp_path / "float.wav"
    flt.write_bytes(wav_bytes(wavutil.test_signal("f32", 44100, 1000, 2, 6), 44100, "f32"))
    d = tmp_path / "out"
    d.mkdir()
    code, out, err = _run("--encode", "--encode-dir", d, src)
    assert code == 0 and err == "" and f"one.wav -> {d / 'one.flac'}" in out and "% of the PCM, verified" in out and "1 of 1 file(s) written" in out
    data = (d / "one.flac").read_bytes()
    assert np.array_equal(flacdec.decode(data)[2], np.stack([np.asarray(c, dtype=np.int64) for c in chans]))
    # the output exists now: the file fails, the status says so, and the float file beside it fails in its own way
    code, out, err = _run("--encode", "--encode-dir", d, "-o", "json", src, flt)
    doc = json.loads(out)
    assert code == 1 and [f["status"] for f in doc["files"]] == ["error", "error"] and "exists" in doc["files"][0]["error"] and "float" in doc["files"][1]["error"]
    assert (d / "one.flac").read_bytes() == data
    d2 = tmp_path / "out2"
    d2.mkdir()
    code, out, err = _run("--encode", "--encode-dir", d2, "--encode-lpc", 0, "--encode-block", 1024, "--no-encode-verify", "-o", "json", src, flt)
    doc = json.loads(out)
    f = doc["files"][0]
    assert code == 1 and f["status"] == "success" and f["verified"] is False and f["block_size"] == 1024 and f["pcm_bytes"] == 12345 * 4
    assert f["stream_bytes"] == (d2 / "one.flac").stat().st_size == doc["stream_bytes"] and doc["summary"]["failed"] == 1
    d3 = tmp_path / "out3"
    d3.mkdir()
    code, out, err = _run("--encode", "--encode-dir", d3, "-o", "tsv", src)
    row = out.rstrip("\n").split("\t")
    assert code == 0 and row[0] == "one.wav" and row[1] == str(d3 / "one.flac") and int(row[2]) == len(data) and row[10] == "1" and len(row) == 12
    assert (d3 / "one.flac").read_bytes() == data
