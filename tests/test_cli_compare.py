"""`--compare` of the command line (mp3rgain_amd/cli.py) without a GPU: option parsing, its errors and its conflicts, and every
line shape, the TSV and the JSON on records the host route (rg_compare_arena, route 0) computes from constructed planes, handed to
the command in place of the GPU's."""
import io
import json
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import arena_layouts as al  # noqa: E402
import compare_cases as cc  # noqa: E402

from mp3rgain_amd import _capi, cli  # noqa: E402
from mp3rgain_amd import replaygain as rg  # noqa: E402


def _run(*args):
    out, err = io.StringIO(), io.StringIO()
    code = cli.main([str(a) for a in args], out, err)
    return code, out.getvalue(), err.getvalue()


def test_option_parsing_errors_and_conflicts():
    o = cli.parse_args(["--compare", "--compare-radius", "100", "--compare-hint", "588", "-o", "json", "a.wav", "b.flac"], io.StringIO(), io.StringIO())
    assert (o.compare, o.compare_radius, o.compare_hint, o.output_format, [str(f) for f in o.files]) == (True, 100, 588, "json", ["a.wav", "b.flac"])
    o = cli.parse_args(["--compare", "a.wav", "b.wav", "c.wav"], io.StringIO(), io.StringIO())
    assert (o.compare, o.compare_radius, o.compare_hint, len(o.files)) == (True, None, None, 3)
    for args, text in ((["--compare-radius", "5", "a.wav", "b.wav"], "--compare-radius requires --compare"),
                       (["--compare-hint", "5", "a.wav", "b.wav"], "--compare-hint requires --compare"),
                       (["--compare", "--compare-radius", "2048", "a.wav", "b.wav"], "0 to 2047"),
                       (["--compare", "--compare-radius", "x", "a.wav", "b.wav"], "invalid radius: x"),
                       (["--compare", "--compare-hint", "1.5", "a.wav", "b.wav"], "invalid hint: 1.5"),
                       (["--compare", "--compare-hint", str((1 << 32) + 1), "a.wav", "b.wav"], "2^32"),
                       (["--compare", "a.wav"], "at least one file to hold against it"),
                       (["--compare", "--stereo", "a.wav", "b.wav"], "cannot be combined with --stereo"),
                       (["--stats", "--compare", "a.wav", "b.wav"], "cannot be combined with --stats"), (["--compare", "--dr", "a.wav", "b.wav"], "--dr"),
                       (["--compare", "--duplicates", "a.wav", "b.wav"], "--duplicates"), (["--compare", "--rip", "a.wav", "b.wav"], "--rip"),
                       (["--compare", "--verify", "a.wav", "b.wav"], "--verify"), (["--compare", "--r128", "a.wav", "b.wav"], "--r128"),
                       (["--compare", "--clicks", "a.wav", "b.wav"], "--clicks"), (["--compare", "-r", "a.wav", "b.wav"], "-r"),
                       (["--compare", "-a", "a.wav", "b.wav"], "-a"), (["--compare", "-g", "2", "a.wav", "b.wav"], "-g")):
        with pytest.raises(cli.CliError) as e:
            cli.parse_args(args, io.StringIO(), io.StringIO())
        assert text in str(e.value), args
        code, _, err = _run(*args)
        assert code == 1 and text in err
    code, _, err = _run("--compare", "--compare-radius")
    assert code == 1 and "--compare-radius requires an argument" in err
    out = io.StringIO()
    cli.print_usage(out)
    assert "--compare " in out.getvalue() and "--compare-radius <N>" in out.getvalue() and "--compare-hint <FRAMES>" in out.getvalue()


def _planes():
    rng = np.random.default_rng(3)
    n = 3 * 8000 + 500
    x = rng.integers(-20000, 20000, size=n).astype(np.int16)
    t = np.arange(n)
    drift = x.copy()
    drift[n // 2 + 7:] = x[n // 2:n - 7]
    coded = (x + rng.integers(-900, 900, size=n) * (t > 8000 + 104)).astype(np.int16)
    return {"ref.wav": x, "same.wav": x.copy(), "late.wav": np.concatenate([np.zeros(588, np.int16), x[:-1176]]),
            "gain.wav": np.rint(x * 10 ** (-3.01 / 20) + rng.triangular(-1, 0, 1, size=n)).astype(np.int16), "coded.wav": coded, "drift.wav": drift,
            "inverted.wav": (-x).astype(np.int16), "other.wav": rng.integers(-20000, 20000, size=n).astype(np.int16), "r48.wav": x.copy()}


class _HostAnalyzer:
    """Analyzer.compare from the serial host twin: the named planes instead of files, every file against the first."""

    def __init__(self, device=0):
        pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False

    def compare(self, files, hints=None, radius=None):
        planes = _planes()
        recs, trs, pairs = [], [], []
        for f in files:
            name = Path(str(f)).name
            trs.append(cc.Tr(name, [planes.get(name, np.zeros(4, np.int16))], 48000 if name == "r48.wav" else 8000))
        arena, descs, _ = al.pack(trs, al.Layout("abut", "loud", "input"))
        live = [k for k in range(1, len(files)) if Path(str(files[k])).name in planes]
        got = rg.compare_arena(None, 0, list(descs)[:len(trs)], [(0, k, hints or 0) for k in live], arena, radius=radius, segments=4, segment_frames=2000)
        by = dict(zip(live, got))
        for k in range(1, len(files)):
            if k in by:
                recs.append(rg.compare_from_record(by[k]))
            else:
                recs.append(rg.compare_from_record(_capi.CompareRecord(status=-8), rg.ReplayGainError(-8, f"Failed to open: {files[k]}")))
        return recs


@pytest.fixture()
def host(monkeypatch):
    monkeypatch.setattr(cli.rgmod, "Analyzer", _HostAnalyzer)


NAMES = ["same.wav", "late.wav", "gain.wav", "coded.wav", "drift.wav", "inverted.wav", "other.wav", "r48.wav"]


def test_every_line_shape(host):
    code, out, err = _run("--compare", "ref.wav", *NAMES)
    assert code == 0 and err == ""
    lines = out.strip().split("\n")
    assert lines[0].startswith("mp3rgain null test of 8 file(s) against ref.wav")
    body = lines[2:]
    assert body[0] == "identical  same.wav"
    assert body[1] == "identical samples, starts 588 samples later, 1176 shorter at the end  late.wav"
    assert body[2].startswith("same master  (gain +3.01 dB, residual 0.") and body[2].endswith(" LSB^2)  gain.wav")
    assert body[3].startswith("same recording, differs  (null -") and " dB after " in body[3] and "worst 0:0" in body[3]
    assert "first difference at 0:01.013)  coded.wav" in body[3]
    assert body[4] == "same recording, drifts  (lag 0 .. 7 samples over the file)  drift.wav"
    assert body[5].startswith("inverted copy, same master  (gain +0.00 dB, residual 0.00 LSB^2)  inverted.wav")
    assert body[6].startswith("not the same recording  (best correlation 0.0") and body[6].endswith(")  other.wav")
    assert body[7] == "different sample rate: not compared  r48.wav"


def test_a_failing_file_tsv_and_json(host):
    code, out, err = _run("--compare", "ref.wav", "late.wav", "missing.wav")
    assert code == 1 and "missing.wav - " in err and "Failed to open" in err and "late.wav" in out
    code, out, _ = _run("--compare", "-o", "tsv", "--compare-hint", "580", "--compare-radius", "16", "ref.wav", "late.wav", "gain.wav")
    rows = [ln.split("\t") for ln in out.strip().split("\n")]
    assert code == 0 and len(rows) == 2 and all(len(r) == 20 for r in rows)
    assert rows[0][:4] == ["late.wav", "identical,shifted,lengths differ", "588", "1"] and rows[0][8:13] == [str(24500 - 1176), "0", "1176", "588", "0"]
    assert rows[1][0] == "gain.wav" and rows[1][1].startswith("unrelated")  # the hint is every file's: 580 frames off, nothing within 16 of it
    code, out, _ = _run("--compare", "-o", "json", "ref.wav", "coded.wav", "same.wav", "missing.wav")
    doc = json.loads(out)
    assert code == 1 and doc["reference"] == "ref.wav" and [f["status"] for f in doc["files"]] == ["success", "success", "error"]
    rec = doc["files"][0]
    assert set(rg._COMPARE_FIELDS) <= set(rec) and rec["verdicts"] == ["differs"] and rec["first_diff"] == 8105 and rec["reading"].startswith("same recording")
    assert doc["files"][1]["first_diff"] is None and doc["files"][1]["null_db"] is None and doc["files"][1]["verdicts"] == ["identical"]
    assert doc["summary"] == {"total_files": 3, "successful": 2, "failed": 1}
