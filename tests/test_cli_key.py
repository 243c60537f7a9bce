"""`--key` of the command line (mp3rgain_amd/cli.py) without a GPU: option parsing, its errors and its conflicts, and the text, TSV
and JSON shapes on canned records (and on one the host routes compute, rg_key_arena route 2), handed to the command in place of
the GPU's."""
import io
import json
import sys
from pathlib import Path

import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import key_cases as kc  # noqa: E402

from mp3rgain_amd import cli  # noqa: E402
from mp3rgain_amd import replaygain as rg  # noqa: E402

_capi = rg._capi
C, S, R, N = _capi.KEY_COMPLETE, _capi.KEY_SHORT, _capi.KEY_RATE, _capi.KEY_NONE


def _run(*args):
    out, err = io.StringIO(), io.StringIO()
    code = cli.main([str(a) for a in args], out, err)
    return code, out.getvalue(), err.getvalue()


def test_option_parsing_errors_and_conflicts():
    o = cli.parse_args(["--key", "--key-segment", "64", "-o", "json", "a.wav", "b.flac"], io.StringIO(), io.StringIO())
    assert (o.key, o.key_segment, o.output_format, [str(f) for f in o.files]) == (True, 64, "json", ["a.wav", "b.flac"])
    assert cli.parse_args(["--key", "a.wav"], io.StringIO(), io.StringIO()).key_segment is None
    for args, text in ((["--key-segment", "90", "a.wav"], "--key-segment requires --key"),
                       (["--key", "--key-segment", "7", "a.wav"], "8 to 4096"), (["--key", "--key-segment", "4097", "a.wav"], "8 to 4096"),
                       (["--key", "--key-segment", "x", "a.wav"], "invalid number of rows: x"),
                       (["--key", "--tempo", "a.wav"], "--key is a command of its own and cannot be combined with --tempo"),
                       (["--tempo", "--key", "a.wav"], "cannot be combined with --tempo"),
                       (["--key", "--stats", "a.wav"], "cannot be combined with --stats"), (["--spectrum", "--key", "a.wav"], "--spectrum"),
                       (["--key", "--dr", "a.wav"], "--dr"), (["--key", "--verify", "a.wav"], "--verify"), (["--key", "--rip", "a.wav"], "--rip"),
                       (["--key", "--ancestry", "a.wav"], "--ancestry"), (["--key", "--duplicates", "a.wav"], "--duplicates"),
                       (["--key", "--r128", "a.wav"], "--r128"), (["--key", "-r", "a.wav"], "-r"), (["--key", "-a", "a.wav"], "-a"),
                       (["--key", "-x", "a.wav"], "-x"), (["--key", "-g", "2", "a.wav"], "-g")):
        with pytest.raises(cli.CliError) as e:
            cli.parse_args(args, io.StringIO(), io.StringIO())
        assert text in str(e.value), args
        code, _, err = _run(*args)
        assert code == 1 and text in err
    code, _, err = _run("--key", "--key-segment")
    assert code == 1 and "--key-segment requires an argument" in err
    code, _, err = _run("--key")
    assert code == 1 and "no files specified" in err
    out = io.StringIO()
    cli.print_usage(out)
    for field in ("--key ", "--key-segment <rows>", "open_key", "no", "other key finder", "synthetic", f"default {_capi.KEY_SEGMENT},"):
        assert field in out.getvalue(), field


def _rec(**kw):
    base = dict(frames=1764000, sample_rate=44100, channels=2, format=_capi.FMT_S16_PLANAR, dropped_frames=0, flags=C, decim=8, decimated=220485, rows=423,
                silent_rows=0, nonfinite_frames=0, key=21, tonic=9, mode=1, correlation_permille=931, margin_permille=274, segments=3, stable_permille=1000)
    base.update(kw)
    return rg.Key(**base)


class _CannedAnalyzer:
    records = {}
    seen = []

    def __init__(self, device=0):
        pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False

    def key(self, files, segment=None):
        type(self).seen.append(segment)
        return [self.records[str(f)] if str(f) in self.records else
                rg.key_from_record(_capi.KeyRecord(status=-8), rg.ReplayGainError(-8, f"Failed to open: {f}")) for f in files]


@pytest.fixture()
def canned(capi, monkeypatch):
    none = dict(key=0, tonic=0, mode=0, correlation_permille=0, margin_permille=0, stable_permille=0)
    # one record is not canned: 6 s of a C major chord through the kernels' arithmetic on the host
    arena, descs = kc.pack([kc.Case("x", [kc.fc.as_format(kc.chord(6 * 44100, 44100), "s16")], 44100)])
    _CannedAnalyzer.records = {"song.flac": _rec(), "major.mp3": _rec(key=0, tonic=0, mode=0, correlation_permille=887, margin_permille=301, stable_permille=666,
                                                                      format=_capi.FMT_F32_PLANAR),
                               "silence.wav": _rec(flags=C | N, silent_rows=423, **none), "jingle.wav": _rec(flags=C | S, decimated=100, rows=0, segments=0, **none),
                               "lowrate.wav": _rec(flags=C | S | R, sample_rate=4000, decim=0, decimated=0, rows=0, segments=0, **none),
                               "damaged.flac": _rec(flags=0, dropped_frames=2),
                               "chord.wav": rg.key_from_record(rg.key_arena(None, 2, descs, arena, segment=16, bands=False)[0][0])}
    _CannedAnalyzer.seen = []
    monkeypatch.setattr(cli.rgmod, "Analyzer", _CannedAnalyzer)
    return _CannedAnalyzer


def test_text_a_line_per_file(canned):
    code, out, err = _run("--key", "song.flac", "major.mp3", "silence.wav", "jingle.wav", "lowrate.wav")
    lines = out.splitlines()
    assert code == 0 and err == ""
    assert lines[0].startswith("mp3rgain key of 5 file(s)") and "synthetic material only" in lines[0] and lines[1] == ""
    assert lines[2:] == ["A minor  (8A, correlation 0.93, margin 0.27, steady 1.00)  song.flac",
                         "C major  (8B, correlation 0.89, margin 0.30, steady 0.67)  major.mp3",
                         "no key found  silence.wav", "no key found  jingle.wav  [short]", "no key found  lowrate.wav  [rate]"]
    code, out, _ = _run("--key", "-q", "song.flac")
    assert code == 0 and out.splitlines() == ["A minor  (8A, correlation 0.93, margin 0.27, steady 1.00)  song.flac"]
    code, out, _ = _run("--key", "-q", "chord.wav")
    r = canned.records["chord.wav"]
    assert code == 0 and r.name == "C major" and out.splitlines() == [f"{cli.key_line(r)}  chord.wav"] and out.startswith("C major  (8B, ")


def test_the_option_reaches_the_analyzer(canned):
    _run("--key", "--key-segment", "64", "-q", "song.flac")
    assert canned.seen[-1] == 64
    _run("--key", "-q", "song.flac")
    assert canned.seen[-1] is None


def test_tsv_and_json(canned):
    code, out, _ = _run("--key", "-o", "tsv", "song.flac", "silence.wav", "missing.wav")
    rows = [line.split("\t") for line in out.splitlines()]
    assert code == 1 and len(rows) == 3
    assert rows[0] == ["song.flac", "A minor", "8A", "1m", "0.931", "0.274", "1.000", "ok", "21", "423", "3", "1764000", "44100", "0"]
    assert rows[1] == ["silence.wav", "", "", "", "", "", "", "none", "", "423", "3", "1764000", "44100", "0"]
    assert rows[2] == ["missing.wav", "Failed to open: missing.wav"]
    code, out, _ = _run("--key", "-o", "json", "song.flac", "jingle.wav")
    d = json.loads(out)
    assert code == 0 and d["summary"] == {"total_files": 2, "successful": 2, "failed": 0}
    f = d["files"][0]
    assert (f["file"], f["status"], f["key"], f["camelot"], f["open_key"], f["key_number"], f["tonic"], f["mode"], f["correlation"], f["margin"], f["steady"]) == \
        ("song.flac", "success", "A minor", "8A", "1m", 21, 9, "minor", 0.931, 0.274, 1.0)
    assert (f["verdicts"], f["complete"], f["rows"], f["segments"], f["decim"], f["frames"], f["sample_rate"], f["channels"]) == (["ok"], True, 423, 3, 8, 1764000, 44100, 2)
    g = d["files"][1]
    assert (g["key"], g["camelot"], g["open_key"], g["key_number"], g["mode"], g["verdicts"]) == (None, None, None, None, None, ["short"])


def test_exit_status_and_failing_files(canned):
    code, out, err = _run("--key", "-q", "song.flac", "missing.wav")
    assert code == 1 and "missing.wav - Failed to open: missing.wav" in err and len(out.splitlines()) == 1
    code, out, _ = _run("--key", "-q", "damaged.flac")  # dropped frames: a reading, and exit status 1
    assert code == 1 and out.splitlines() == ["A minor  (8A, correlation 0.93, margin 0.27, steady 1.00)  damaged.flac  [incomplete, 2 frames dropped]"]
    code, out, _ = _run("--key", "-o", "json", "silence.wav", "missing.wav")
    d = json.loads(out)
    assert code == 1 and d["summary"] == {"total_files": 2, "successful": 1, "failed": 1}
    assert d["files"][1] == {"file": "missing.wav", "status": "error", "error": "Failed to open: missing.wav"}
