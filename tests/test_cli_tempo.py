"""`--tempo` of the command line (mp3rgain_amd/cli.py) without a GPU: option parsing, its errors and its conflicts, and the text,
TSV and JSON shapes on canned records (and on one the host routes compute, rg_tempo_arena route 2), handed to the command in place
of the GPU's."""
import io
import json
import sys
from pathlib import Path

import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import tempo_cases as tc  # noqa: E402

from mp3rgain_amd import cli  # noqa: E402
from mp3rgain_amd import replaygain as rg  # noqa: E402

_capi = rg._capi
C, S, R, N = _capi.TEMPO_COMPLETE, _capi.TEMPO_SHORT, _capi.TEMPO_RATE, _capi.TEMPO_NONE


def _run(*args):
    out, err = io.StringIO(), io.StringIO()
    code = cli.main([str(a) for a in args], out, err)
    return code, out.getvalue(), err.getvalue()


def test_option_parsing_errors_and_conflicts():
    o = cli.parse_args(["--tempo", "--tempo-min", "60", "-o", "json", "a.wav", "b.flac"], io.StringIO(), io.StringIO())
    assert (o.tempo, o.tempo_min, o.output_format, [str(f) for f in o.files]) == (True, 60, "json", ["a.wav", "b.flac"])
    assert cli.parse_args(["--tempo", "a.wav"], io.StringIO(), io.StringIO()).tempo_min is None
    for args, text in ((["--tempo-min", "90", "a.wav"], "--tempo-min requires --tempo"),
                       (["--tempo", "--tempo-min", "29", "a.wav"], "30 to 300"), (["--tempo", "--tempo-min", "301", "a.wav"], "30 to 300"),
                       (["--tempo", "--tempo-min", "x", "a.wav"], "invalid BPM: x"),
                       (["--tempo", "--stats", "a.wav"], "cannot be combined with --stats"), (["--spectrum", "--tempo", "a.wav"], "--spectrum"),
                       (["--tempo", "--dr", "a.wav"], "--dr"), (["--tempo", "--verify", "a.wav"], "--verify"), (["--tempo", "--rip", "a.wav"], "--rip"),
                       (["--tempo", "--ancestry", "a.wav"], "--ancestry"), (["--tempo", "--duplicates", "a.wav"], "--duplicates"),
                       (["--duplicates", "--tempo", "a.wav"], "--tempo is a command of its own and cannot be combined with --duplicates"),
                       (["--tempo", "--r128", "a.wav"], "--r128"), (["--tempo", "-r", "a.wav"], "-r"), (["--tempo", "-a", "a.wav"], "-a"),
                       (["--tempo", "-x", "a.wav"], "-x"), (["--tempo", "-g", "2", "a.wav"], "-g")):
        with pytest.raises(cli.CliError) as e:
            cli.parse_args(args, io.StringIO(), io.StringIO())
        assert text in str(e.value), args
        code, _, err = _run(*args)
        assert code == 1 and text in err
    code, _, err = _run("--tempo", "--tempo-min")
    assert code == 1 and "--tempo-min requires an argument" in err
    code, _, err = _run("--tempo")
    assert code == 1 and "no files specified" in err
    out = io.StringIO()
    cli.print_usage(out)
    for field in ("--tempo ", "--tempo-min <BPM>", "first_beat_seconds", "no other BPM tool", "synthetic", f"default {_capi.TEMPO_MIN_BPM};"):
        assert field in out.getvalue(), field


def _rec(**kw):
    base = dict(frames=1764000, sample_rate=44100, channels=2, format=_capi.FMT_S16_PLANAR, dropped_frames=0, flags=C, onsets=3437, windows=6, period16=646,
                harmonics=8, bpm_milli=127999, confidence_permille=894, stable_permille=1000, first_beat=6924, nonfinite_frames=0)
    base.update(kw)
    return rg.Tempo(**base)


class _CannedAnalyzer:
    records = {}
    seen = []

    def __init__(self, device=0):
        pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False

    def tempo(self, files, window=None, hop=None, min_bpm=None):
        type(self).seen.append((window, hop, min_bpm))
        return [self.records[str(f)] if str(f) in self.records else
                rg.tempo_from_record(_capi.TempoRecord(status=-8), rg.ReplayGainError(-8, f"Failed to open: {f}")) for f in files]


@pytest.fixture()
def canned(capi, monkeypatch):
    none = dict(period16=0, bpm_milli=0, confidence_permille=0, stable_permille=0, first_beat=0)
    # one record is not canned: 12 s of a click track at 120 BPM through the kernels' arithmetic on the host, a shorter window
    arena, descs = tc.pack([tc.Case("x", [tc.fc.as_format(tc.click_track(120, 44100, 12) * 29000.0, "s16")], 44100)])
    _CannedAnalyzer.records = {"house.flac": _rec(), "drift.mp3": _rec(bpm_milli=90468, period16=914, confidence_permille=412, stable_permille=566, first_beat=15000,
                                                                        format=_capi.FMT_F32_PLANAR),
                               "silence.wav": _rec(flags=C | N, **none), "jingle.wav": _rec(flags=C | S, onsets=100, windows=0, **none),
                               "lowrate.wav": _rec(flags=C | S | R, sample_rate=8000, onsets=0, windows=0, harmonics=0, **none),
                               "damaged.flac": _rec(flags=0, dropped_frames=2),
                               "click.wav": rg.tempo_from_record(rg.tempo_arena(None, 2, descs, arena, window=256, hop=64, bands=False)[0][0])}
    _CannedAnalyzer.seen = []
    monkeypatch.setattr(cli.rgmod, "Analyzer", _CannedAnalyzer)
    return _CannedAnalyzer


def test_text_a_line_per_file(canned):
    code, out, err = _run("--tempo", "house.flac", "drift.mp3", "silence.wav", "jingle.wav", "lowrate.wav")
    lines = out.splitlines()
    assert code == 0 and err == ""
    assert lines[0].startswith("mp3rgain tempo of 5 file(s)") and "synthetic material only" in lines[0] and lines[1] == ""
    assert lines[2:] == ["128.00 BPM  (confidence 0.89, steady 1.00, first beat 0.157 s)  house.flac",
                         "90.47 BPM  (confidence 0.41, steady 0.57, first beat 0.340 s)  drift.mp3",
                         "no tempo found  silence.wav", "no tempo found  jingle.wav  [short]", "no tempo found  lowrate.wav  [rate]"]
    code, out, _ = _run("--tempo", "-q", "house.flac")
    assert code == 0 and out.splitlines() == ["128.00 BPM  (confidence 0.89, steady 1.00, first beat 0.157 s)  house.flac"]
    code, out, _ = _run("--tempo", "-q", "click.wav")
    r = canned.records["click.wav"]
    assert code == 0 and abs(r.bpm - 120.0) < 1.0 and out.splitlines() == [f"{cli.tempo_line(r)}  click.wav"] and out.startswith("1")


def test_the_option_reaches_the_analyzer(canned):
    _run("--tempo", "--tempo-min", "100", "-q", "house.flac")
    assert canned.seen[-1] == (None, None, 100)
    _run("--tempo", "-q", "house.flac")
    assert canned.seen[-1] == (None, None, None)


def test_tsv_and_json(canned):
    code, out, _ = _run("--tempo", "-o", "tsv", "house.flac", "silence.wav", "missing.wav")
    rows = [line.split("\t") for line in out.splitlines()]
    assert code == 1 and len(rows) == 3
    assert rows[0] == ["house.flac", "127.999", "0.894", "1.000", "0.157", "ok", "646", "3437", "6", "1764000", "44100", "0"]
    assert rows[1] == ["silence.wav", "", "", "", "", "none", "0", "3437", "6", "1764000", "44100", "0"]
    assert rows[2] == ["missing.wav", "Failed to open: missing.wav"]
    code, out, _ = _run("--tempo", "-o", "json", "house.flac", "jingle.wav")
    d = json.loads(out)
    assert code == 0 and d["summary"] == {"total_files": 2, "successful": 2, "failed": 0}
    f = d["files"][0]
    assert (f["file"], f["status"], f["bpm"], f["confidence"], f["steady"], f["first_beat"], f["period16"], f["harmonics"], f["verdicts"], f["complete"]) == \
        ("house.flac", "success", 127.999, 0.894, 1.0, 6924, 646, 8, ["ok"], True)
    assert abs(f["first_beat_seconds"] - 6924 / 44100) < 1e-12 and (f["onsets"], f["windows"], f["frames"], f["sample_rate"], f["channels"]) == (3437, 6, 1764000, 44100, 2)
    g = d["files"][1]
    assert (g["bpm"], g["first_beat_seconds"], g["first_beat"], g["verdicts"], g["period16"]) == (None, None, None, ["short"], 0)


def test_exit_status_and_failing_files(canned):
    code, out, err = _run("--tempo", "-q", "house.flac", "missing.wav")
    assert code == 1 and "missing.wav - Failed to open: missing.wav" in err and len(out.splitlines()) == 1
    code, out, _ = _run("--tempo", "-q", "damaged.flac")  # dropped frames: a reading, and exit status 1
    assert code == 1 and out.splitlines() == ["128.00 BPM  (confidence 0.89, steady 1.00, first beat 0.157 s)  damaged.flac  [incomplete, 2 frames dropped]"]
    code, out, _ = _run("--tempo", "-o", "json", "silence.wav", "missing.wav")
    d = json.loads(out)
    assert code == 1 and d["summary"] == {"total_files": 2, "successful": 1, "failed": 1}
    assert d["files"][1] == {"file": "missing.wav", "status": "error", "error": "Failed to open: missing.wav"}
