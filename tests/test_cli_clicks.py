"""`--clicks` of the command line (mp3rgain_amd/cli.py) without a GPU: option parsing, its errors and its conflicts, and the text,
TSV and JSON shapes on records the host route (rg_clicks_arena, route 2) computes, handed to the command in place of the GPU's."""
import io
import json

import numpy as np
import pytest

from mp3rgain_amd import cli
from mp3rgain_amd import replaygain as rg


def _run(*args):
    out, err = io.StringIO(), io.StringIO()
    code = cli.main([str(a) for a in args], out, err)
    return code, out.getvalue(), err.getvalue()


def test_option_parsing_errors_and_conflicts():
    o = cli.parse_args(["--clicks", "--click-ratio", "12.5", "--click-order", "4", "--click-block", "512", "--click-list", "3", "-o", "json", "a.wav", "b.flac"],
                       io.StringIO(), io.StringIO())
    assert (o.clicks, o.click_ratio, o.click_order, o.click_block, o.click_list, o.output_format, [str(f) for f in o.files]) == (
        True, 12.5, 4, 512, 3, "json", ["a.wav", "b.flac"])
    o = cli.parse_args(["--clicks", "a.wav"], io.StringIO(), io.StringIO())
    assert (o.clicks, o.click_ratio, o.click_order, o.click_block, o.click_list) == (True, None, None, None, None)
    assert cli.parse_args(["--clicks", "--click-list", "0", "a.wav"], io.StringIO(), io.StringIO()).click_list == 0
    for args, text in ((["--click-ratio", "5", "a.wav"], "--click-ratio requires --clicks"), (["--click-list", "5", "a.wav"], "--click-list requires --clicks"),
                       (["--click-order", "4", "a.wav"], "--click-order requires --clicks"), (["--click-block", "256", "a.wav"], "--click-block requires --clicks"),
                       (["--clicks", "--click-ratio", "0.5", "a.wav"], "1 to 1000"), (["--clicks", "--click-ratio", "1001", "a.wav"], "1 to 1000"),
                       (["--clicks", "--click-ratio", "x", "a.wav"], "invalid ratio: x"), (["--clicks", "--click-order", "7", "a.wav"], "even order from 2 to 12"),
                       (["--clicks", "--click-order", "14", "a.wav"], "even order"), (["--clicks", "--click-block", "1000", "a.wav"], "256, 512, 1024, 2048 or 4096"),
                       (["--clicks", "--click-list", "257", "a.wav"], "0 to 256 events"), (["--clicks", "--click-list", "-1", "a.wav"], "invalid number of events: -1"),
                       (["--clicks", "--stats", "a.wav"], "cannot be combined with --stats"), (["--stereo", "--clicks", "a.wav"], "--stereo"),
                       (["--clicks", "--dr", "a.wav"], "--dr"), (["--clicks", "--key", "a.wav"], "--key"), (["--tempo", "--clicks", "a.wav"], "--tempo"),
                       (["--clicks", "--spectrum", "a.wav"], "--spectrum"), (["--clicks", "--verify", "a.wav"], "--verify"), (["--clicks", "--rip", "a.wav"], "--rip"),
                       (["--clicks", "--r128", "a.wav"], "--r128"), (["--clicks", "-r", "a.wav"], "-r"), (["--clicks", "-a", "a.wav"], "-a"),
                       (["--clicks", "-x", "a.wav"], "-x"), (["--clicks", "-g", "2", "a.wav"], "-g")):
        with pytest.raises(cli.CliError) as e:
            cli.parse_args(args, io.StringIO(), io.StringIO())
        assert text in str(e.value), args
        code, _, err = _run(*args)
        assert code == 1 and text in err
    code, _, err = _run("--clicks", "--click-ratio")
    assert code == 1 and "--click-ratio requires an argument" in err
    code, _, err = _run("--clicks")
    assert code == 1 and "no files specified" in err
    out = io.StringIO()
    cli.print_usage(out)
    text = out.getvalue()
    assert "--clicks " in text and "--click-ratio <X>" in text and "--click-list <K>" in text and "held" in text


class _HostAnalyzer:
    """Analyzer.clicks from the host route: the named planes instead of files."""
    planes = {}
    seen = []

    def __init__(self, device=0):
        pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False

    def clicks(self, files, **kw):
        type(self).seen.append(kw)
        res = []
        for f in files:
            if str(f) not in self.planes:
                res.append(rg.clicks_from_record(rg._capi.ClicksRecord(status=-8), (), rg.ReplayGainError(-8, f"Failed to open: {f}")))
                continue
            chans, rate, dropped = self.planes[str(f)]
            arena, descs = rg.pack_tracks([rg.PcmTrack(chans, rate)])
            recs, rows = rg.clicks_arena(None, 2, list(descs)[:1], arena, **kw)
            rec = recs[0]
            rec.dropped_frames = dropped
            if dropped:
                rec.flags &= ~rg._capi.CK_COMPLETE
            res.append(rg.clicks_from_record(rec, rows))
        return res


def _tone(n, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(n)
    return 6000.0 * (np.sin(t * 0.031) + 0.5 * np.sin(t * 0.173 + 1.0)) + rng.normal(0.0, 4.0, n)


def _s16(x):
    return np.clip(np.rint(x), -32768, 32767).astype(np.int16)


@pytest.fixture()
def host(capi, monkeypatch):
    n = 20000
    left, right = _tone(n, 1), _tone(n, 2)
    clean = [_s16(left), _s16(right)]
    l2, r2 = left.copy(), right.copy()
    l2[8500] += 3000.0    # 1.0625 s at 8 kHz
    l2[12000] -= 2500.0
    r2[16004] += 12000.0  # 2.0005 s
    r2[3000:3048:4] += 9000.0 * np.array([1, -1] * 6)  # a scratch: a burst
    nan = [(left / 32768.0).astype(np.float32)]
    nan[0][77] = np.nan
    many = left.copy()
    many[2000:19000:1000] += 9000.0
    _HostAnalyzer.planes = {"clean.flac": (clean, 8000, 0), "ticks.wav": ([_s16(l2), _s16(r2)], 8000, 0), "mono.wav": ([_s16(l2)], 8000, 0),
                            "quiet.wav": ([np.zeros(500, np.int16)], 8000, 0), "damaged.flac": (clean, 8000, 2), "nan.wav": (nan, 8000, 0),
                            "many.wav": ([_s16(many)], 8000, 0), "six.wav": ([_s16(l2)] + [_s16(right)] * 5, 8000, 0)}
    _HostAnalyzer.seen = []
    monkeypatch.setattr(cli.rgmod, "Analyzer", _HostAnalyzer)
    return _HostAnalyzer


def _record(host, name, **kw):
    return host().clicks([name], **kw)[0]


def test_text_one_line_per_file_and_the_events_under_it(host):
    t = _record(host, "ticks.wav")
    assert (t.ch[0].clicks, t.ch[1].clicks, t.ch[1].bursts) == (2, 1, 1)
    code, out, err = _run("--clicks", "clean.flac", "ticks.wav", "mono.wav", "quiet.wav")
    lines = out.splitlines()
    assert code == 0 and err == ""
    assert lines[0].startswith("mp3rgain click scan of 4 file(s): residual of a linear predictor against 8.371 times its local median") and lines[1] == ""
    assert "synthetic material only" in lines[0]
    assert lines[2] == "no clicks  clean.flac"
    s = t.strongest_click
    assert lines[3] == f"3 clicks (first at 0:01.062 left, strongest x{s[0] / 1000.0:.1f} at {cli._click_time(s[1], 8000)} {('left', 'right')[s[2]]}), 1 burst  ticks.wav"
    assert min(abs(s[1] - p) for p in (8500, 12000, 16004)) <= 9
    events = lines[4:8]
    assert [e.split(",")[0] for e in events] == ["    burst at 0:00.375 right", "    click at 0:01.062 left", "    click at 0:01.500 left", "    click at 0:02.000 right"]
    e = t.events[1]
    assert events[1] == f"    click at 0:01.062 left, {e.width} samples, x{e.strength_permille / 1000.0:.1f}"
    assert lines[8].startswith("2 clicks (first at 0:01.062, strongest x") and lines[8].endswith("  mono.wav") and " left" not in lines[8]
    assert lines[9].startswith("    click at 0:01.062, ") and lines[11] == "no clicks  quiet.wav  [silent]" and len(lines) == 12
    # -q: no header; notes: non-finite samples; more than two channels are named by number; a truncated list says so
    code, out, _ = _run("--clicks", "-q", "--click-list", "2", "nan.wav", "six.wav", "many.wav")
    lines = out.splitlines()
    # (a NaN reads as a zero in the middle of the wave: a click of its own)
    assert code == 0 and lines[0].startswith("1 click (first at 0:00.009, ") and lines[0].endswith("  nan.wav  [nonfinite]") and lines[1].startswith("    click at 0:00.009, ")
    assert lines[2].startswith("2 clicks (first at 0:01.062 ch 0, ") and lines[2].endswith("  six.wav") and lines[3].startswith("    click at 0:01.062 ch 0, ")
    assert lines[5].startswith("17 clicks (first at 0:00.250, strongest x") and lines[5].endswith("many.wav  [the first 2 of 17 events listed]")
    assert len(lines) == 8


def test_the_options_reach_the_analyzer(host):
    code, out, _ = _run("--clicks", "--click-ratio", "500", "--click-order", "4", "--click-block", "512", "--click-list", "5", "ticks.wav")
    assert code == 0 and host.seen == [dict(block_samples=512, order=4, ratio_permille=500000, max_events=5)]
    assert "against 500 times" in out
    assert out.splitlines()[2] == "no clicks  ticks.wav"
    code, out, _ = _run("--clicks", "-q", "--click-list", "0", "ticks.wav")
    assert code == 0 and host.seen[-1]["max_events"] == 0 and len(out.splitlines()) == 1 and out.startswith("3 clicks (")


def test_tsv_and_json(host):
    t = _record(host, "ticks.wav")
    code, out, _ = _run("--clicks", "-o", "tsv", "ticks.wav", "clean.flac")
    rows = [line.split("\t") for line in out.splitlines()]
    assert code == 0 and len(rows) == 1 + 4 + 1
    s = t.strongest_click
    assert rows[0] == ["ticks.wav", "3", "1", str(sum(c.flagged for c in t.ch)), str(t.first_click[0]), "0", f"{s[0] / 1000.0:.3f}", str(s[1]), str(s[2]), "4", "4", "20000",
                       "8000", "2", "8.371", "0"]
    e = t.events[0]
    assert rows[1] == ["ticks.wav", "burst", str(e.start), str(e.width), "1", str(e.peak_at), f"{e.strength_permille / 1000.0:.3f}"]
    assert rows[5][:6] == ["clean.flac", "0", "0", "0", "", ""]
    code, out, _ = _run("--clicks", "-o", "json", "ticks.wav", "clean.flac", "quiet.wav")
    d = json.loads(out)
    assert code == 0 and d["summary"] == {"total_files": 3, "successful": 3, "failed": 0}
    f = d["files"][0]
    assert (f["file"], f["status"], f["clicks"], f["bursts"], f["events_total"], f["listed"], f["truncated"]) == ("ticks.wav", "success", 3, 1, 4, 4, False)
    assert f["first_click"] == {"sample": t.first_click[0], "channel": 0, "time": "0:01.062"} and f["strongest_click"]["strength"] == s[0] / 1000.0
    assert f["events"][1] == dict(start=t.events[1].start, width=t.events[1].width, channel=0, kind="click", peak_at=t.events[1].peak_at,
                                  strength_permille=t.events[1].strength_permille, time="0:01.062")
    assert f["channel_records"][1]["bursts"] == 1 and f["channel_records"][0]["first_click"] == t.ch[0].first_click
    for name in ("block_samples", "order", "ratio_permille", "floor", "gap", "max_width", "max_events", "frames", "sample_rate", "channels", "format", "flags",
                 "dropped_frames", "nonfinite"):
        assert f[name] == getattr(t, name), name
    assert f["complete"] is True and f["reading"].startswith("3 clicks (first at 0:01.062 left")
    assert d["files"][1]["first_click"] is None and d["files"][1]["strongest_click"] is None and d["files"][1]["events"] == []
    assert d["files"][2]["reading"] == "no clicks" and d["files"][2]["channels"] == 1


def test_exit_status_and_failing_files(host):
    code, out, err = _run("--clicks", "clean.flac", "missing.wav")
    assert code == 1 and "missing.wav - Failed to open: missing.wav" in err and out.splitlines()[-1] == "no clicks  clean.flac"
    code, out, _ = _run("--clicks", "-o", "json", "clean.flac", "missing.wav")
    d = json.loads(out)
    assert code == 1 and d["summary"] == {"total_files": 2, "successful": 1, "failed": 1} and d["files"][1] == {"file": "missing.wav", "status": "error",
                                                                                                                "error": "Failed to open: missing.wav"}
    code, out, _ = _run("--clicks", "-o", "tsv", "missing.wav")
    assert code == 1 and out.splitlines() == ["missing.wav\tFailed to open: missing.wav"]
    code, out, _ = _run("--clicks", "-q", "damaged.flac", "clean.flac")
    lines = out.splitlines()
    assert code == 1 and lines[0] == "no clicks  damaged.flac  [2 frames dropped]" and lines[1] == "no clicks  clean.flac"
    # clicks never change the exit status
    assert _run("--clicks", "-q", "ticks.wav", "many.wav", "quiet.wav")[0] == 0
