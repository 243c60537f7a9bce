"""`--stereo` of the command line (mp3rgain_amd/cli.py) without a GPU: option parsing, its errors and its conflicts, and the text,
TSV and JSON shapes on records the host route (rg_stereo_arena, route 2) computes, handed to the command in place of the GPU's."""
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
    o = cli.parse_args(["--stereo", "--stereo-radius", "100", "-o", "json", "a.wav", "b.flac"], io.StringIO(), io.StringIO())
    assert (o.stereo, o.stereo_radius, o.output_format, [str(f) for f in o.files]) == (True, 100, "json", ["a.wav", "b.flac"])
    o = cli.parse_args(["--stereo", "a.wav"], io.StringIO(), io.StringIO())
    assert (o.stereo, o.stereo_radius) == (True, None)
    assert cli.parse_args(["--stereo", "--stereo-radius", "0", "a.wav"], io.StringIO(), io.StringIO()).stereo_radius == 0
    for args, text in ((["--stereo-radius", "5", "a.wav"], "--stereo-radius requires --stereo"), (["--stereo", "--stereo-radius", "256", "a.wav"], "0 to 255"),
                       (["--stereo", "--stereo-radius", "x", "a.wav"], "invalid radius: x"), (["--stereo", "--stereo-radius", "-3", "a.wav"], "invalid radius: -3"),
                       (["--stereo", "--stats", "a.wav"], "cannot be combined with --stats"), (["--spectrum", "--stereo", "a.wav"], "cannot be combined with --spectrum"),
                       (["--stereo", "--dr", "a.wav"], "--dr"), (["--stereo", "--key", "a.wav"], "--key"), (["--tempo", "--stereo", "a.wav"], "--tempo"),
                       (["--stereo", "--duplicates", "a.wav"], "--duplicates"), (["--stereo", "--ancestry", "a.wav"], "--ancestry"),
                       (["--stereo", "--verify", "a.wav"], "--verify"), (["--stereo", "--rip", "a.wav"], "--rip"), (["--stereo", "--r128", "a.wav"], "--r128"),
                       (["--stereo", "-r", "a.wav"], "-r"), (["--stereo", "-a", "a.wav"], "-a"), (["--stereo", "-x", "a.wav"], "-x"),
                       (["--stereo", "-g", "2", "a.wav"], "-g")):
        with pytest.raises(cli.CliError) as e:
            cli.parse_args(args, io.StringIO(), io.StringIO())
        assert text in str(e.value), args
        code, _, err = _run(*args)
        assert code == 1 and text in err
    code, _, err = _run("--stereo", "--stereo-radius")
    assert code == 1 and "--stereo-radius requires an argument" in err
    code, _, err = _run("--stereo")
    assert code == 1 and "no files specified" in err
    out = io.StringIO()
    cli.print_usage(out)
    assert "--stereo " in out.getvalue() and "--stereo-radius <N>" in out.getvalue() and "held to no other tool" in out.getvalue()


class _HostAnalyzer:
    """Analyzer.stereo from the host route: the named planes instead of files."""
    planes = {}
    seen = []

    def __init__(self, device=0):
        pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False

    def stereo(self, files, radius=None, **kw):
        type(self).seen.append(radius)
        res = []
        for f in files:
            if str(f) not in self.planes:
                res.append(rg.stereo_from_record(rg._capi.StereoRecord(status=-8), rg.ReplayGainError(-8, f"Failed to open: {f}")))
                continue
            chans, rate, dropped = self.planes[str(f)]
            arena, descs = rg.pack_tracks([rg.PcmTrack(chans, rate)])
            rec = rg.stereo_arena(None, 2, list(descs)[:1], arena, radius)[0]
            rec.dropped_frames = dropped
            if dropped:
                rec.flags &= ~rg._capi.ST_COMPLETE
            res.append(rg.stereo_from_record(rec))
        return res


def _late(x, d):
    y = np.zeros_like(x)
    y[d:] = x[:len(x) - d]
    return y


@pytest.fixture()
def host(capi, monkeypatch):
    rng = np.random.default_rng(11)
    a = rng.integers(-12000, 12000, size=6000).astype(np.int16)
    b = rng.integers(-12000, 12000, size=6000).astype(np.int16)
    wide = [(a + b // 2).astype(np.int16), (a - b // 2).astype(np.int16)]
    nan = [(a / 32768.0).astype(np.float32), (b / 32768.0).astype(np.float32)]
    nan[0][77] = np.nan
    _HostAnalyzer.planes = {"wide.flac": (wide, 8000, 0), "dual.wav": ([a, a.copy()], 8000, 0), "flipped.wav": ([a, (-a).astype(np.int16)], 8000, 0),
                            "late.wav": ([a, _late(a, 3)], 8000, 0), "early.wav": ([_late(a, 1), a], 8000, 0), "far.wav": ([a, _late(a, 100)], 8000, 0),
                            "left.wav": ([a, np.zeros_like(a)], 8000, 0), "phase.wav": ([a, (-(a // 2) + b // 8).astype(np.int16)], 8000, 0),
                            "one.wav": ([a], 8000, 0), "quiet.wav": ([np.zeros(500, np.int16), np.zeros(500, np.int16)], 8000, 0),
                            "damaged.flac": (wide, 8000, 2), "nan.wav": (nan, 8000, 0), "six.wav": ([a, b, a, b, a, b], 8000, 0)}
    _HostAnalyzer.seen = []
    monkeypatch.setattr(cli.rgmod, "Analyzer", _HostAnalyzer)
    return _HostAnalyzer


def _record(host, name, radius=None):
    """The StereoImage the command is handed for `name`, to derive the expected numbers from."""
    return host().stereo([name], radius)[0]


def test_text_one_line_per_file(host):
    w, late, early = _record(host, "wide.flac"), _record(host, "late.wav"), _record(host, "early.wav")
    assert 0.5 < w.correlation < 0.7 and (late.lag, early.lag) == (3, -1)
    code, out, err = _run("--stereo", "wide.flac", "dual.wav", "flipped.wav", "late.wav", "early.wav", "left.wav", "phase.wav", "one.wav", "quiet.wav")
    lines = out.splitlines()
    assert code == 0 and err == ""
    assert lines[0].startswith("mp3rgain stereo image of 9 file(s): correlation, balance and channel delay within 64 samples") and lines[1] == ""
    assert "synthetic material only" in lines[0]
    assert lines[2] == f"stereo  (correlation {w.correlation:.2f}, side {w.side_db:+.1f} dB, balance {w.balance_db:+.1f} dB)  wide.flac"
    assert lines[3] == "dual mono  dual.wav"
    assert lines[4] == "right channel is the inverted left  flipped.wav  [out of phase]"
    assert lines[5] == f"right channel late by 3 samples (correlation {late.lag_correlation:.3f} there, {late.correlation:.2f} in place)  late.wav"
    assert lines[6] == f"left channel late by 1 sample (correlation {early.lag_correlation:.3f} there, {early.correlation:.2f} in place)  early.wav"
    assert lines[7].startswith("one-sided  (correlation 0.00, side +0.0 dB, balance +inf dB)  left.wav")
    assert lines[8].startswith("channels out of phase  (correlation -0.9") and lines[8].endswith("  phase.wav")
    assert lines[9] == "mono file  one.wav" and lines[10] == "silent  quiet.wav  [dual mono]" and len(lines) == 11
    # -q: no header; notes: non-finite samples, more channels; a delay beyond the radius is not found
    code, out, _ = _run("--stereo", "-q", "nan.wav", "six.wav", "far.wav")
    lines = out.splitlines()
    assert code == 0 and len(lines) == 3 and lines[0].endswith("nan.wav  [nonfinite]") and lines[1].endswith("six.wav  [more channels]")
    assert lines[2].startswith("stereo  (") and lines[2].endswith("far.wav")


def test_the_radius_reaches_the_analyzer(host):
    code, out, _ = _run("--stereo", "--stereo-radius", "128", "far.wav")
    assert code == 0 and host.seen == [128] and "within 128 samples" in out and "right channel late by 100 samples" in out
    code, out, _ = _run("--stereo", "-q", "--stereo-radius", "2", "late.wav")
    assert code == 0 and host.seen[-1] == 2 and out.startswith("stereo  (")


def test_tsv_and_json(host):
    late = _record(host, "late.wav")
    code, out, _ = _run("--stereo", "-o", "tsv", "late.wav", "left.wav")
    rows = [line.split("\t") for line in out.splitlines()]
    assert code == 0 and len(rows) == 2
    assert rows[0] == ["late.wav", "delayed", f"{late.correlation:.4f}", f"{late.side_db:.2f}", f"{late.balance_db:.2f}", "3", f"{late.lag_correlation:.4f}",
                       str(late.anti_lag), f"{late.anti_correlation:.4f}", "6000", "8000", "2", "64", "0"]
    assert rows[1][:5] == ["left.wav", "one-sided", "0.0000", "0.00", "inf"]
    code, out, _ = _run("--stereo", "-o", "json", "late.wav", "left.wav", "one.wav")
    d = json.loads(out)
    assert code == 0 and d["summary"] == {"total_files": 3, "successful": 3, "failed": 0}
    f = d["files"][0]
    assert (f["file"], f["status"], f["verdicts"], f["lag"], f["lag_sum"], f["lag_correlation"]) == ("late.wav", "success", ["delayed"], 3, late.lag_sum, late.lag_correlation)
    for name in ("correlation", "anti_correlation", "balance_db", "side_db", "anti_lag", "anti_sum", "ell", "err", "elr", "equal_frames", "opposite_frames",
                 "zero_frames", "nonfinite", "blocks", "active_blocks", "neg_blocks", "mono_blocks", "block_frames", "radius", "frames", "sample_rate", "channels",
                 "format", "flags", "dropped_frames"):
        assert f[name] == getattr(late, name), name
    assert f["complete"] is True and f["reading"].startswith("right channel late by 3 samples") and f["balance"] is None and f["side"] is None
    left = d["files"][1]
    assert left["verdicts"] == ["one-sided"] and left["balance_db"] is None and left["balance"] == "left" and left["side_db"] == 0.0
    assert d["files"][2]["verdicts"] == ["mono file"] and d["files"][2]["channels"] == 1


def test_exit_status_and_failing_files(host):
    code, out, err = _run("--stereo", "wide.flac", "missing.wav")
    assert code == 1 and "missing.wav - Failed to open: missing.wav" in err and out.splitlines()[-1].endswith("wide.flac")
    code, out, _ = _run("--stereo", "-o", "json", "dual.wav", "missing.wav")
    d = json.loads(out)
    assert code == 1 and d["summary"] == {"total_files": 2, "successful": 1, "failed": 1} and d["files"][1] == {"file": "missing.wav", "status": "error",
                                                                                                                "error": "Failed to open: missing.wav"}
    code, out, _ = _run("--stereo", "-o", "tsv", "missing.wav")
    assert code == 1 and out.splitlines() == ["missing.wav\tFailed to open: missing.wav"]
    code, out, _ = _run("--stereo", "-q", "damaged.flac", "dual.wav")
    lines = out.splitlines()
    assert code == 1 and lines[0].endswith("damaged.flac  [2 frames dropped]") and lines[1] == "dual mono  dual.wav"
    # verdicts never change the exit status
    assert _run("--stereo", "-q", "flipped.wav", "left.wav", "quiet.wav", "one.wav")[0] == 0
