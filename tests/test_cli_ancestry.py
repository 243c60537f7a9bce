"""`--ancestry` of the command line (mp3rgain_amd/cli.py) without a GPU: option parsing, its errors and its conflicts, and the
text, TSV and JSON shapes on records the host route (rg_ancestry_arena, route 2) computes, handed to the command in place of
the GPU's."""
import io
import json
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import ancestry_cases as ac  # noqa: E402

from mp3rgain_amd import cli  # noqa: E402
from mp3rgain_amd import replaygain as rg  # noqa: E402


def _run(*args):
    out, err = io.StringIO(), io.StringIO()
    code = cli.main([str(a) for a in args], out, err)
    return code, out.getvalue(), err.getvalue()


def test_option_parsing_errors_and_conflicts():
    o = cli.parse_args(["--ancestry", "--ancestry-segments", "4", "--ancestry-granules", "8", "-o", "json", "a.wav", "b.flac"], io.StringIO(), io.StringIO())
    assert (o.ancestry, o.ancestry_segments, o.ancestry_granules, o.output_format, [str(f) for f in o.files]) == (True, 4, 8, "json", ["a.wav", "b.flac"])
    o = cli.parse_args(["--ancestry", "--ancestry-segments", "0", "a.wav"], io.StringIO(), io.StringIO())
    assert (o.ancestry, o.ancestry_segments, o.ancestry_granules) == (True, 0, None)
    for args, text in ((["--ancestry-segments", "5", "a.wav"], "--ancestry-segments requires --ancestry"),
                       (["--ancestry-granules", "5", "a.wav"], "--ancestry-granules requires --ancestry"),
                       (["--ancestry", "--ancestry-granules", "0", "a.wav"], "at least 1"),
                       (["--ancestry", "--ancestry-segments", "x", "a.wav"], "invalid segment count: x"),
                       (["--ancestry", "--ancestry-granules", "-3", "a.wav"], "invalid granule count: -3"),
                       (["--ancestry", "--stats", "a.wav"], "cannot be combined with --stats"), (["--spectrum", "--ancestry", "a.wav"], "--spectrum"),
                       (["--ancestry", "--dr", "a.wav"], "--dr"), (["--ancestry", "--verify", "a.wav"], "--verify"), (["--ancestry", "--rip", "a.wav"], "--rip"),
                       (["--ancestry", "--r128", "a.wav"], "--r128"), (["--ancestry", "-r", "a.wav"], "-r"), (["--ancestry", "-a", "a.wav"], "-a"),
                       (["--ancestry", "-x", "a.wav"], "-x"), (["--ancestry", "-g", "2", "a.wav"], "-g")):
        with pytest.raises(cli.CliError) as e:
            cli.parse_args(args, io.StringIO(), io.StringIO())
        assert text in str(e.value), args
        code, _, err = _run(*args)
        assert code == 1 and text in err
    code, _, err = _run("--ancestry", "--ancestry-segments")
    assert code == 1 and "--ancestry-segments requires an argument" in err
    code, _, err = _run("--ancestry")
    assert code == 1 and "no files specified" in err
    out = io.StringIO()
    cli.print_usage(out)
    assert "--ancestry " in out.getvalue() and "--ancestry-segments <S>" in out.getvalue() and "--ancestry-granules <G>" in out.getvalue()
    for field in ("grid_offset", "best_view", "active_total", "held to no", "short-block", "Opus"):
        assert field in out.getvalue()


class _HostAnalyzer:
    """Analyzer.ancestry from the host route: the named planes instead of files."""
    planes = {}
    seen = []

    def __init__(self, device=0):
        pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False

    def ancestry(self, files, segments=None, granules=None, z_min=None, iso_min=None, active_floor=None):
        type(self).seen.append((segments, granules))
        res = []
        for f in files:
            if str(f) not in self.planes:
                res.append(rg.ancestry_from_record(rg._capi.AncestryRecord(status=-8), rg.ReplayGainError(-8, f"Failed to open: {f}")))
                continue
            chans, rate, dropped = self.planes[str(f)]
            arena, descs = rg.pack_tracks([rg.PcmTrack(chans, rate)])
            rec = rg.ancestry_arena(None, 2, list(descs)[:1], arena, 3 if segments is None else segments, 3 if granules is None else granules)[0][0]
            rec.dropped_frames = dropped
            if dropped:
                rec.flags &= ~rg._capi.ANC_COMPLETE
            res.append(rg.ancestry_from_record(rec))
        return res


@pytest.fixture()
def host(capi, monkeypatch):
    by = {c.name: c for c in ac.cases()}
    coded, ms, clean = by["cut_coarse_k2000"], by["mp3_64_ms_k2000_s16"], by["clean_music_stereo"]
    nan = (clean.channels[0] / 32768.0).astype(np.float32)
    nan[777] = np.nan
    _HostAnalyzer.planes = {"coded.flac": (list(coded.channels), 44100, 0), "joint.wav": (list(ms.channels), 44100, 0), "clean.flac": (list(clean.channels), 44100, 0),
                            "damaged.flac": (list(coded.channels), 44100, 2), "short.wav": ([coded.channels[0][:100].copy()], 44100, 0),
                            "zeros.wav": ([np.zeros(5000, np.int16)], 44100, 0), "nan.wav": ([nan], 44100, 0)}
    _HostAnalyzer.seen = []
    monkeypatch.setattr(cli.rgmod, "Analyzer", _HostAnalyzer)
    return _HostAnalyzer


def _record(host, name, *opts):
    return host().ancestry([name], *opts)[0]


def test_text_one_line_per_file_and_the_views(host):
    coded, joint = _record(host, "coded.flac"), _record(host, "joint.wav")
    assert coded.mp3_grid and coded.grid_offset == 209 and joint.mp3_grid and joint.midside and joint.grid_offset == 209
    code, out, err = _run("--ancestry", "coded.flac", "joint.wav", "clean.flac")
    lines = out.splitlines()
    assert code == 0 and err == ""
    assert lines[0].startswith("mp3rgain ancestry scan of 3 file(s)") and "no other checker" in lines[0] and lines[1] == ""
    assert lines[2] == f"mp3 grid at +209 (z {coded.z:.1f}, x{coded.iso:.2f})   coded.flac"
    v = coded.views[0]
    assert lines[3] == f"    ch0: +209  {100 * v.ratio:.1f} % small (next {100 * v.second:.1f} %, others {100 * v.p0:.1f} %)  z {v.z:.1f}  x{v.iso:.2f}  *"
    assert lines[4] == f"mp3 grid at +209 (z {joint.z:.1f}, x{joint.iso:.2f}, mid/side)   joint.wav"
    assert [ln.split(":")[0].strip() for ln in lines[5:9]] == ["ch0", "ch1", "mid", "side"]
    assert lines[9] == "no grid found   clean.flac" and len(lines) == 14 and not any(ln.endswith("*") for ln in lines[10:])
    code, out, _ = _run("--ancestry", "-q", "coded.flac")
    assert code == 0 and out.splitlines() == [lines[2]]
    code, out, _ = _run("--ancestry", "-q", "short.wav", "zeros.wav", "nan.wav")
    lines = out.splitlines()
    assert code == 0 and lines[0] == "no grid found   short.wav  [silent, short]" and lines[1] == "no grid found   zeros.wav  [silent]"
    assert lines[2] == "no grid found   nan.wav  [nonfinite]"


def test_the_options_reach_the_analyzer(host):
    code, out, _ = _run("--ancestry", "--ancestry-segments", "0", "-o", "json", "coded.flac")
    d = json.loads(out)
    assert code == 0 and (0, None) in host.seen and d["files"][0]["segments"] == 1 and d["files"][0]["granules"] == len(ac.cases()[0].channels[0]) // 576 - 2
    code, out, _ = _run("--ancestry", "--ancestry-segments", "2", "--ancestry-granules", "1", "-o", "json", "coded.flac")
    d = json.loads(out)
    assert code == 0 and (2, 1) in host.seen and (d["files"][0]["segments"], d["files"][0]["granules"]) == (2, 1)


def test_tsv_and_json(host):
    joint = _record(host, "joint.wav")
    code, out, _ = _run("--ancestry", "-o", "tsv", "joint.wav", "clean.flac")
    rows = [line.split("\t") for line in out.splitlines()]
    assert code == 0 and len(rows) == 10
    n = len(ac.cases()[0].channels[0])
    assert rows[0] == ["joint.wav", "mp3-grid,mid/side", "209", f"{joint.z:.2f}", f"{joint.iso:.3f}", joint.views[joint.best_view].name, str(n), "44100", "2", "3", "3", "0"]
    v = joint.views[2]
    assert rows[3] == ["joint.wav", "view", "mid", str(v.offset), f"{v.ratio:.5f}", f"{v.second:.5f}", f"{v.p0:.5f}", f"{v.z:.2f}", f"{v.iso:.3f}", str(v.small),
                       str(v.active), str(int(v.flagged)), "0"]
    assert rows[5][:6] == ["clean.flac", "ok", "", "0.00", "0.000", ""]
    code, out, _ = _run("--ancestry", "-o", "json", "joint.wav", "zeros.wav")
    d = json.loads(out)
    assert code == 0 and d["summary"] == {"total_files": 2, "successful": 2, "failed": 0}
    f = d["files"][0]
    assert (f["file"], f["status"], f["verdicts"], f["mp3_grid"], f["grid_offset"], f["z"], f["iso"], f["midside"]) == \
        ("joint.wav", "success", ["mp3-grid", "mid/side"], True, 209, joint.z, joint.iso, True)
    assert (f["frames"], f["sample_rate"], f["segments"], f["granules"], f["dropped_frames"], f["complete"], f["short"], f["silent"]) == (n, 44100, 3, 3, 0, True, False, False)
    assert f["best_view"] in ("mid", "side") and f["views"][2] == {"view": "mid", "offset": v.offset, "ratio": v.ratio, "second": v.second, "p0": v.p0, "z": v.z,
                                                                    "iso": v.iso, "small": v.small, "active": v.active, "active_total": v.active_total,
                                                                    "flagged": v.flagged, "nonfinite": 0}
    z = d["files"][1]
    assert z["verdicts"] == ["silent"] and z["mp3_grid"] is False and z["grid_offset"] is None and z["best_view"] is None and z["views"][0]["active_total"] == 0


def test_exit_status_and_failing_files(host):
    code, out, err = _run("--ancestry", "-q", "coded.flac", "missing.wav")
    assert code == 1 and "missing.wav - Failed to open: missing.wav" in err and out.splitlines()[0].startswith("mp3 grid at +209")
    code, out, _ = _run("--ancestry", "-o", "json", "clean.flac", "missing.wav")
    d = json.loads(out)
    assert code == 1 and d["summary"] == {"total_files": 2, "successful": 1, "failed": 1} and d["files"][1] == {"file": "missing.wav", "status": "error",
                                                                                                                "error": "Failed to open: missing.wav"}
    code, out, _ = _run("--ancestry", "-o", "tsv", "missing.wav")
    assert code == 1 and out.splitlines() == ["missing.wav\tFailed to open: missing.wav"]
    code, out, _ = _run("--ancestry", "-q", "damaged.flac", "clean.flac")
    lines = out.splitlines()
    assert code == 1 and lines[0].startswith("mp3 grid at +209") and lines[0].endswith("damaged.flac  [incomplete, 2 frames dropped]")
    assert lines[1] == "no grid found   clean.flac"
