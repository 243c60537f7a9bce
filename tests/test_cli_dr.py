"""`--dr` of the command line (mp3rgain_amd/cli.py) without a GPU: option parsing, its errors and its conflicts, and the text, TSV
and JSON shapes on records the host route (rg_dr_arena, route 2) computes, handed to the command in place of the GPU's."""
import io
import json
import math

import numpy as np
import pytest

from mp3rgain_amd import cli
from mp3rgain_amd import replaygain as rg


def _run(*args):
    out, err = io.StringIO(), io.StringIO()
    code = cli.main([str(a) for a in args], out, err)
    return code, out.getvalue(), err.getvalue()


def test_option_parsing_errors_and_conflicts():
    o = cli.parse_args(["--dr", "--dr-top", "100", "-o", "json", "a.wav", "b.flac"], io.StringIO(), io.StringIO())
    assert (o.dr, o.dr_top, o.output_format, [str(f) for f in o.files]) == (True, 100, "json", ["a.wav", "b.flac"])
    o = cli.parse_args(["--dr", "a.wav"], io.StringIO(), io.StringIO())
    assert (o.dr, o.dr_top) == (True, None)
    for args, text in ((["--dr-top", "5", "a.wav"], "--dr-top requires --dr"), (["--dr", "--dr-top", "0", "a.wav"], "1 to 1000"),
                       (["--dr", "--dr-top", "1001", "a.wav"], "1 to 1000"), (["--dr", "--dr-top", "x", "a.wav"], "invalid per mille value: x"),
                       (["--dr", "--dr-top", "-3", "a.wav"], "invalid per mille value: -3"),
                       (["--dr", "--stats", "a.wav"], "cannot be combined with --stats"), (["--spectrum", "--dr", "a.wav"], "cannot be combined with --spectrum"),
                       (["--dr", "--verify", "a.wav"], "--verify"), (["--dr", "--rip", "a.wav"], "--rip"), (["--dr", "--r128", "a.wav"], "--r128"),
                       (["--dr", "-r", "a.wav"], "-r"), (["--dr", "-a", "a.wav"], "-a"), (["--dr", "-x", "a.wav"], "-x"), (["--dr", "-g", "2", "a.wav"], "-g")):
        with pytest.raises(cli.CliError) as e:
            cli.parse_args(args, io.StringIO(), io.StringIO())
        assert text in str(e.value), args
        code, _, err = _run(*args)
        assert code == 1 and text in err
    code, _, err = _run("--dr", "--dr-top")
    assert code == 1 and "--dr-top requires an argument" in err
    code, _, err = _run("--dr")
    assert code == 1 and "no files specified" in err
    out = io.StringIO()
    cli.print_usage(out)
    assert "--dr " in out.getvalue() and "--dr-top <permille>" in out.getvalue() and "unverified" in out.getvalue()
    for field in ("dr_mean", "peak_db", "rms_db", "block_frames", "top_blocks", "album_dr"):
        assert field in out.getvalue()


class _HostAnalyzer:
    """Analyzer.dynamic_range from the host route: the named planes instead of files."""
    planes = {}
    seen = []

    def __init__(self, device=0):
        pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False

    def dynamic_range(self, files, block_frames=None, top_permille=None):
        type(self).seen.append((block_frames, top_permille))
        res = []
        for f in files:
            if str(f) not in self.planes:
                res.append(rg.dynamic_range_from_record(rg._capi.DrRecord(status=-8), rg.ReplayGainError(-8, f"Failed to open: {f}")))
                continue
            chans, rate, dropped = self.planes[str(f)]
            arena, descs = rg.pack_tracks([rg.PcmTrack(chans, rate)])
            rec = rg.dr_arena(None, 2, list(descs)[:1], arena, block_frames, top_permille)[0]
            rec.dropped_frames = dropped
            if dropped:
                rec.flags &= ~rg._capi.DR_COMPLETE
            res.append(rg.dynamic_range_from_record(rec))
        return res


@pytest.fixture()
def host(capi, monkeypatch):
    t = np.arange(20 * 8000)
    env = np.where((t // 24000) % 2 == 0, 1.0, 0.25)  # 3-second blocks at 8 kHz, loud and quiet in turn
    loud = np.rint(7500.0 * env * np.sin(2.0 * np.pi * 441.0 * t / 8000.0)).astype(np.int16)
    loud[[1000, 50000]] = 32767  # single full-scale samples in two blocks
    flat = np.rint(30000.0 * np.sin(2.0 * np.pi * 441.0 * t / 8000.0)).astype(np.int16)
    nan = (loud / 32768.0).astype(np.float32)
    nan[777] = np.nan
    _HostAnalyzer.planes = {"loud.flac": ([loud, flat], 8000, 0), "flat.wav": ([flat], 8000, 0), "damaged.flac": ([flat], 8000, 2),
                            "short.wav": ([flat[:100].copy()], 8000, 0), "zeros.wav": ([np.zeros(50000, np.int16)], 8000, 0), "nan.wav": ([nan], 8000, 0)}
    _HostAnalyzer.seen = []
    monkeypatch.setattr(cli.rgmod, "Analyzer", _HostAnalyzer)
    return _HostAnalyzer


def _record(host, name, *opts):
    """The DynamicRange the command is handed for `name`, to derive the expected numbers from."""
    return host().dynamic_range([name], *opts)[0]


def test_text_one_line_per_file_channels_and_the_album_line(host):
    loud, flat = _record(host, "loud.flac"), _record(host, "flat.wav")
    assert loud.channels[0].dr > 10.0 and abs(flat.dr_mean) < 0.05 and loud.dr == round((loud.channels[0].dr + loud.channels[1].dr) / 2)
    code, out, err = _run("--dr", "loud.flac", "flat.wav")
    lines = out.splitlines()
    assert code == 0 and err == ""
    assert lines[0].startswith("mp3rgain dynamic range of 2 file(s): 3-second blocks, the loudest 200 per mille") and "unverified" in lines[0] and lines[1] == ""
    assert lines[2] == f"DR{loud.dr:<3d} {loud.peak_db:8.2f} dB peak {loud.rms_db:8.2f} dB RMS   loud.flac"
    assert lines[3] == f"    ch 0: DR {loud.channels[0].dr:.2f}  peak {loud.channels[0].peak_db:.2f} dB  RMS {loud.channels[0].rms_db:.2f} dB  blocks 1 of 7"
    assert lines[4].startswith("    ch 1: DR ") and lines[5].startswith(f"DR{flat.dr:<3d} ") and lines[5].endswith("flat.wav")
    assert lines[-1] == f"album DR{rg.album_dr([loud, flat])}" and len(lines) == 8
    # one file: no album line; -q: no header and no channel lines
    code, out, _ = _run("--dr", "-q", "loud.flac")
    assert code == 0 and out.splitlines() == [lines[2]]
    # notes: short, silent, non-finite
    code, out, _ = _run("--dr", "-q", "short.wav", "zeros.wav", "nan.wav")
    lines = out.splitlines()
    assert code == 0 and lines[0].endswith("short.wav  [short]") and lines[1].endswith("zeros.wav  [silent]") and lines[2].endswith("nan.wav  [nonfinite]")
    assert lines[1].startswith("DR0       -inf dB peak     -inf dB RMS")


def test_dr_top_reaches_the_analyzer(host):
    code, out, _ = _run("--dr", "--dr-top", "1000", "loud.flac")
    all_blocks = _record(host, "loud.flac", None, 1000)
    assert code == 0 and (None, 1000) in host.seen and "the loudest 1000 per mille" in out and "blocks 7 of 7" in out
    assert f"DR{all_blocks.dr:<3d} " in out and all_blocks.channels[0].dr > _record(host, "loud.flac").channels[0].dr + 1.0


def test_tsv_and_json(host):
    loud = _record(host, "loud.flac")
    code, out, _ = _run("--dr", "-o", "tsv", "loud.flac", "flat.wav")
    rows = [line.split("\t") for line in out.splitlines()]
    assert code == 0 and len(rows) == 6
    assert rows[0] == ["loud.flac", "ok", str(loud.dr), f"{loud.dr_mean:.2f}", f"{loud.peak_db:.2f}", f"{loud.rms_db:.2f}", "160000", "8000", "2", "24000", "0"]
    c = loud.channels[1]
    assert rows[2] == ["loud.flac", "ch", "1", f"{c.dr:.2f}", f"{c.peak_db:.2f}", f"{c.rms_db:.2f}", str(c.peak), str(c.peak2), "7", "1", "0"]
    assert rows[-1] == ["album", str(rg.album_dr([loud, _record(host, "flat.wav")]))]
    code, out, _ = _run("--dr", "-o", "json", "loud.flac", "zeros.wav")
    d = json.loads(out)
    assert code == 0 and d["summary"] == {"total_files": 2, "successful": 2, "failed": 0} and d["album_dr"] == rg.album_dr([loud, _record(host, "zeros.wav")])
    f = d["files"][0]
    assert (f["file"], f["status"], f["verdicts"], f["dr"], f["dr_mean"], f["peak_db"], f["rms_db"]) == ("loud.flac", "success", ["ok"], loud.dr, loud.dr_mean,
                                                                                                         loud.peak_db, loud.rms_db)
    assert (f["frames"], f["sample_rate"], f["block_frames"], f["dropped_frames"], f["complete"], f["short"], f["silent"]) == (160000, 8000, 24000, 0, True, False, False)
    assert f["channels"][1] == {"dr": c.dr, "peak_db": c.peak_db, "rms_db": c.rms_db, "top_ms": c.top_ms, "mean_square": c.mean_square, "peak": c.peak,
                                "peak2": c.peak2, "blocks": 7, "top_blocks": 1, "nonfinite": 0}
    z = d["files"][1]
    assert z["verdicts"] == ["silent"] and z["peak_db"] is None and z["rms_db"] is None and z["channels"][0]["peak_db"] is None and z["dr"] == 0
    code, out, _ = _run("--dr", "-o", "json", "loud.flac")
    assert "album_dr" not in json.loads(out)


def test_exit_status_and_failing_files(host):
    code, out, err = _run("--dr", "loud.flac", "missing.wav")
    assert code == 1 and "missing.wav - Failed to open: missing.wav" in err and out.splitlines()[-1] == f"album DR{_record(host, 'loud.flac').dr}"
    code, out, _ = _run("--dr", "-o", "json", "flat.wav", "missing.wav")
    d = json.loads(out)
    assert code == 1 and d["summary"] == {"total_files": 2, "successful": 1, "failed": 1} and d["files"][1] == {"file": "missing.wav", "status": "error",
                                                                                                                "error": "Failed to open: missing.wav"}
    code, out, _ = _run("--dr", "-o", "tsv", "missing.wav")
    assert code == 1 and out.splitlines() == ["missing.wav\tFailed to open: missing.wav"]
    code, out, _ = _run("--dr", "-q", "damaged.flac", "flat.wav")
    lines = out.splitlines()
    assert code == 1 and lines[0].endswith("damaged.flac  [incomplete, 2 frames dropped]") and lines[2] == f"album DR{_record(host, 'flat.wav').dr}"
    code, out, _ = _run("--dr", "-q", "damaged.flac", "missing.wav")
    assert code == 1 and out.splitlines()[-1] == "album DR  none: no complete track"
    assert math.isfinite(_record(host, "damaged.flac").dr_mean)
