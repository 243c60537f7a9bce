"""`--spectrum` of the command line (mp3rgain_amd/cli.py) without a GPU: option parsing and its errors, and the text, TSV and
JSON shapes on records the host routes (rg_spectrum_arena, route 2) compute, handed to the command in place of the GPU's."""
import io
import json
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import spectrum_cases as sc  # noqa: E402

from mp3rgain_amd import cli  # noqa: E402
from mp3rgain_amd import replaygain as rg  # noqa: E402


def _run(*args):
    out, err = io.StringIO(), io.StringIO()
    code = cli.main([str(a) for a in args], out, err)
    return code, out.getvalue(), err.getvalue()


def test_option_parsing_and_its_errors():
    o = cli.parse_args(["--spectrum", "--edge-db", "40", "--min-cutoff", "8000.5", "-o", "json", "a.wav", "b.flac"], io.StringIO(), io.StringIO())
    assert (o.spectrum, o.edge_db, o.min_cutoff, o.output_format, [str(f) for f in o.files]) == (True, 40.0, 8000.5, "json", ["a.wav", "b.flac"])
    o = cli.parse_args(["--spectrum", "a.wav"], io.StringIO(), io.StringIO())
    assert (o.spectrum, o.edge_db, o.min_cutoff) == (True, None, None)
    for args, text in ((["--edge-db", "5", "a.wav"], "--edge-db requires --spectrum"), (["--min-cutoff", "5", "a.wav"], "--min-cutoff requires --spectrum"),
                       (["--spectrum", "--edge-db", "0", "a.wav"], "invalid edge depth: 0"), (["--spectrum", "--min-cutoff", "-4", "a.wav"], "invalid frequency: -4"),
                       (["--spectrum", "--edge-db", "x", "a.wav"], "invalid edge depth: x"), (["--spectrum", "--min-cutoff", "inf", "a.wav"], "invalid frequency: inf"),
                       (["--spectrum", "--edge-db", "nan", "a.wav"], "invalid edge depth: nan")):
        with pytest.raises(cli.CliError) as e:
            cli.parse_args(args, io.StringIO(), io.StringIO())
        assert text in str(e.value), args
        code, _, err = _run(*args)
        assert code == 1 and text in err
    code, _, err = _run("--spectrum", "--edge-db")
    assert code == 1 and "--edge-db requires an argument" in err
    code, _, err = _run("--spectrum")
    assert code == 1 and "no files specified" in err
    out = io.StringIO()
    cli.print_usage(out)
    assert "--spectrum " in out.getvalue() and "--edge-db <dB>" in out.getvalue() and "--min-cutoff <Hz>" in out.getvalue()


class _HostAnalyzer:
    """Analyzer.spectrum from the host route: the named planes instead of files."""
    planes = {}
    seen = []

    def __init__(self, device=0):
        pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False

    def spectrum(self, files, edge_db=None, min_cutoff_hz=None, bands=False):
        type(self).seen.append((edge_db, min_cutoff_hz, bands))
        res = []
        for f in files:
            if str(f) not in self.planes:
                res.append(rg.spectrum_from_record(rg._capi.SpectrumRecord(status=-8), rg.ReplayGainError(-8, f"Failed to open: {f}")))
                continue
            chans, rate, dropped = self.planes[str(f)]
            arena, descs = rg.pack_tracks([rg.PcmTrack(chans, rate)])
            recs, e = rg.spectrum_arena(None, 2, list(descs)[:1], arena, edge_db, min_cutoff_hz)
            rec = recs[0]
            rec.dropped_frames = dropped
            if dropped:
                rec.flags &= ~rg._capi.SPEC_COMPLETE
            res.append(rg.spectrum_from_record(rec, None, e[0] if bands else None))
        return res


@pytest.fixture()
def host(capi, monkeypatch):
    cut, _ = sc.verdict_signal("white-16k")
    up, _ = sc.verdict_signal("pink-up96k")
    white, _ = sc.verdict_signal("white")
    nan = white.astype(np.float32)
    nan[5000] = np.nan
    _HostAnalyzer.planes = {"cut.flac": ([sc.as_s16(cut), sc.as_s16(white)], 44100, 0), "up.flac": ([sc.as_s24(up)], 96000, 0),
                            "white.wav": ([sc.as_s16(white)], 44100, 0), "damaged.flac": ([sc.as_s16(white)], 44100, 2),
                            "short.wav": ([np.zeros(100, np.int16)], 44100, 0), "nan.wav": ([nan], 44100, 0)}
    _HostAnalyzer.seen = []
    monkeypatch.setattr(cli.rgmod, "Analyzer", _HostAnalyzer)
    return _HostAnalyzer


def _records(host, name):
    """The Spectrum the command is handed for `name`, to derive the expected numbers from."""
    return host().spectrum([name])[0]


def test_text_one_line_of_words_and_one_per_channel(host):
    cut, up = _records(host, "cut.flac"), _records(host, "up.flac")
    host.seen.clear()
    code, out, err = _run("--spectrum", "white.wav", "cut.flac", "up.flac", "short.wav", "nan.wav")
    assert code == 0 and err == "" and host.seen == [(None, None, False)]  # findings are a report, not a failure
    lines = out.splitlines()
    assert lines[0] == "mp3rgain spectrum of 5 file(s): edges of at least 30 dB above 4000 Hz" and lines[1] == ""
    assert lines[2:5] == ["white.wav - ok  [44100 Hz]", "    no cutoff below Nyquist", "    ch 0: cutoff 22050 Hz  edge 0.0 dB  frames 40  ok"]
    # only the first channel is cut off (the second is white noise): the words name it and give its edge, not the record's
    # cutoff_hz, which is the maximum over the channels and so Nyquist
    c0 = cut.channels[0]
    assert c0.bandlimited and not cut.channels[1].bandlimited and cut.cutoff_hz == 22050.0 and abs(c0.cutoff_hz - 16200.0) <= 172.3 and c0.edge_db >= 30.0
    assert lines[5] == "cut.flac - bandlimited  [44100 Hz]"
    assert lines[6] == f"    cut off at {c0.cutoff_hz / 1000:.1f} kHz, edge {c0.edge_db:.0f} dB (channel 0 of 2)"
    assert lines[7] == f"    ch 0: cutoff {c0.cutoff_hz:.0f} Hz  edge {c0.edge_db:.1f} dB  frames 40  bandlimited"
    assert lines[8] == "    ch 1: cutoff 22050 Hz  edge 0.0 dB  frames 40  ok"
    u0 = up.channels[0]
    assert u0.upsampled and 21900.0 <= u0.cutoff_hz <= 22800.0
    assert lines[9] == "up.flac - bandlimited, upsampled  [96000 Hz]"
    assert lines[10] == f"    96 kHz file with nothing above {u0.cutoff_hz / 1000:.1f} kHz"
    assert lines[11].endswith("bandlimited,upsampled")
    assert lines[12:14] == ["short.wav - short  [44100 Hz]", "    too short to analyse"]
    assert lines[15] == "nan.wav - nonfinite  [44100 Hz]" and "frames 38 (+2 skipped)" in lines[17]
    code, out, _ = _run("--spectrum", "--edge-db", "70", "--min-cutoff", "5000", "-q", "cut.flac")
    assert code == 0 and host.seen[-1] == (70.0, 5000.0, False) and out == ""  # quiet


def test_words_of_files_cut_in_every_channel_and_in_some(host):
    planes = host.planes["cut.flac"][0]
    host.planes["mono-cut.flac"] = (planes[:1], 44100, 0)
    host.planes["cut-1-2.flac"] = ([planes[1], planes[0], planes[0]], 44100, 0)
    c0 = _records(host, "mono-cut.flac").channels[0]
    want = f"cut off at {c0.cutoff_hz / 1000:.1f} kHz, edge {c0.edge_db:.0f} dB"
    code, out, _ = _run("--spectrum", "mono-cut.flac", "cut-1-2.flac")
    lines = out.splitlines()
    assert code == 0 and lines[3] == "    " + want and lines[6] == "    " + want + " (channels 1, 2 of 3)"
    r = _records(host, "cut-1-2.flac")
    assert (r.cut_channels, r.lowest_cut.cutoff_hz, r.edge_db, r.cutoff_hz) == ([1, 2], c0.cutoff_hz, c0.edge_db, 22050.0)
    assert _records(host, "white.wav").lowest_cut is None and _records(host, "white.wav").edge_db == 0.0


def test_tsv_and_json_shapes(host):
    code, out, _ = _run("--spectrum", "-o", "tsv", "cut.flac", "up.flac")
    rows = [line.split("\t") for line in out.splitlines()]
    assert code == 0 and [len(r) for r in rows] == [8, 8, 8, 8, 8]
    c0 = _records(host, "cut.flac").channels[0]
    assert rows[0] == ["cut.flac", "bandlimited", "22050.0", f"{c0.edge_db:.1f}", str(sc.L + 39 * sc.H + 37), "44100", "2", "0"]
    assert rows[1] == ["cut.flac", "ch", "0", f"{c0.cutoff_hz:.1f}", f"{c0.edge_db:.1f}", "40", "0", "bandlimited"] and rows[2][7] == "ok"
    assert rows[3][1] == "bandlimited,upsampled" and rows[4][7] == "bandlimited,upsampled"
    code, out, _ = _run("--spectrum", "-o", "json", "--edge-db", "35", "cut.flac", "short.wav")
    d = json.loads(out)
    assert code == 0 and d["summary"] == {"total_files": 2, "successful": 2, "failed": 0} and host.seen[-1] == (35.0, None, True)
    f0, f1 = d["files"]
    assert f0["status"] == "success" and f0["verdicts"] == ["bandlimited"] and (f0["sample_rate"], f0["dropped_frames"], f0["complete"]) == (44100, 0, True)
    c0, c1 = f0["channels"]
    want = _records(host, "cut.flac")
    assert c0["bandlimited"] and not c1["bandlimited"] and c0["cutoff_hz"] == want.channels[0].cutoff_hz and c0["analysed_frames"] == 40
    assert (f0["cutoff_hz"], f0["edge_db"], f0["summary"]) == (22050.0, want.edge_db, want.words) and "(channel 0 of 2)" in want.words
    assert len(c0["levels_db"]) == 256 and max(c0["levels_db"]) == 0.0 and c0["levels_db"][255] < -30.0 and c0["band_hz"] == 44100 * 8 / 4096
    assert f1["verdicts"] == ["short"] and f1["channels"][0]["levels_db"] == [None] * 256 and f1["summary"] == "too short to analyse"


def test_exit_status_is_1_only_for_a_failing_file_or_dropped_frames(host):
    code, out, err = _run("--spectrum", "cut.flac", "missing.wav")
    assert code == 1 and "missing.wav - Failed to open" in err and "cut.flac - bandlimited" in out
    code, out, _ = _run("--spectrum", "-o", "json", "white.wav", "missing.wav")
    d = json.loads(out)
    assert code == 1 and d["summary"]["failed"] == 1 and d["files"][1] == {"file": "missing.wav", "status": "error", "error": "Failed to open: missing.wav"}
    code, out, _ = _run("--spectrum", "-o", "tsv", "missing.wav")
    assert code == 1 and out == "missing.wav\tFailed to open: missing.wav\n"
    code, out, _ = _run("--spectrum", "-q", "damaged.flac", "white.wav")
    assert code == 1 and out.splitlines()[0] == "damaged.flac - incomplete  [44100 Hz, 2 frames dropped]" and "white.wav" not in out
