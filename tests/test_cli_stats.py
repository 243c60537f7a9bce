"""`--stats` of the command line (mp3rgain_amd/cli.py) without a GPU: option parsing and its errors, and the text, TSV and JSON
shapes on records the serial host twin (rg_pcm_stats_arena, route 0) computes, handed to the command in place of the GPU's."""
import io
import json
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))

from mp3rgain_amd import cli  # noqa: E402
from mp3rgain_amd import replaygain as rg  # noqa: E402


def _run(*args):
    out, err = io.StringIO(), io.StringIO()
    code = cli.main([str(a) for a in args], out, err)
    return code, out.getvalue(), err.getvalue()


def test_option_parsing_and_its_errors():
    o = cli.parse_args(["--stats", "--clip-run", "5", "--zero-run", "100", "-o", "json", "a.wav", "b.flac"], io.StringIO(), io.StringIO())
    assert (o.stats, o.clip_run, o.zero_run, o.output_format, [str(f) for f in o.files]) == (True, 5, 100, "json", ["a.wav", "b.flac"])
    o = cli.parse_args(["--stats", "a.wav"], io.StringIO(), io.StringIO())
    assert (o.stats, o.clip_run, o.zero_run) == (True, None, None)
    for args, text in ((["--clip-run", "5", "a.wav"], "--clip-run requires --stats"), (["--zero-run", "5", "a.wav"], "--zero-run requires --stats"),
                       (["--stats", "--clip-run", "0", "a.wav"], "at least 1"), (["--stats", "--zero-run", "0", "a.wav"], "at least 1"),
                       (["--stats", "--clip-run", "x", "a.wav"], "invalid run length: x"), (["--stats", "--zero-run", "-4", "a.wav"], "invalid run length: -4")):
        with pytest.raises(cli.CliError) as e:
            cli.parse_args(args, io.StringIO(), io.StringIO())
        assert text in str(e.value), args
        code, _, err = _run(*args)
        assert code == 1 and text in err
    code, _, err = _run("--stats", "--clip-run")
    assert code == 1 and "--clip-run requires an argument" in err
    code, _, err = _run("--stats")
    assert code == 1 and "no files specified" in err
    out = io.StringIO()
    cli.print_usage(out)
    assert "--stats " in out.getvalue() and "--clip-run <n>" in out.getvalue() and "--zero-run <n>" in out.getvalue()


class _HostAnalyzer:
    """Analyzer.pcm_stats from the serial host twin: the named planes instead of files."""
    planes = {}
    seen = []

    def __init__(self, device=0):
        pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False

    def pcm_stats(self, files, min_clip_run=3, min_zero_run=64):
        type(self).seen.append((min_clip_run, min_zero_run))
        res = []
        for f in files:
            if str(f) not in self.planes:
                res.append(rg.pcm_stats_from_record(rg._capi.PcmStatsRecord(status=-8), rg.ReplayGainError(-8, f"Failed to open: {f}")))
                continue
            chans, rate, bits, dropped = self.planes[str(f)]
            arena, descs = rg.pack_tracks([rg.PcmTrack(chans, rate)])
            rec = rg.pcm_stats_arena(None, 0, list(descs)[:1], [bits], arena, min_clip_run, min_zero_run)[0]
            rec.dropped_frames = dropped
            if dropped:
                rec.flags &= ~rg._capi.STATS_COMPLETE
            res.append(rg.pcm_stats_from_record(rec))
        return res


@pytest.fixture()
def host(capi, monkeypatch):
    n = 48000
    left = ((np.arange(n) % 200 - 100) * 100 + 50).astype(np.int16)  # never zero, never full scale
    right = left.copy()
    left[24000:24004] = 32767       # a clip run half a second in
    right[:10] = 0
    left[:12] = 0
    right[30000:30100] = 0          # a dropout
    left[-5:] = 0
    right[-7:] = 0
    padded = [((np.arange(1000) % 50 - 25) * 2 + 1).astype(np.int32) << 16]
    _HostAnalyzer.planes = {"clip.wav": ([left, right], 48000, 16, 0), "padded.flac": (padded, 44100, 24, 0),
                            "damaged.flac": ([np.full(100, 5, np.int16)], 44100, 16, 2),
                            "hot.mp3": ([np.array([0.5, 1.25, 1.5, 1.0, -0.25], np.float32)], 44100, 32, 0)}
    _HostAnalyzer.seen = []
    monkeypatch.setattr(cli.rgmod, "Analyzer", _HostAnalyzer)
    return _HostAnalyzer


def test_text_one_line_per_file_and_channel(host):
    code, out, err = _run("--stats", "clip.wav", "padded.flac", "hot.mp3")
    assert code == 0 and err == "" and host.seen == [(3, 64)]  # findings are a report, not a failure
    lines = out.splitlines()
    assert lines[0] == "mp3rgain PCM stats of 3 file(s): clip runs from 3 samples, dropouts from 64" and lines[1] == ""
    assert lines[2] == "clip.wav - clipped, dropout  [16 of 16 bits, silence 10 + 5 frames]"
    assert lines[3].startswith("    ch 0: peak 0.999969  DC ") and "clipped 4 in 1 run(s) first at 0:00.500  dropouts 0" in lines[3]
    assert "clipped 0 in 0 run(s)  dropouts 1 (longest 100)" in lines[4] and "first at" not in lines[4]
    assert lines[5] == "padded.flac - padded  [16 of 24 bits, silence 0 + 0 frames]"
    assert lines[7] == "hot.mp3 - clipped  [float, silence 0 + 0 frames]" and "peak 1.500000" in lines[8] and "clipped 3 in 1 run(s) first at 0:00.000" in lines[8]
    assert len(lines) == 9
    code, out, _ = _run("--stats", "--clip-run", "5", "--zero-run", "101", "-q", "clip.wav")
    assert code == 0 and host.seen[-1] == (5, 101) and out == ""  # quiet, and nothing at these thresholds anyway


def test_tsv_and_json_shapes(host):
    code, out, _ = _run("--stats", "-o", "tsv", "clip.wav", "padded.flac")
    rows = [line.split("\t") for line in out.splitlines()]
    assert code == 0 and [len(r) for r in rows] == [10, 12, 12, 10, 12]
    assert rows[0] == ["clip.wav", "clipped,dropout", "48000", "48000", "2", "16", "16", "10", "5", "0"]
    assert rows[1][:3] == ["clip.wav", "ch", "0"] and rows[1][5:9] == ["4", "1", "4", "24000"] and rows[2][8] == "" and rows[2][10:] == ["1", "100"]
    assert rows[3][1] == "padded" and rows[3][5:7] == ["24", "16"]
    code, out, _ = _run("--stats", "-o", "json", "--zero-run", "50", "clip.wav", "hot.mp3")
    d = json.loads(out)
    assert code == 0 and d["summary"] == {"total_files": 2, "successful": 2, "failed": 0} and host.seen[-1] == (3, 50)
    f0, f1 = d["files"]
    assert f0["status"] == "success" and f0["verdicts"] == ["clipped", "dropout"] and (f0["frames"], f0["sample_rate"], f0["bits"], f0["effective_bits"]) == (48000, 48000, 16, 16)
    assert (f0["lead_silence_frames"], f0["trail_silence_frames"], f0["dropped_frames"], f0["clipped"], f0["padded"], f0["complete"]) == (10, 5, 0, True, False, True)
    assert len(f0["channels"]) == 2 and f0["channels"][0]["first_clip_run"] == 24000 and f0["channels"][1]["first_clip_run"] is None
    assert f0["channels"][1]["longest_zero_run"] == 100 and f0["channels"][0]["or_mask"] == "0000FFFF" and abs(f0["channels"][0]["dc_offset"]) < 0.01
    assert f1["float"] and f1["bits"] == 0 and f1["channels"][0]["max"] == 1.5 and f1["channels"][0]["clip_runs"] == 1


def test_exit_status_is_1_only_for_a_failing_file_or_dropped_frames(host):
    code, out, err = _run("--stats", "clip.wav", "missing.wav")
    assert code == 1 and "missing.wav - Failed to open" in err and "clip.wav - clipped" in out
    code, out, _ = _run("--stats", "-o", "json", "clip.wav", "missing.wav")
    d = json.loads(out)
    assert code == 1 and d["summary"]["failed"] == 1 and d["files"][1] == {"file": "missing.wav", "status": "error", "error": "Failed to open: missing.wav"}
    code, out, _ = _run("--stats", "-o", "tsv", "missing.wav")
    assert code == 1 and out == "missing.wav\tFailed to open: missing.wav\n"
    code, out, _ = _run("--stats", "-q", "damaged.flac", "padded.flac")
    assert code == 1 and out.splitlines()[0] == "damaged.flac - incomplete  [16 of 16 bits, silence 0 + 0 frames, 2 frames dropped]" and "padded.flac" not in out
