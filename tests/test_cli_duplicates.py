"""`--duplicates` of the command line (mp3rgain_amd/cli.py) without a GPU: option parsing, its errors and its conflicts, and the
text, TSV and JSON shapes on records, pairs and groups the host routes compute (rg_fingerprint_arena route 2,
rg_fingerprint_match_codes route 0, rg_fingerprint_groups), handed to the command in place of the GPU's."""
import io
import json
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import fingerprint_cases as fc  # noqa: E402

from mp3rgain_amd import cli  # noqa: E402
from mp3rgain_amd import replaygain as rg  # noqa: E402

_capi = rg._capi


def _run(*args):
    out, err = io.StringIO(), io.StringIO()
    code = cli.main([str(a) for a in args], out, err)
    return code, out.getvalue(), err.getvalue()


def test_option_parsing_errors_and_conflicts():
    o = cli.parse_args(["--duplicates", "--dup-radius", "2.5", "--dup-ber", "200", "-o", "json", "a.wav", "b.flac"], io.StringIO(), io.StringIO())
    assert (o.duplicates, o.dup_radius, o.dup_ber, o.output_format, [str(f) for f in o.files]) == (True, 2.5, 200, "json", ["a.wav", "b.flac"])
    assert cli.dup_radius_codes(2.5) == 215 and cli.dup_radius_codes(5.944) == 512
    for args, text in ((["--dup-radius", "5", "a.wav"], "--dup-radius requires --duplicates"),
                       (["--dup-ber", "5", "a.wav"], "--dup-ber requires --duplicates"),
                       (["--duplicates", "--dup-ber", "0", "a.wav"], "1 to 1000"), (["--duplicates", "--dup-ber", "1001", "a.wav"], "1 to 1000"),
                       (["--duplicates", "--dup-ber", "x", "a.wav"], "invalid per mille value: x"),
                       (["--duplicates", "--dup-radius", "0", "a.wav"], "invalid radius: 0"),
                       (["--duplicates", "--dup-radius", "0.001", "a.wav"], "--dup-radius takes"),
                       (["--duplicates", "--dup-radius", "24", "a.wav"], "--dup-radius takes"),
                       (["--duplicates", "--stats", "a.wav"], "cannot be combined with --stats"), (["--spectrum", "--duplicates", "a.wav"], "--spectrum"),
                       (["--duplicates", "--dr", "a.wav"], "--dr"), (["--duplicates", "--verify", "a.wav"], "--verify"),
                       (["--duplicates", "--rip", "a.wav"], "--rip"), (["--duplicates", "--ancestry", "a.wav"], "--ancestry"),
                       (["--duplicates", "--r128", "a.wav"], "--r128"), (["--duplicates", "-r", "a.wav"], "-r"), (["--duplicates", "-a", "a.wav"], "-a"),
                       (["--duplicates", "-x", "a.wav"], "-x"), (["--duplicates", "-g", "2", "a.wav"], "-g")):
        with pytest.raises(cli.CliError) as e:
            cli.parse_args(args, io.StringIO(), io.StringIO())
        assert text in str(e.value), args
        code, _, err = _run(*args)
        assert code == 1 and text in err
    code, _, err = _run("--duplicates", "--dup-radius")
    assert code == 1 and "--dup-radius requires an argument" in err
    code, _, err = _run("--duplicates")
    assert code == 1 and "no files specified" in err
    out = io.StringIO()
    cli.print_usage(out)
    for field in ("--duplicates ", "--dup-radius <seconds>", "--dup-ber <permille>", "lag_seconds", "no other fingerprint", "synthetic material",
                  f"default {_capi.FP_MAX_BER_PERMILLE})"):
        assert field in out.getvalue(), field


class _HostAnalyzer:
    """Analyzer.same_recording from the host routes: the named planes instead of files."""
    planes = {}
    seen = []

    def __init__(self, device=0):
        pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        return False

    def same_recording(self, files, block=None, probes=None, radius=None, max_ber_permille=None):
        type(self).seen.append((block, probes, radius, max_ber_permille))
        known = [f for f in files if str(f) in self.planes]
        tracks = [rg.PcmTrack(self.planes[str(f)][0], self.planes[str(f)][1]) for f in known]
        arena, descs = rg.pack_tracks(tracks)
        recs, codes, _ = rg.fingerprint_arena(None, 2, list(descs)[:len(known)], arena, bands=False)
        pair_records = rg.fingerprint_match_codes(None, 0, [codes[r.codes_at:r.codes_at + r.codes] for r in recs], [r.sample_rate for r in recs],
                                                  block, probes, radius, max_ber_permille)
        groups, matches, _ = rg.fingerprint_groups(len(known), pair_records)
        index = [k for k, f in enumerate(files) if str(f) in self.planes]  # of the known files among all
        out = []
        for k, f in enumerate(files):
            if str(f) not in self.planes:
                out.append(rg.fingerprint_from_record(_capi.FingerprintRecord(status=-8), rg.ReplayGainError(-8, f"Failed to open: {f}")))
                continue
            q = index.index(k)
            rec = recs[q]
            rec.group, rec.matches, rec.dropped_frames = index[int(groups[q])], int(matches[q]), self.planes[str(f)][2]
            if rec.dropped_frames:
                rec.flags &= ~_capi.FP_COMPLETE
            out.append(rg.fingerprint_from_record(rec))
        pairs, rec_at = [], 0
        for a in range(len(known)):
            for b in range(a + 1, len(known)):
                r = pair_records[rec_at]
                rec_at += 1
                if r["flags"] & _capi.FP_PAIR_MATCH:
                    pairs.append(rg.SamePair(index[a], index[b], int(r["errors"]), int(r["bits"]), int(r["lag"]), int(r["flags"])))
        by = {}
        for k, r in enumerate(out):
            if r.error is None:
                by.setdefault(r.group, []).append(k)
        return out, pairs, [g for _, g in sorted(by.items()) if len(g) > 1]


N = fc.L + 300 * fc.H  # 300 codes: enough for the default block of 256


@pytest.fixture()
def host(capi, monkeypatch):
    x, y = fc.noise(N + 5 * fc.H, 700), fc.noise(N, 701)
    rng = np.random.default_rng(702)
    late = np.concatenate([np.zeros(3 * fc.H), x])[:N] * 0.5 + rng.standard_normal(N) * 30.0  # three codes late, quieter, noisy
    _HostAnalyzer.planes = {"one.flac": ([fc.as_format(x[:N], "s16")], 44100, 0), "other.wav": ([fc.as_format(y, "s16")], 44100, 0),
                            "one_again.wav": ([fc.as_format(late, "f32"), fc.as_format(late, "f32")], 44100, 0),
                            "one_cut.flac": ([fc.as_format(x[2 * fc.H:2 * fc.H + N], "s32")], 44100, 2),
                            "short.wav": ([fc.as_format(y[:4500], "s16")], 44100, 0), "hires.wav": ([fc.as_format(y, "s32")], 96000, 0)}
    _HostAnalyzer.seen = []
    monkeypatch.setattr(cli.rgmod, "Analyzer", _HostAnalyzer)
    return _HostAnalyzer


def test_text_a_paragraph_per_group_and_the_closing_line(host):
    code, out, err = _run("--duplicates", "one.flac", "other.wav", "one_again.wav")
    lines = out.splitlines()
    assert code == 0 and err == ""
    assert lines[0].startswith("mp3rgain duplicate search among 3 file(s)") and "no other fingerprint" in lines[0] and lines[1] == ""
    recs, pairs, groups = host().same_recording(["one.flac", "other.wav", "one_again.wav"])
    assert groups == [[0, 2]] and len(pairs) == 1 and (pairs[0].i, pairs[0].j, pairs[0].lag_of_j) == (0, 2, 3)
    assert lines[2:] == ["group 1: 2 files", "    one.flac", f"    one_again.wav   {3 * 512 / 44100:+.3f} s   {100 * pairs[0].ber:.1f} % of bits differ", "",
                         "3 files, 1 groups of duplicates"]
    assert 0.0 < pairs[0].ber < 0.2
    code, out, _ = _run("--duplicates", "-q", "other.wav", "short.wav", "hires.wav")
    assert code == 0 and out.splitlines() == ["3 files, 0 groups of duplicates"]
    code, out, _ = _run("--duplicates", "other.wav", "short.wav", "hires.wav")
    assert code == 0 and out.splitlines()[2:] == ["short.wav  [short]", "hires.wav  [rate]", "3 files, 0 groups of duplicates"]


def test_the_options_reach_the_analyzer(host):
    code, out, _ = _run("--duplicates", "--dup-radius", "0.02", "--dup-ber", "150", "-q", "one.flac", "one_again.wav", "one_cut.flac")
    assert (None, None, 2, 150) in host.seen
    # radius 2 codes: the copy 3 codes late is out of reach, the one 2 codes early is found
    assert code == 1 and out.splitlines()[-1] == "3 files, 1 groups of duplicates" and "    one_cut.flac   -0.023 s   0.0 % of bits differ" in out.splitlines()
    _run("--duplicates", "-q", "one.flac", "other.wav")
    assert host.seen[-1] == (None, None, None, None)


def test_tsv_and_json(host):
    files = ["one.flac", "other.wav", "one_again.wav", "one_cut.flac"]
    recs, pairs, groups = host().same_recording(files)
    assert groups == [[0, 2, 3]] and [(p.i, p.j) for p in pairs] == [(0, 2), (0, 3), (2, 3)]
    code, out, _ = _run("--duplicates", "-o", "tsv", *files)
    rows = [line.split("\t") for line in out.splitlines()]
    assert code == 1 and len(rows) == 7  # one_cut.flac has dropped frames
    assert rows[0] == ["one.flac", "0", "ok", "300", "2", str(N), "44100", "0"] and rows[1][:5] == ["other.wav", "1", "ok", "300", "0"]
    assert rows[3] == ["one_cut.flac", "0", "incomplete", "300", "2", str(N), "44100", "2"]
    p = pairs[1]
    assert rows[5] == ["pair", "one.flac", "one_cut.flac", f"{-2 * 512 / 44100:.3f}", str(p.errors), str(p.bits), f"{1000 * p.ber:.1f}"]
    assert rows[6][:4] == ["pair", "one_again.wav", "one_cut.flac", f"{-5 * 512 / 44100:.3f}"]
    code, out, _ = _run("--duplicates", "-o", "json", *files[:3])
    d = json.loads(out)
    assert code == 0 and d["summary"] == {"total_files": 3, "successful": 3, "failed": 0}
    f = d["files"][2]
    assert (f["file"], f["status"], f["verdicts"], f["group"], f["matches"], f["codes"], f["frames"], f["sample_rate"], f["channels"], f["complete"]) == \
        ("one_again.wav", "success", ["ok"], 0, 1, 300, N, 44100, 2, True)
    p = pairs[0]
    assert d["pairs"] == [{"i": 0, "j": 2, "lag_codes": 3, "lag_seconds": 3 * 512 / 44100, "errors": p.errors, "bits": p.bits, "ber": p.ber}]
    assert d["groups"] == [["one.flac", "one_again.wav"]]


def test_exit_status_and_failing_files(host):
    code, out, err = _run("--duplicates", "-q", "one.flac", "missing.wav", "one_again.wav")
    assert code == 1 and "missing.wav - Failed to open: missing.wav" in err
    assert out.splitlines()[0] == "group 1: 2 files" and out.splitlines()[-1] == "3 files, 1 groups of duplicates"
    code, out, _ = _run("--duplicates", "-o", "json", "other.wav", "missing.wav")
    d = json.loads(out)
    assert code == 1 and d["summary"] == {"total_files": 2, "successful": 1, "failed": 1}
    assert d["files"][1] == {"file": "missing.wav", "status": "error", "error": "Failed to open: missing.wav"} and d["groups"] == [] and d["pairs"] == []
    code, out, _ = _run("--duplicates", "-o", "tsv", "missing.wav")
    assert code == 1 and out.splitlines() == ["missing.wav\tFailed to open: missing.wav"]
