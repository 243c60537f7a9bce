"""`--rip-offsets` of the command line (mp3rgain_amd/cli.py) on the GPU: a rip of a disc against an XLD-shaped log the test writes
from the numbers of the same disc read 6 frames later -- offset +6, exit status 0, as text, TSV and JSON -- against a log of
unrelated numbers, and the unchanged output without the option."""
import io
import json
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import flacenc  # noqa: E402
import rip_cases as rc  # noqa: E402
from wavutil import wav_bytes  # noqa: E402

pytestmark = pytest.mark.gpu

SHIFT = 6


def _run(*args):
    from mp3rgain_amd import cli

    out, err = io.StringIO(), io.StringIO()
    rc_ = cli.main([str(a) for a in args], out, err)
    return rc_, out.getvalue(), err.getvalue()


def _log(wants):
    out = "XLD extraction logfile\n\n"
    for k, w in enumerate(wants):
        out += (f"Track {k + 1:02d}\n    CRC32 hash               : {w.crc32:08X}\n    CRC32 hash (skip zero)   : {w.crc32_nonnull:08X}\n"
                f"    AccurateRip v1 signature : {w.arv1:08X}\n    AccurateRip v2 signature : {w.arv2:08X}\n")
    return out


@pytest.fixture(scope="module")
def rips(tmp_path_factory):
    """Disc PCM D cut into rip A (files) at the track boundaries; rip B, the same boundaries in D read SHIFT frames later, is
    only restated: (directory, A's files, A's numbers, B's numbers)."""
    tmp = tmp_path_factory.mktemp("cli_rip_offsets")
    rng = np.random.default_rng(43)
    bounds = np.cumsum([0, 588 * 12, 3000 + 77, 588 * 9 + 5])
    pad = 16
    whole = flacenc.test_pcm(rng, 2, int(bounds[-1]) + 2 * pad, 16).astype(np.int16)
    files, wants = [], {0: [], SHIFT: []}
    for k in range(3):
        flags = (rc.FIRST if k == 0 else 0) | (rc.LAST if k == 2 else 0)
        for s in wants:
            cut = whole[:, pad + s + bounds[k]:pad + s + bounds[k + 1]]
            wants[s].append(rc.want(cut[0], cut[1], flags))
        cut = whole[:, pad + bounds[k]:pad + bounds[k + 1]]
        p = tmp / (f"{k + 1:02d}.flac" if k == 1 else f"{k + 1:02d}.wav")
        p.write_bytes(flacenc.encode(cut, 44100, 16, flacenc.Options(block_size=1152)) if k == 1 else wav_bytes([cut[0], cut[1]], 44100, "s16"))
        files.append(p)
    return tmp, files, wants[0], wants[SHIFT]


def test_a_log_of_the_disc_read_six_frames_later_matches_at_offset_plus_6(rips):
    tmp, files, own, later = rips
    log = tmp / "later.log"
    log.write_text(_log(later))
    code, out, err = _run("--rip", "--rip-log", log, *files)  # without the search: a mismatch
    assert code == 1 and out.count("mismatch") == 3
    code, out, err = _run("--rip", "--rip-offsets", "--rip-log", log, *files)
    assert code == 0, (out, err)
    assert out.count("log: match at offset +6; CRC-32 not comparable at offset +6") == 3 and "mismatch" not in out
    assert out.splitlines()[-1] == "log: offset +6 matches 6 signature(s) of 3 track(s)"
    for f, w in zip(files, own):  # the files' own numbers, as without the option
        assert f"{f.name} - CRC32 {w.crc32:08X}  w/o null {w.crc32_nonnull:08X}  ARv1 {w.arv1:08X}  ARv2 {w.arv2:08X}" in out
    code, out, _ = _run("--rip", "--rip-offsets", "--rip-log", log, "-o", "tsv", *files)
    rows = out.splitlines()
    assert code == 0 and len(rows) == 4 and rows[-1] == "offset\t6"
    assert [r.split("\t")[-1] for r in rows[:3]] == ["match at offset +6; CRC-32 not comparable at offset +6"] * 3
    code, out, _ = _run("--rip", "--rip-offsets", "--rip-log", log, "-o", "json", *files)
    d = json.loads(out)
    assert code == 0 and d["offset"] == 6 and d["summary"] == {"total_files": 3, "successful": 3, "failed": 0}
    for j, w in zip(d["files"], own):
        assert j["offset"] == 6 and (j["arv1"], j["arv2"], j["crc32"]) == (f"{w.arv1:08X}", f"{w.arv2:08X}", f"{w.crc32:08X}")
        assert [(c["name"], c["ok"], c["text"]) for c in j["log_checks"]] == [
            ("CRC32 hash", None, "not comparable at offset +6"), ("CRC32 hash (skip zero)", None, "not comparable at offset +6"),
            ("AccurateRip v1", True, "match at offset +6"), ("AccurateRip v2", True, "match at offset +6")]


def test_offset_zero_and_no_common_offset_are_todays_verdicts(rips):
    tmp, files, own, later = rips
    good = tmp / "own.log"
    good.write_text(_log(own))
    for fmt in ("text", "tsv", "json"):
        args = ["--rip", "--rip-log", good] + (["-o", fmt] if fmt != "text" else []) + files
        code0, out0, err0 = _run(*args)
        code1, out1, err1 = _run("--rip-offsets", *args)
        assert code0 == code1 == 0 and err0 == err1
        if fmt == "json":
            d0, d1 = json.loads(out0), json.loads(out1)
            assert d1.pop("offset") == 0 and "offset +0" in d1.pop("offset_search") and d0 == d1
        else:
            assert out1.splitlines()[:-1] == out0.splitlines()
            assert out1.splitlines()[-1] == ("offset\t0" if fmt == "tsv" else "log: offset +0 matches 6 signature(s) of 3 track(s)")
    # unrelated numbers: no common offset, the verdicts and the exit status of --rip --rip-log
    bad = tmp / "unrelated.log"
    bad.write_text(_log([w._replace(arv1=w.arv1 ^ 0x5A5A5A5A, arv2=(w.arv2 + 12345) & 0xFFFFFFFF) for w in own]))
    code0, out0, _ = _run("--rip", "--rip-log", bad, *files)
    code1, out1, _ = _run("--rip", "--rip-offsets", "--rip-log", bad, *files)
    assert code0 == code1 == 1 and out1.splitlines()[:-1] == out0.splitlines() and "no common offset" in out1.splitlines()[-1]
    assert out1.count("log: mismatch: AccurateRip v1, AccurateRip v2") == 3
    d = json.loads(_run("--rip", "--rip-offsets", "--rip-log", bad, "-o", "json", *files)[1])
    assert d["offset"] is None and d["summary"]["failed"] == 3
