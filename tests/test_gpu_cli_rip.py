"""`--rip` and `--rip-log` of the command line (mp3rgain_amd/cli.py) on the GPU: one row per file as text, TSV and JSON, and the
verdicts and exit statuses against rip logs the test writes itself from the Python restatement (tests/rip_cases.py)."""
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


def _run(*args):
    from mp3rgain_amd import cli

    out, err = io.StringIO(), io.StringIO()
    rc_ = cli.main([str(a) for a in args], out, err)
    return rc_, out.getvalue(), err.getvalue()


@pytest.fixture(scope="module")
def disc(tmp_path_factory):
    tmp = tmp_path_factory.mktemp("cli_rip")
    rng = np.random.default_rng(41)
    files, wants = [], []
    lens = (588 * 10, 3000 + 77)
    for k, n in enumerate(lens):
        pcm = flacenc.test_pcm(rng, 2, n, 16)
        pcm[1, 10:30] = 0
        p = tmp / (f"{k + 1:02d}.flac" if k == 0 else f"{k + 1:02d}.wav")
        p.write_bytes(flacenc.encode(pcm, 44100, 16, flacenc.Options(block_size=1152)) if k == 0 else wav_bytes([pcm[0], pcm[1]], 44100, "s16"))
        files.append(p)
        wants.append(rc.want(pcm[0], pcm[1], (rc.FIRST if k == 0 else 0) | (rc.LAST if k == len(lens) - 1 else 0)))
    return tmp, files, wants, lens


def test_rip_text_tsv_json(disc):
    tmp, files, wants, lens = disc
    code, out, err = _run("--rip", *files)
    assert code == 0 and "Rip checksums of 2 file(s)" in out
    for f, w in zip(files, wants):
        assert f"{f.name} - CRC32 {w.crc32:08X}  w/o null {w.crc32_nonnull:08X}  ARv1 {w.arv1:08X}  ARv2 {w.arv2:08X}" in out
    assert "not a whole number of sectors" in out.splitlines()[-1] and "sectors" not in out.splitlines()[-2]
    code, out, _ = _run("--rip", "-o", "tsv", *files)
    assert code == 0 and out.splitlines() == [f"{f.name}\tok\t{n}\t{w.null_samples}\t{w.crc32:08X}\t{w.crc32_nonnull:08X}\t{w.arv1:08X}\t{w.arv2:08X}"
                                              for f, n, w in zip(files, lens, wants)]
    code, out, _ = _run("--rip", "-o", "json", files[0], tmp / "missing.wav", files[1])  # a failing file between the disc's first and last
    assert code == 1
    d = json.loads(out)
    assert d["summary"] == {"total_files": 3, "successful": 2, "failed": 1}
    for k, (j, w, n) in enumerate(zip(d["files"][0::2], wants, lens)):
        assert j["status"] == "success" and (j["frames"], j["sample_rate"], j["null_samples"], j["dropped_frames"]) == (n, 44100, w.null_samples, 0)
        assert (j["crc32"], j["crc32_nonnull"], j["arv1"], j["arv2"]) == tuple(f"{x:08X}" for x in (w.crc32, w.crc32_nonnull, w.arv1, w.arv2))
        assert j["first_track"] == (k == 0) and j["last_track"] == (k == 1) and j["cd_rate"] and j["complete"] and j["cd_frames"] == (n % 588 == 0)
        assert "log" not in j
    assert d["files"][1]["status"] == "error" and "Failed to open" in d["files"][1]["error"]


def _log(wants, copy_crc):
    out = "XLD extraction logfile\n\n"
    for k, w in enumerate(wants):
        out += f"Track {k + 1:02d}\n"
        if copy_crc:
            out += f"     Copy CRC {w.crc32_nonnull if k else w.crc32:08X}\n"
        else:
            out += (f"    CRC32 hash               : {w.crc32:08X}\n    CRC32 hash (skip zero)   : {w.crc32_nonnull:08X}\n"
                    f"    AccurateRip v1 signature : {w.arv1:08X}\n    AccurateRip v2 signature : {w.arv2:08X}\n")
    return out


def test_rip_log_verdicts_and_exit_statuses(disc):
    tmp, files, wants, lens = disc
    good = tmp / "good.log"
    good.write_text(_log(wants, False))
    code, out, err = _run("--rip", "--rip-log", good, *files)
    assert code == 0 and out.count("log: match") == 2 and "mismatch" not in out
    eac = tmp / "eac.log"
    eac.write_bytes(b"\xff\xfe" + _log(wants, True).encode("utf-16-le"))
    code, out, _ = _run("--rip", "--rip-log", eac, "-o", "tsv", *files)
    assert code == 0 and [line.split("\t")[-1] for line in out.splitlines()] == ["match", "match"]
    bad = tmp / "bad.log"
    bad.write_text(_log([wants[0], wants[1]._replace(arv2=wants[1].arv2 ^ 0x100)], False))
    code, out, _ = _run("--rip", "--rip-log", bad, "-o", "json", *files)
    d = json.loads(out)
    assert code == 1 and [f["log"] for f in d["files"]] == ["match", "mismatch: AccurateRip v2"]
    assert d["summary"] == {"total_files": 2, "successful": 1, "failed": 1}
    assert [c["ok"] for c in d["files"][1]["log_checks"]] == [True, True, True, False]
    short = tmp / "short.log"
    short.write_text(_log(wants[:1], False))
    code, out, err = _run("--rip", "--rip-log", short, *files)
    assert code == 1 and "1 track section(s) for 2 file(s)" in err and "log: match" in out and "no log section" in out
    code, out, err = _run("--rip", "--rip-log", tmp / "nowhere.log", *files)
    assert code == 1 and "cannot read" in err
    code, out, err = _run("--rip-log", good, *files)
    assert code != 0 and "--rip-log requires --rip" in err
