"""The host side of the PCM defect scan (rg_stats_host.cpp with rg_stats.h, the header the kernels share) under
AddressSanitizer + UndefinedBehaviorSanitizer: built with gcc's sanitizers and a small stand-alone driver with its own main,
which runs the serial twin (route 0) and the kernels' chunking and fold arithmetic (route 2) on a handful of the shared cases,
each in an exact-size heap arena.  Run on the CPU as a child process; nothing is loaded into Python."""
import shutil
import struct
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))
import arena_layouts as al  # noqa: E402
import pcm_stats_cases as pc  # noqa: E402


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    tmp = tmp_path_factory.mktemp("san")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    # does this toolchain have the sanitizers' runtimes at all?  A trivial program of the test's own says so; after that a
    # failing build of the project's sources is a failure, whatever its diagnostics mention
    probe = tmp / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    r = subprocess.run(["g++"] + san + [str(probe), "-o", str(tmp / "probe")], capture_output=True, text=True)
    if r.returncode != 0 or subprocess.run([str(tmp / "probe")], capture_output=True).returncode != 0:
        pytest.skip("this toolchain has no sanitizer runtime")
    out = tmp / "pcm_stats_driver"
    cmd = ["g++", "-std=c++17", "-O1", "-g"] + san + [f"-I{ROOT / 'include'}", str(ROOT / "tests" / "san" / "pcm_stats_driver.cpp"),
                                                       str(ROOT / "mp3rgain_amd" / "csrc" / "rg_stats_host.cpp"), "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return out


def test_pcm_stats_host_routes_under_asan_ubsan(driver, tmp_path):
    c, t, f = pc.shape()
    pick = {0, 1, c + 1, t - 1, t + 1, 3 * t + c + 1}
    kinds = ("random", "zero_", "pos_fs", "clip_three", "zero_lengths", "pos_neg", "special", "6ch", "padded16")
    chosen = [tr for tr in pc.tracks() if len(tr.channels[0]) in pick and any(k in tr.name for k in kinds)]
    chosen = chosen[::max(1, len(chosen) // 24)]
    assert len(chosen) >= 20 and {tr.channels[0].dtype for tr in chosen} == {np.dtype(np.int16), np.dtype(np.int32), np.dtype(np.float32)}
    files, want = [], []
    for k, tr in enumerate(chosen):
        opts = pc.OPTIONS[k % 3]
        p = tmp_path / f"{k:03d}.bin"
        dt = tr.channels[0].dtype
        p.write_bytes(struct.pack("<Q5I", len(tr.channels[0]), len(tr.channels), al.FMT[dt], tr.bits, *opts)
                      + b"".join(np.ascontiguousarray(ch, dt.newbyteorder("<")).tobytes() for ch in tr.channels))
        files.append(str(p))
        want.append(pc.wants(opts)[tr.name])
    r = subprocess.run([str(driver)] + files, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln.split(" ") for ln in r.stdout.split("\n")[:-1]]
    assert len(lines) == 2 * sum(w["channels"] for w in want)
    at = 0
    for k, w in enumerate(want):
        for route in (0, 2):
            for c_, wc in enumerate(w["ch"]):
                name, rt, ch, flags, mn, mx, *ints = lines[at]
                at += 1
                assert (name, int(rt), int(ch), int(flags)) == (files[k], route, c_, w["flags"]), chosen[k].name
                assert (float.fromhex(mn), float.fromhex(mx)) == (wc["min"], wc["max"]), chosen[k].name
                assert [int(v) for v in ints] == [wc[f_] for f_ in pc.CHANNEL_FIELDS[2:]], (chosen[k].name, route, c_)
