"""The host side of the rip checksums (rg_rip_host.cpp with rg_rip.h and rg_crc32.h, the headers the kernels share) under
AddressSanitizer + UndefinedBehaviorSanitizer: built with gcc's sanitizers and a small stand-alone driver with its own main,
which runs the serial twin (route 0) and the kernels' fold arithmetic (route 2) on a handful of the shared cases, each in an
exact-size heap arena.  Run on the CPU as a child process; nothing is loaded into Python."""
import shutil
import struct
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))
import rip_cases as rc  # noqa: E402


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
    out = tmp / "rip_driver"
    cmd = ["g++", "-std=c++17", "-O1", "-g"] + san + [f"-I{ROOT / 'include'}", str(ROOT / "tests" / "san" / "rip_driver.cpp"),
                                                       str(ROOT / "mp3rgain_amd" / "csrc" / "rg_rip_host.cpp"), "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return out


def test_rip_host_routes_under_asan_ubsan(driver, tmp_path):
    c, t, f = rc.shape()
    pick = {0, 1, c + 1, t - 1, t + 1, 2941, 5881, 3 * t + c + 1}
    chosen = [cs for cs in rc.cases() if len(cs.left) in pick and cs.name.split("_")[0] in ("random", "sparse", "ffff", "zero", "one")]
    assert len(chosen) >= 20
    files, want = [], []
    for k, cs in enumerate(chosen):
        fl = rc.ALL_FLAGS[k % 4]
        p = tmp_path / f"{k:03d}.bin"
        p.write_bytes(struct.pack("<QI", len(cs.left), fl) + np.ascontiguousarray(cs.left, "<i2").tobytes() + np.ascontiguousarray(cs.right, "<i2").tobytes())
        files.append(str(p))
        want.append(rc.wants()[(cs.name, fl)])
    r = subprocess.run([str(driver)] + files, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = r.stdout.split("\n")[:-1]
    assert len(lines) == 2 * len(files)
    for k, w in enumerate(want):
        for line in lines[2 * k:2 * k + 2]:
            name, route, crc, nn, nulls, v1, v2 = line.split(" ")
            assert name == files[k]
            assert rc.Want(int(crc, 16), int(nn, 16), int(nulls), int(v1, 16), int(v2, 16)) == w, (chosen[k].name, route)
