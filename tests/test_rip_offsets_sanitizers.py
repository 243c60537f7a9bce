"""The host side of the AccurateRip signatures at every drive offset (rg_rip_host.cpp with rg_rip.h, the header the kernel
shares) under AddressSanitizer + UndefinedBehaviorSanitizer: built with gcc's sanitizers and a small stand-alone driver with
its own main, which runs the definition (route 0) and the sliding recurrence (route 2) on discs whose halos leave the disc on
both sides, in an exact-size heap arena.  Run on the CPU as a child process; nothing is loaded into Python."""
import shutil
import struct
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))
import rip_offset_cases as oc  # noqa: E402


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    tmp = tmp_path_factory.mktemp("san_offsets")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    # does this toolchain have the sanitizers' runtimes at all?  A trivial program of the test's own says so; after that a
    # failing build of the project's sources is a failure, whatever its diagnostics mention
    probe = tmp / "probe.cpp"
    probe.write_text("int main() { return 0; }\n")
    r = subprocess.run(["g++"] + san + [str(probe), "-o", str(tmp / "probe")], capture_output=True, text=True)
    if r.returncode != 0 or subprocess.run([str(tmp / "probe")], capture_output=True).returncode != 0:
        pytest.skip("this toolchain has no sanitizer runtime")
    out = tmp / "rip_offsets_driver"
    cmd = ["g++", "-std=c++17", "-O1", "-g"] + san + [f"-I{ROOT / 'include'}", str(ROOT / "tests" / "san" / "rip_offsets_driver.cpp"),
                                                       str(ROOT / "mp3rgain_amd" / "csrc" / "rg_rip_host.cpp"), "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return out


@pytest.mark.parametrize("name,radius", [("short", oc.RADIUS_MAX), ("mixed_a", 300), ("impulses", oc.RADIUS_MAX), ("single_empty", 40)])
def test_rip_offsets_host_routes_under_asan_ubsan(driver, tmp_path, name, radius):
    """`short` is shorter than the radius and unflagged: every halo leaves the disc on both sides."""
    disc = next(d for d in oc.discs() if d.name == name)
    blob = struct.pack("<II", len(disc.tracks), radius)
    for (left, right), fl in zip(disc.tracks, disc.flags):
        blob += struct.pack("<QI", len(left), fl) + np.ascontiguousarray(left, "<i2").tobytes() + np.ascontiguousarray(right, "<i2").tobytes()
    src, dst = tmp_path / "disc.bin", tmp_path / "tables.bin"
    src.write_bytes(blob)
    r = subprocess.run([str(driver), str(src), str(dst)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    got = np.frombuffer(dst.read_bytes(), dtype="<u4").reshape(3, len(disc.tracks), 2 * radius + 1)
    w1, w2 = oc.restate(disc, radius)
    assert np.array_equal(got[0], w1) and np.array_equal(got[1], w2) and np.array_equal(got[2], w1)
