"""The host side of the lossy ancestry scan (rg_ancestry_host.cpp with rg_ancestry.h, the header the kernels share) under
AddressSanitizer + UndefinedBehaviorSanitizer: built with gcc's sanitizers and a small stand-alone driver with its own main,
which runs the serial twin (route 0) and the kernels' cutting (route 2) on a handful of the shared cases, each in an exact-size
heap arena.  Run on the CPU as a child process; nothing is loaded into Python."""
import shutil
import struct
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))
import ancestry_cases as ac  # noqa: E402
import arena_layouts as al  # noqa: E402

import mp3rgain_amd as rg  # noqa: E402
from mp3rgain_amd import _capi  # noqa: E402


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
    out = tmp / "ancestry_driver"
    # -ffp-contract=off as the library builds these sources: the counts are then the library's, byte for byte
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off"] + san + [f"-I{ROOT / 'include'}", str(ROOT / "tests" / "san" / "ancestry_driver.cpp"),
                                                                          str(ROOT / "mp3rgain_amd" / "csrc" / "rg_ancestry_host.cpp"), "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return out


def test_ancestry_host_routes_under_asan_ubsan(driver, tmp_path):
    names = {"shape_g1_s1_n1727", "shape_g1_s1_n1728", "shape_g2_s2_n2303", "shape_g1_s2_n3463", "shape_whole_plane", "shape_tile_plus_1", "shape_2ch_s32",
             "shape_2ch_f32", "shape_3ch"}
    chosen = [c for c in ac.cases() if c.name in names]
    assert {c.name for c in chosen} == names
    nf = chosen[0].channels[0][:1000].astype(np.float32)
    nf[[0, 999]] = [np.nan, np.inf]
    chosen.append(ac.Case("f32_short_nan", [nf], 44100, 1, 1, "shape"))
    files = []
    for k, c in enumerate(chosen):
        p = tmp_path / f"{k:03d}.bin"
        dt = c.channels[0].dtype
        p.write_bytes(struct.pack("<Q5I", len(c.channels[0]), len(c.channels), al.FMT[dt], c.sample_rate, c.segments, c.granules)
                      + b"".join(np.ascontiguousarray(ch, dt.newbyteorder("<")).tobytes() for ch in c.channels))
        files.append(str(p))
    r = subprocess.run([str(driver)] + files, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln.split(" ") for ln in r.stdout.split("\n")[:-1]]
    assert len(lines) == 2 * len(chosen)
    for k, c in enumerate(chosen):
        serial, folded = lines[2 * k], lines[2 * k + 1]
        assert serial[:2] == [files[k], "0"] and folded[:2] == [files[k], "2"] and serial[2:] == folded[2:], c.name
        rec = _capi.AncestryRecord.from_buffer_copy(bytes.fromhex(serial[2]))
        cnt = np.frombuffer(bytes.fromhex(serial[3]), dtype="<u8").reshape(rec.views, 2, 576)
        arena, descs = ac.pack_one(c)
        want, wcnt = rg.ancestry_arena(None, 0, descs, arena, c.segments, c.granules)
        assert bytes(rec) == bytes(want[0]) and np.array_equal(cnt, wcnt[0, :rec.views]), c.name
