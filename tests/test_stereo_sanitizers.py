"""The host side of the stereo image scan (rg_stereo_host.cpp with rg_stereo.h, the header the kernels share) under
AddressSanitizer + UndefinedBehaviorSanitizer: built with gcc's sanitizers and a small stand-alone driver with its own main, which
runs the serial twin (route 0) and the kernels' arithmetic (route 2) on a handful of the shared cases, each in an exact-size heap
arena.  Run on the CPU as a child process; nothing is loaded into Python."""
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
import stereo_cases as sc  # noqa: E402

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
    out = tmp / "stereo_driver"
    cmd = ["g++", "-std=c++17", "-O1", "-g"] + san + [f"-I{ROOT / 'include'}", str(ROOT / "tests" / "san" / "stereo_driver.cpp"),
                                                      str(ROOT / "mp3rgain_amd" / "csrc" / "rg_stereo_host.cpp"), "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return out


def test_stereo_host_routes_under_asan_ubsan(driver, tmp_path):
    wanted = {("r0_bNone", "_n0"), ("r0_bNone", "_n1"), ("r1_bNone", "_n2"), ("r7_b7", "_n15"), ("r7_b1", "_n8"), ("r64_bNone", "_n4097"), ("r255_bNone", "_n1"),
              ("r255_bNone", "_n255"), ("r255_bNone", "_n4351"), ("r255_bNone", "_delay-255"), ("r255_bNone", "_delay255"), ("r7_b4097", "_n8195"),
              ("r64_bNone", "_dual_mono"), ("r64_bNone", "_inverted"), ("r7_b7", "_one_channel"), ("r7_b7", "_eight_channels"), ("r7_b7", "_tie_sign")}
    exact = {("r64_bNone", "s16_all_minus_full_scale"), ("r64_bNone", "s16_minus_against_plus_full_scale"), ("r7_b7", "s32_all_int_min"),
             ("r7_b7", "s32_floor_shift"), ("r7_b7", "s32_opposite_raw"), ("r7_b7", "f32_edges"), ("r7_b7", "f32_signed_zeros"),
             ("r7_b7", "f32_nonfinite_first_both"), ("r7_b7", "f32_nonfinite_last_one"), ("r7_b7", "f32_nan_against_itself")}
    chosen = [(g, tr) for g in sc.groups() for tr in g.tracks
              if (g.name, tr.name) in exact or any(g.name == gn and tr.name[3:] == tail for gn, tail in wanted)]
    assert len(chosen) == 3 * len(wanted) + len(exact)
    files = []
    for k, (g, tr) in enumerate(chosen):
        p = tmp_path / f"{k:03d}.bin"
        dt = tr.channels[0].dtype
        p.write_bytes(struct.pack("<Q5I", len(tr.channels[0]), len(tr.channels), al.FMT[dt], tr.sample_rate, g.block_frames or 0, g.radius)
                      + b"".join(np.ascontiguousarray(ch, dt.newbyteorder("<")).tobytes() for ch in tr.channels))
        files.append(str(p))
    r = subprocess.run([str(driver)] + files, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln.split(" ") for ln in r.stdout.split("\n")[:-1]]
    assert len(lines) == 2 * len(chosen)
    for k, (g, tr) in enumerate(chosen):
        serial, folded = lines[2 * k], lines[2 * k + 1]
        assert serial[:2] == [files[k], "0"] and folded[:2] == [files[k], "2"] and serial[2:] == folded[2:], tr.name
        rec = _capi.StereoRecord.from_buffer_copy(bytes.fromhex(serial[2]))
        want = sc.wants(g.name)[tr.name]
        assert not sc.differences(sc.got(rec), want), tr.name
        assert [int(v) for v in np.frombuffer(bytes.fromhex(serial[3]), "<i8")] == want["sums"], tr.name
