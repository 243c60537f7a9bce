"""The host side of the dynamic range scan (rg_dr_host.cpp with rg_dr.h, the header the kernels share) under AddressSanitizer +
UndefinedBehaviorSanitizer: built with gcc's sanitizers and a small stand-alone driver with its own main, which runs the serial
twin (route 0) and the kernels' arithmetic (route 2) on a handful of the shared cases, each in an exact-size heap arena.  Run on
the CPU as a child process; nothing is loaded into Python."""
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
import dr_cases as dc  # noqa: E402

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
    out = tmp / "dr_driver"
    cmd = ["g++", "-std=c++17", "-O1", "-g"] + san + [f"-I{ROOT / 'include'}", str(ROOT / "tests" / "san" / "dr_driver.cpp"),
                                                      str(ROOT / "mp3rgain_amd" / "csrc" / "rg_dr_host.cpp"), "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return out


def test_dr_host_routes_under_asan_ubsan(driver, tmp_path):
    names = set()
    for tag, fmt in (("s16", _capi.FMT_S16_PLANAR), ("s32", _capi.FMT_S32_PLANAR), ("f32", _capi.FMT_F32_PLANAR)):
        c, t = dc.shape(fmt)
        names |= {f"{tag}_n{n}_b{b}" for n, b in ((0, 1), (1, 1), (c + 1, c), (t + 1, t), (2 * t + 3, 7))}
    names |= {"s32_int_min_blocks_of_8", "s32_low_limbs_carry", "f32_at_256_and_beyond", "f32_nonfinite_first_middle_last", "f32_all_nan",
              "f32_zeros_and_subnormals", "f32_exact_halves", "s16_minus_full_scale_alone", "s16_ladder", "s32_8ch_n5_b4", "f32_many_blocks"}
    chosen = [(g, tr) for g in dc.groups() for tr in g.tracks if tr.name in names and g.top_permille in (None, 400)]
    assert {tr.name for _, tr in chosen} == names
    files = []
    for k, (g, tr) in enumerate(chosen):
        p = tmp_path / f"{k:03d}.bin"
        dt = tr.channels[0].dtype
        p.write_bytes(struct.pack("<Q5I", len(tr.channels[0]), len(tr.channels), al.FMT[dt], tr.sample_rate, g.block_frames or 0, g.top_permille or 200)
                      + b"".join(np.ascontiguousarray(ch, dt.newbyteorder("<")).tobytes() for ch in tr.channels))
        files.append(str(p))
    r = subprocess.run([str(driver)] + files, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln.split(" ") for ln in r.stdout.split("\n")[:-1]]
    assert len(lines) == 2 * len(chosen)
    for k, (g, tr) in enumerate(chosen):
        serial, folded = lines[2 * k], lines[2 * k + 1]
        assert serial[:2] == [files[k], "0"] and folded[:2] == [files[k], "2"] and serial[2] == folded[2], tr.name
        rec = _capi.DrRecord.from_buffer_copy(bytes.fromhex(serial[2]))
        assert not dc.differences(dc.got(rec), dc.wants(g.name)[tr.name]), tr.name
