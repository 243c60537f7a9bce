"""The host side of the rational resampler and of the cross-rate fingerprint (rg_resample_host.cpp with rg_resample.h, and
rg_fprint_host.cpp and rg_spectrum_host.cpp behind it) under AddressSanitizer + UndefinedBehaviorSanitizer: built with gcc's
sanitizers and a small stand-alone driver with its own main, which runs route 0 and the kernel's arithmetic (route 2) on a handful
of the shared cases, each in an exact-size heap arena with exact-size outputs.  Run on the CPU as a child process; nothing is
loaded into Python."""
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
import resample_cases as rc  # noqa: E402

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
    out = tmp / "resample_driver"
    # -ffp-contract=off as the library builds these sources: y and the codes are then the library's, byte for byte
    csrc = ROOT / "mp3rgain_amd" / "csrc"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off"] + san + [f"-I{ROOT / 'include'}", str(ROOT / "tests" / "san" / "resample_driver.cpp"),
                                                                          str(csrc / "rg_resample_host.cpp"), str(csrc / "rg_fprint_host.cpp"),
                                                                          str(csrc / "rg_spectrum_host.cpp"), "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return out


def test_resample_host_routes_under_asan_ubsan(driver, tmp_path):
    names = {"m0_r48000_f32_1ch", "m1_r48000_s16_2ch", "m257_r48000_s16_3ch", "m511_r8000_s16_2ch", "m256_r44100_s32_2ch", "m300_tail_r32000_s16_1ch",
             "identity_r11025_f32_2ch", "l7_r37800_s32_2ch", "r192k_r192000_s16_1ch", "unsupported_r384000_f32_2ch", "nan_r48000_f32_2ch"}
    chosen = [c for c in rc.cases() if c.name in names]
    assert {c.name for c in chosen} == names
    # one track long enough for codes: 3 of them
    chosen.append(rc.Case("long", [rc.fc.as_format(rc.fc.noise(rc.n_for(4096 + 3 * 512 + 5, 48000), 901), "s16")], 48000))
    files = []
    for k, c in enumerate(chosen):
        p = tmp_path / f"{k:03d}.bin"
        dt = c.channels[0].dtype
        p.write_bytes(struct.pack("<Q3I", len(c.channels[0]), len(c.channels), al.FMT[dt], c.sample_rate)
                      + b"".join(np.ascontiguousarray(ch, dt.newbyteorder("<")).tobytes() for ch in c.channels))
        files.append(str(p))
    r = subprocess.run([str(driver)] + files, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln.split(" ") for ln in r.stdout.split("\n")[:-1]]
    assert len(lines) == 2 * len(chosen)
    for k, c in enumerate(chosen):
        arena, descs = rc.pack([c])
        for line, route in ((lines[2 * k], 0), (lines[2 * k + 1], 2)):
            assert line[:2] == [files[k], str(route)]
            rec = _capi.XrateRecord.from_buffer_copy(bytes.fromhex(line[2]))
            want, wcodes, wbands, wy = rg.xrate_fingerprint_arena(None, route, descs, arena)
            assert bytes(rec) == bytes(want[0]), (c.name, route)
            assert bytes.fromhex(line[3][1:]) == wy.tobytes() and bytes.fromhex(line[4][1:]) == wcodes.tobytes(), (c.name, route)
            assert bytes.fromhex(line[5][1:]) == wbands.tobytes(), (c.name, route)
    assert _capi.XrateRecord.from_buffer_copy(bytes.fromhex(lines[-1][2])).codes == 3
