"""The host side of the duplicate finder (rg_fprint_host.cpp with rg_fprint.h and rg_spectrum.h, the headers the kernels share,
and rg_spectrum_host.cpp for the tables) under AddressSanitizer + UndefinedBehaviorSanitizer: built with gcc's sanitizers and a
small stand-alone driver with its own main, which runs the serial twin (route 0) and the kernels' arithmetic (route 2) on a
handful of the shared cases, each in an exact-size heap arena with exact-size outputs, and the serial match over their codes.
Run on the CPU as a child process; nothing is loaded into Python."""
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
import fingerprint_cases as fc  # noqa: E402

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
    out = tmp / "fingerprint_driver"
    # -ffp-contract=off as the library builds these sources: the codes are then the library's, byte for byte
    csrc = ROOT / "mp3rgain_amd" / "csrc"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off"] + san + [f"-I{ROOT / 'include'}", str(ROOT / "tests" / "san" / "fingerprint_driver.cpp"),
                                                                          str(csrc / "rg_fprint_host.cpp"), str(csrc / "rg_spectrum_host.cpp"), "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return out


def test_fingerprint_host_routes_under_asan_ubsan(driver, tmp_path):
    T = fc.tile_codes()
    names = {"n4095_s16_1ch", "n4096_f32_1ch", "n4608_s32_3ch", "k2_tail_s16_1ch", f"k{T + 1}_s16_2ch", f"k{2 * T - 1}_f32_1ch", "nonfinite_f32_2ch",
             "rate8000_f32_2ch", "rate96000_s16_1ch"}
    chosen = [c for c in fc.cases() if c.name in names]
    assert {c.name for c in chosen} == names
    # two tracks long enough for the match at block 32: a copy three codes late, and the original
    x = fc.noise(fc.L + 60 * fc.H, 900)
    chosen += [fc.Case("long", [fc.as_format(x, "s16")], 44100), fc.Case("long_late", [fc.as_format(x[3 * fc.H:] * 0.5, "f32")], 44100)]
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
    assert len(lines) == 2 * len(chosen) + 1
    codes = []
    for k, c in enumerate(chosen):
        arena, descs = fc.pack([c])
        for line, route in ((lines[2 * k], 0), (lines[2 * k + 1], 2)):
            assert line[:2] == [files[k], str(route)]
            rec = _capi.FingerprintRecord.from_buffer_copy(bytes.fromhex(line[2]))
            want, wcodes, wbands = rg.fingerprint_arena(None, route, descs, arena)
            assert bytes(rec) == bytes(want[0]), (c.name, route)
            assert bytes.fromhex(line[3][1:]) == wcodes.tobytes() and bytes.fromhex(line[4][1:]) == wbands.tobytes(), (c.name, route)
        codes.append(np.frombuffer(bytes.fromhex(lines[2 * k + 1][3][1:]), dtype="<u4"))
    want = rg.fingerprint_match_codes(None, 0, codes, [c.sample_rate for c in chosen], 32, 3, 8, 100)
    last = lines[-1]
    assert last[0] == "pairs" and bytes.fromhex(last[2][1:]) == want.tobytes()
    groups, _, found = rg.fingerprint_groups(len(chosen), want)
    assert int(last[1]) == found == 1 and bytes.fromhex(last[3][1:]) == groups.tobytes()
    k = len(chosen)
    assert groups[k - 1] == k - 2 and want[-1]["lag"] == 3 and want[-1]["flags"] & _capi.FP_PAIR_PROBE_J
