"""The host side of the key scan (rg_key_host.cpp with rg_key.h, rg_fprint.h and rg_spectrum.h, the headers the kernels share,
and rg_spectrum_host.cpp for the tables) under AddressSanitizer + UndefinedBehaviorSanitizer: built with gcc's sanitizers and a
small stand-alone driver with its own main, which runs the serial twin (route 0) and the kernels' arithmetic (route 2) on a
handful of the shared cases, each in an exact-size heap arena with exact-size outputs, and the serial stage 2 over their rows.
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
import key_cases as kc  # noqa: E402

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
    out = tmp / "key_driver"
    # -ffp-contract=off as the library builds these sources: the decimated signal is then the library's, byte for byte
    csrc = ROOT / "mp3rgain_amd" / "csrc"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off"] + san + [f"-I{ROOT / 'include'}", str(ROOT / "tests" / "san" / "key_driver.cpp"),
                                                                          str(csrc / "rg_key_host.cpp"), str(csrc / "rg_spectrum_host.cpp"), "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return out


def test_key_host_routes_under_asan_ubsan(driver, tmp_path):
    W, _, T, _, _ = kc.shape()
    names = {"n16D_s16_1ch", "m1_f32_2ch", "m4095_s32_1ch", "m4096_s16_1ch", "m4096_f32_3ch", f"f{T + 2}_s16_2ch", f"f{2 * T}_f32_1ch", f"m{2 * W + 1}_s32_1ch",
             "nonfinite_f32_2ch", "silence_then_chord_s16_2ch", "rate8000_f32_1ch", "rate192000_s16_1ch", "rate48000_s32_2ch", "rate4000_s16_1ch", "chord_2s_s16_2ch"}
    chosen = [c for c in kc.cases() if c.name in names]
    assert {c.name for c in chosen} == names
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
    rows = []
    for k, c in enumerate(chosen):
        arena, descs = kc.pack([c])
        for line, route in ((lines[2 * k], 0), (lines[2 * k + 1], 2)):
            assert line[:2] == [files[k], str(route)]
            rec = _capi.KeyRecord.from_buffer_copy(bytes.fromhex(line[2]))
            want, wy, wbands, wrows = rg.key_arena(None, route, descs, arena, segment=8)
            assert bytes(rec) == bytes(want[0]), (c.name, route)
            assert bytes.fromhex(line[3][1:]) == wy.tobytes() and bytes.fromhex(line[4][1:]) == wbands.tobytes(), (c.name, route)
            assert bytes.fromhex(line[5][1:]) == wrows.tobytes(), (c.name, route)
        rows.append(np.frombuffer(bytes.fromhex(lines[2 * k + 1][5][1:]), dtype="<u2").reshape(-1, 12))
    want = rg.key_from_chroma(None, 0, rows, segment=8)
    last = lines[-1]
    assert last[0] == "stage2" and bytes.fromhex(last[1][1:]) == b"".join(bytes(w) for w in want)
    assert any(not w.flags & (_capi.KEY_NONE | _capi.KEY_SHORT) for w in want) and any(w.flags & _capi.KEY_SHORT for w in want)
