"""The host side of the spectral scan (rg_spectrum_host.cpp with rg_spectrum.h, the header the kernels share) under
AddressSanitizer + UndefinedBehaviorSanitizer: built with gcc's sanitizers and a small stand-alone driver with its own main,
which runs the serial twin (route 0) and the kernels' arithmetic (route 2) on a handful of the shared cases, each in an
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
import arena_layouts as al  # noqa: E402
import spectrum_cases as sc  # noqa: E402


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
    out = tmp / "spectrum_driver"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off"] + san + [f"-I{ROOT / 'include'}", str(ROOT / "tests" / "san" / "spectrum_driver.cpp"),
                                                                           str(ROOT / "mp3rgain_amd" / "csrc" / "rg_spectrum_host.cpp"), "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return out


def test_spectrum_host_routes_under_asan_ubsan(driver, tmp_path):
    t = sc.shape()[3]
    names = {f"white-{fmt}-{n}" for fmt in ("s16", "s24", "f32") for n in (sc.L - 1, sc.L, sc.L + sc.H - 1, sc.L + sc.H, sc.L + 2 * sc.H + 1)}
    names |= {f"white-s16-{sc.L + t * sc.H + 1}", "evenodd-s24", "six-f32", "nan-first", "nan-overlap", "nan-tail", "nan-everywhere", "silence",
              "verdict-white-16k"}
    chosen = [tr for tr in sc.tracks() if tr.name in names]
    assert len(chosen) == len(names)
    files = []
    for k, tr in enumerate(chosen):
        p = tmp_path / f"{k:03d}.bin"
        dt = tr.channels[0].dtype
        p.write_bytes(struct.pack("<Q3I", len(tr.channels[0]), len(tr.channels), al.FMT[dt], tr.sample_rate)
                      + b"".join(np.ascontiguousarray(ch, dt.newbyteorder("<")).tobytes() for ch in tr.channels))
        files.append(str(p))
    r = subprocess.run([str(driver)] + files, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln.split(" ") for ln in r.stdout.split("\n")[:-1]]
    assert len(lines) == 2 * sum(len(tr.channels) for tr in chosen)
    wants = sc.wants()
    tol = {0: (sc.F64_TOLERANCE, 1e-9), 2: tuple(sc.TOLERANCE_FACTOR * x for x in sc.measured())}
    at = 0
    for k, tr in enumerate(chosen):
        for route in (0, 2):
            for c, (ref, analysed, skipped) in enumerate(wants[tr.name]):
                name, rt, ch, flags, ch_flags, got_analysed, got_skipped, cutoff, edge, *bands = lines[at]
                at += 1
                assert (name, int(rt), int(ch), int(got_analysed), int(got_skipped)) == (files[k], route, c, analysed, skipped), tr.name
                e = np.array([float.fromhex(x) for x in bands])
                a, b = sc.errors(e, ref)
                assert a <= tol[route][0] and b <= tol[route][1], (tr.name, route, a, b)
                assert (float.fromhex(cutoff), float.fromhex(edge), int(ch_flags)) == sc.verdict_of_energy(e, analysed, tr.sample_rate), tr.name
