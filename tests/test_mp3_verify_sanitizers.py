"""The host side of MP3 verification (rg_mp3verify.cpp with rg_crc16.h, the header the kernels share, on top of the host
decoder's frame walk) under AddressSanitizer + UndefinedBehaviorSanitizer: built with gcc's sanitizers and a small stand-alone
driver, fed mutated, truncated and spliced tagged streams as exact-size heap buffers -- a read past a buffer, a signed overflow
or a misaligned access aborts the driver."""
import platform
import random
import shutil
import subprocess
import sys
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))
import mp3_verify_cases as vc  # noqa: E402


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
    out = tmp / "mp3verify_driver"
    csrc = ROOT / "mp3rgain_amd" / "csrc"
    fma = ["-mfma"] if platform.machine() == "x86_64" else []
    cmd = ["g++", "-std=c++17", "-O1", "-g"] + san + ["-ffp-contract=off", f"-I{ROOT / 'include'}"] + fma + [
        str(ROOT / "tests" / "san" / "mp3verify_driver.cpp"), str(csrc / "rg_mp3verify.cpp"), str(csrc / "rg_mp3dec.cpp"), str(csrc / "rg_mp3gain.cpp"),
        str(csrc / "rg_flacdec.cpp"), "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return out


def test_mp3_verification_under_asan_ubsan(driver, tmp_path):
    rng = random.Random(13)
    bases = [c.data for c in vc.clean_cases()[::2] + vc.damaged_cases()] + [p.read_bytes() for p in sorted(vc.FIXTURES.glob("*.mp3"))]
    files = []
    for k, d in enumerate(bases):  # the cases themselves
        f = tmp_path / f"b{k:03d}.mp3"
        f.write_bytes(d)
        files.append(str(f))
    for k in range(1500):
        d = bytearray(rng.choice(bases))
        kind = rng.randrange(5)
        if kind == 0:
            for _ in range(rng.randint(1, 20)):
                d[rng.randrange(len(d))] = rng.randrange(256)
        elif kind == 1:
            d = d[:rng.randrange(len(d) + 1)]
        elif kind == 2:
            a = rng.randrange(len(d))
            del d[a:a + rng.randint(1, 600)]
        elif kind == 3:  # the tag frame's fields: flags word, extension, lengths
            a = rng.randrange(min(len(d), 300))
            d[a:a + 4] = bytes(rng.randrange(256) for _ in range(4))
        else:  # the tag frame cut short, or alone
            d = d[:rng.randrange(min(len(d), 700))]
        f = tmp_path / f"f{k:04d}.mp3"
        f.write_bytes(bytes(d))
        files.append(str(f))
    (tmp_path / "empty.mp3").write_bytes(b"")
    files.append(str(tmp_path / "empty.mp3"))
    for lo in range(0, len(files), 500):
        r = subprocess.run([str(driver)] + files[lo:lo + 500], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
