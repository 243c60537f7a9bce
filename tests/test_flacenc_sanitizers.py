"""The FLAC encoder's serial twin (rg_flacenc_host.cpp with rg_flacenc.h, the header the kernels share) and the host decoder
under AddressSanitizer + UndefinedBehaviorSanitizer: built with gcc's sanitizers and a small stand-alone driver with its own
main, which encodes a handful of the shared cases from exact-size heap arenas into exact-size heap buffers and decodes them
again.  Run on the CPU as a child process; nothing is loaded into Python."""
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
import flacenc_cases as fc  # noqa: E402
from test_flacenc_cpu import twin  # noqa: E402


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
    out = tmp / "flacenc_driver"
    csrc = ROOT / "mp3rgain_amd" / "csrc"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off"] + san + [f"-I{ROOT / 'include'}", str(ROOT / "tests" / "san" / "flacenc_driver.cpp"),
                                                                        str(csrc / "rg_flacenc_host.cpp"), str(csrc / "rg_flacdec.cpp"), "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return out


def test_twin_and_decoder_under_asan_ubsan(driver, tmp_path):
    wanted = {"b4096_lpc8": ("len1", "len2", "len9", "len65", "len4097", "rails24", "noise24", "pad24", "half_silent", "width8", "width20", "ch3",
                             "rate352800", "silence"),
              "b256_lpc12": ("len13", "len63", "len4097", "rails16", "sine24", "r_eq_minus_l"), "b1024_lpc0": ("ar2_20_3ch", "len0")}
    chosen = [(g, k) for g in fc.groups() for k, c in enumerate(g.cases) if c.name in wanted[g.name]]
    assert len(chosen) == sum(len(v) for v in wanted.values())
    files = []
    for j, (g, k) in enumerate(chosen):
        c, tr = g.cases[k], fc.track_of(g.cases[k])
        dt = tr.channels[0].dtype
        p = tmp_path / f"{j:03d}.bin"
        p.write_bytes(struct.pack("<Q6I", c.pcm.shape[1], c.pcm.shape[0], al.FMT[dt], c.rate, c.bps, g.block or 0, 8 if g.lpc is None else g.lpc)
                      + b"".join(np.ascontiguousarray(ch, dt.newbyteorder("<")).tobytes() for ch in tr.channels))
        files.append(str(p))
    r = subprocess.run([str(driver)] + files, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln.split(" ") for ln in r.stdout.split("\n")[:-1]]
    assert len(lines) == len(chosen)
    for (g, k), f, ln in zip(chosen, files, lines):
        want = twin(g.name)[0][k]  # the library's twin, built without sanitizers: the same bytes
        assert ln[0] == f and ln[2] == "1" and int(ln[1]) == len(want) and bytes.fromhex(ln[3]) == want, g.cases[k].name
