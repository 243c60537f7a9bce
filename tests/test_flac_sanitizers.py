"""The host FLAC decoder (rg_flacdec.cpp, with the frame decoder rg_flac_frame.h the device kernel shares) under
AddressSanitizer + UndefinedBehaviorSanitizer: built with gcc's sanitizers and a small driver, fed a few thousand damaged
streams as exact-size heap buffers -- any read past a buffer, signed overflow or misaligned access aborts the driver."""
import random
import shutil
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))
import flacenc as fe  # noqa: E402


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    out = tmp_path_factory.mktemp("san") / "flacdec_driver"
    csrc = ROOT / "mp3rgain_amd" / "csrc"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", f"-I{ROOT / 'include'}",
           str(ROOT / "tests" / "san" / "flacdec_driver.cpp"), str(csrc / "rg_flacdec.cpp"), "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        if "sanitize" in r.stderr or "asan" in r.stderr.lower():
            pytest.skip("this toolchain has no sanitizer runtime")
        raise AssertionError(r.stderr)
    return out


def test_flac_decoder_under_asan_ubsan(driver, tmp_path):
    rng = random.Random(11)
    nrng = np.random.default_rng(11)
    bases = []
    for k, (ch, bps, opt) in enumerate([(2, 16, fe.Options(stereo="alternate", block_size=1152)),
                                        (1, 24, fe.Options(subframe="lpc", order=20, rice2=True, escape_every=2)),
                                        (6, 12, fe.Options(subframe="fixed", order=3, block_size=576)),
                                        (2, 8, fe.Options(variable=True, blocks=[100, 700, 1, 2000, 199], stereo="right_side")),
                                        (2, 20, fe.Options(subframe="verbatim", block_size=256, stereo="mid_side"))]):
        n = sum(opt.blocks) if opt.blocks else 3000 + 517 * k
        bases.append(fe.encode(fe.test_pcm(nrng, ch, n, bps), 44100, bps, opt))
    bases += [d[1] for d in fe.damaged_variants()]
    files = []
    for k in range(3000):
        d = bytearray(rng.choice(bases))
        kind = rng.randrange(5)
        if kind == 0:
            for _ in range(rng.randint(1, 30)):
                d[rng.randrange(len(d))] = rng.randrange(256)
        elif kind == 1:
            d = d[:rng.randrange(len(d) + 1)]
        elif kind == 2:
            a = rng.randrange(len(d))
            del d[a:a + rng.randint(1, 1000)]
        elif kind == 3:
            a = rng.randrange(len(d))
            d[a:a] = bytes(rng.randrange(256) for _ in range(rng.randint(1, 200)))
        else:  # a sync-like run with random header bytes: the header parser's every branch
            a = rng.randrange(len(d))
            d[a:a] = bytes([0xFF, rng.choice([0xF8, 0xF9])] + [rng.randrange(256) for _ in range(rng.randint(0, 14))])
        f = tmp_path / f"f{k:04d}.flac"
        f.write_bytes(bytes(d))
        files.append(str(f))
    (tmp_path / "empty.flac").write_bytes(b"")
    files.append(str(tmp_path / "empty.flac"))
    for lo in range(0, len(files), 500):
        r = subprocess.run([str(driver)] + files[lo:lo + 500], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
