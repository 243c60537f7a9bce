"""The host side of the null test (rg_compare_host.cpp with rg_compare.h, the header the kernels share) under AddressSanitizer +
UndefinedBehaviorSanitizer: built with gcc's sanitizers and a small stand-alone driver with its own main, which runs the serial
twin (route 0) and the kernels' arithmetic (route 2) on a handful of the shared cases, each pair in an exact-size heap arena.  Run
on the CPU as a child process; nothing is loaded into Python."""
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
import compare_cases as cc  # noqa: E402

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
    out = tmp / "compare_driver"
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off"] + san + [f"-I{ROOT / 'include'}", str(ROOT / "tests" / "san" / "compare_driver.cpp"),
                                                                            str(ROOT / "mp3rgain_amd" / "csrc" / "rg_compare_host.cpp"), "-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return out


def test_compare_host_routes_under_asan_ubsan(driver, tmp_path):
    wanted = {"r0_s16": range(12), "r1_s16": (0, 1, 8, 10, 11), "r2047_s16": (0, 4, 5, 10, 11), "r255_s16": range(12, 15), "r17_f32": range(12), "r17_s32": (3, 5, 7),
              "values": None, "channels": None, "bNone": None, "b7": (0, 3), "b1": (0,), "single_bNone": None, "single_b4097": None, "seg16x4097": (1, 2),
              "seg4x4096": (0,), "residues": (0, 16, 17, 33, 34, 50)}
    chosen = []
    for c in cc.calls():
        if c.name in wanted:
            picks = range(len(c.pairs)) if wanted[c.name] is None else wanted[c.name]
            chosen += [(c, k) for k in picks]
    assert len({c.name for c, _ in chosen}) == len(wanted)
    files = []
    for k, (c, i) in enumerate(chosen):
        a, b, hint = c.pairs[i]
        ta, tb = c.tracks[a], c.tracks[b]
        p = tmp_path / f"{k:03d}.bin"
        o = c.opts
        head = struct.pack("<QQq10I", len(ta.channels[0]), len(tb.channels[0]), hint, len(ta.channels), len(tb.channels), al.FMT[ta.channels[0].dtype],
                           al.FMT[tb.channels[0].dtype], ta.sample_rate, tb.sample_rate, o["radius"], o["segments"], o["segment_frames"], o.get("block_frames") or 0)
        p.write_bytes(head + b"".join(np.ascontiguousarray(ch, ch.dtype.newbyteorder("<")).tobytes() for t in (ta, tb) for ch in t.channels))
        files.append(str(p))
    r = subprocess.run([str(driver)] + files, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln.split(" ") for ln in r.stdout.split("\n")[:-1]]
    assert len(lines) == 2 * len(chosen)
    for k, (c, i) in enumerate(chosen):
        serial, folded = lines[2 * k], lines[2 * k + 1]
        assert serial[:2] == [files[k], "0"] and folded[:2] == [files[k], "2"] and serial[2:] == folded[2:], (c.name, i)
        rec = _capi.CompareRecord.from_buffer_copy(bytes.fromhex(serial[2]))
        want = dict(cc.wants(c.name)[i], a=0, b=1)
        assert not cc.differences(cc.got(rec), want), (c.name, i)
        R, S = c.opts["radius"], c.opts["segments"]
        rows = np.frombuffer(bytes.fromhex(serial[3]), "<i8").reshape(S, _capi.CMP_MAX_CHANNELS, 2 * R + 3)
        raw = bytes.fromhex(serial[4])
        blocks = [_capi.CompareBlock.from_buffer_copy(raw[j:j + 48]) for j in range(0, len(raw), 48)]
        assert not cc.row_differences(rows, blocks, want, R), (c.name, i)
