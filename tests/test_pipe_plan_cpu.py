"""The two sizing rules of the MP3 loader pipeline (mp3rgain_amd/csrc/rg_pipe_plan.h), compiled with the host compiler alone:
how many granule-channels the open chunk may hold (warm-up of 1/8, 1/4, 1/2 of a chunk, whole chunks, the taper once the device
waits for the loaders), and which decoded chunks are analysed right away as an album part.  Through the pipeline itself they can
only be met with chunking that depends on timing."""
from __future__ import annotations

import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parents[1]
CHUNK = 786432  # kPipeChunkUnits


@pytest.fixture(scope="module")
def ask(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("no g++")
    exe = tmp_path_factory.mktemp("pipe_plan") / "pipe_plan_driver"
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", f"-I{ROOT / 'mp3rgain_amd' / 'csrc'}",
                        str(ROOT / "tests" / "san" / "pipe_plan_driver.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr

    def ask(*lines):
        out = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True, check=True).stdout.split("\n")
        return [tuple(int(x) for x in l.split()) for l in out if l]

    return ask


def test_unit_cap_warm_up(ask):
    got = ask(*[f"cap {k} 0 0 0 0 10" for k in (0, 1, 2, 3, 7)])
    assert got == [(98304, 0), (196608, 0), (393216, 0), (786432, 0), (786432, 0)]
    assert [g[0] for g in got] == [CHUNK >> 3, CHUNK >> 2, CHUNK >> 1, CHUNK, CHUNK]


def test_unit_cap_taper(ask):
    got = ask("cap 3 100000 1 5 500000 10",  # left = 100000 + 5 files x 100000 = 600000: half of it
              "cap 0 100000 1 5 500000 10",  # the warm-up cap is smaller
              "cap 5 10000 1 9 90000 10",    # left = 20000: the floor of an eighth of a chunk
              "cap 3 0 1 0 0 10",            # starved before any file has its place: nothing to go by
              "cap 3 100000 0 5 500000 10")  # not starved
    assert got == [(300000, 1), (98304, 0), (98304, 1), (786432, 0), (786432, 0)]


def test_chunk_is_part(ask):
    got = ask("part 1200 10 120.0 0", "part 1199 10 120.0 0", "part 0 0 0.0 0", "part 0 0 120.0 0", "part 1 10 120.0 1", "part 0 0 120.0 1",
              "part 1 10 0.0 0")
    assert got == [(1,), (0,), (0,), (0,), (1,), (1,), (1,)]
