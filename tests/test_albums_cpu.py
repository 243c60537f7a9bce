"""rg_analyze_albums_node (include/mp3rgain_amd_node.h) without a GPU: whole albums dealt out by their files' bytes, every
album through its device's album entries, results scattered back to input order, the first failing file in input order
ending its album and no other (src/replaygain.rs:1055, per album).  The engines are tests/test_node_cpu.py's stand-ins
behind rg_node_create_backend; the real engine is exercised by tests/test_gpu_albums.py."""
import ctypes as C
import os
import re
import shutil
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
from test_node_cpu import FakeEngines, _write  # noqa: E402

from mp3rgain_amd import _capi, album  # noqa: E402
from mp3rgain_amd import replaygain as R  # noqa: E402

H = _capi.HISTOGRAM_SIZE


def _library(tmp_path, sizes, seed=5):
    rng = np.random.default_rng(seed)
    albums, k = [], 0
    for n in sizes:
        files = []
        for _ in range(n):
            bins = {int(b): int(c) for b, c in zip(rng.integers(5000, 9000, 5), rng.integers(1, 300, 5))}
            files.append(_write(tmp_path, k, bins, peak=float(rng.uniform(0.1, 1.2)), pad=int(rng.integers(0, 9000))))
            k += 1
        albums.append(files)
    return albums


def _want(fe, files):
    total, peak, tracks = np.zeros(H, np.uint32), 0.0, []
    for f in files:
        (hist, loud, pk), _ = fe._one(str(f))
        total += hist
        peak = max(peak, pk)
        tracks.append((loud, pk))
    return album.album_result_from_hist(total, peak), tracks


@pytest.mark.parametrize("devices", [[0], [0, 1], [2, 0, 1]])
def test_albums_dealt_whole_and_scattered_back(tmp_path, devices):
    albums = _library(tmp_path, [3, 1, 0, 5, 2, 4, 1, 6, 0, 2])
    fe = FakeEngines()
    with R.Node(devices, _backend=fe.table) as node:
        got = node.analyze_albums_files(albums)
        own = node.last_partition(sum(len(a) for a in albums))
    # dealing: albums by their files' bytes, every file of an album on its album's device
    weights = [sum(os.path.getsize(f) for f in a) for a in albums]
    album_owner = R.node_partition(weights, len(devices))
    assert own == [album_owner[a] for a, files in enumerate(albums) for _ in files]
    begins = sorted((d, n) for what, d, n in fe.calls if what == "begin")
    assert begins == sorted((devices[album_owner[a]], len(files)) for a, files in enumerate(albums))
    assert sum(1 for what, _, _ in fe.calls if what == "pack") == len(albums)
    assert len(got) == len(albums)
    for files, g in zip(albums, got):
        want, tracks = _want(fe, files)
        assert isinstance(g, R.AlbumGainResult)
        assert (g.album_loudness_db, g.album_gain_db, g.album_peak) == (want["album_loudness_db"], want["album_gain_db"], want["album_peak"])
        assert [(t.loudness_db, t.peak) for t in g.tracks] == tracks


def test_first_failing_file_ends_its_album_only(tmp_path):
    albums = _library(tmp_path, [4, 3, 5, 2])
    albums[1][2] = _write(tmp_path, 101, fail="Unsupported sample rate: 44000 Hz. Supported rates: ...", code=-2)
    albums[2][1] = _write(tmp_path, 102, fail=f"Failed to probe format: {tmp_path}/x.fake", code=-9)
    albums[2][3] = _write(tmp_path, 103, fail="Unsupported sample rate: 7000 Hz. Supported rates: ...", code=-2)
    albums[3][0] = tmp_path / "missing.fake"
    fe = FakeEngines()
    with R.Node([0, 1], _backend=fe.table) as node:
        got = node.analyze_albums_files(albums)
    want, _ = _want(fe, albums[0])
    assert isinstance(got[0], R.AlbumGainResult) and got[0].album_loudness_db == want["album_loudness_db"]
    assert isinstance(got[1], R.ReplayGainError) and got[1].code == -2 and str(got[1]).startswith("Unsupported sample rate: 44000")
    assert isinstance(got[2], R.ReplayGainError) and got[2].code == -9 and "Failed to probe format" in str(got[2])  # not the later -2
    assert isinstance(got[3], R.ReplayGainError) and got[3].code == -8 and str(got[3]) == f"Failed to open: {albums[3][0]}"


def _raw_call(node, paths, first, n_albums):
    lib = _capi.load()
    n = len(paths)
    p = (C.c_char_p * max(1, n))(*[os.fsencode(str(x)) for x in paths])
    fa = (C.c_size_t * len(first))(*first) if first is not None else None
    out = (_capi.TrackResult * max(1, n))()
    st = (C.c_int32 * max(1, n))()
    alb = (_capi.AlbumResult * max(1, n_albums))()
    ast = (C.c_int32 * max(1, n_albums))()
    return lib.rg_analyze_albums_node(node._node, p, n, fa, n_albums, -1, out, st, alb, ast)


@pytest.mark.parametrize("first, n_albums, why", [
    (None, 2, "NULL"),
    ([1, 2, 3], 2, "album_first[0]"),
    ([0, 1, 2], 2, "number of files"),
    ([0, 2, 1, 3], 3, "decreases"),
])
def test_malformed_album_first_is_refused(tmp_path, first, n_albums, why):
    paths = [p for a in _library(tmp_path, [1, 2]) for p in a]
    fe = FakeEngines()
    with R.Node([0], _backend=fe.table) as node:
        rc = _raw_call(node, paths, first, n_albums)
        assert rc == _capi.RG_ERR_INVALID_ARG
        assert why in R._capi.load().rg_node_last_error(node._node).decode()
    assert not [c for c in fe.calls if c[0] == "begin"]


def test_no_albums_is_a_valid_call(tmp_path):
    fe = FakeEngines()
    with R.Node([0, 1], _backend=fe.table) as node:
        assert node.analyze_albums_files([]) == []
        assert _raw_call(node, [], None, 0) == _capi.RG_OK


def test_album_kernels_keep_to_registers(tmp_path):
    """rg_albums.hip (the fold and the batched read-out): no private segment, no scratch instruction."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not Path(hipcc).exists():
        pytest.skip("no hipcc")
    root = Path(__file__).resolve().parent.parent
    out = tmp_path / "rg_albums.s"
    subprocess.run([hipcc, "-O3", "-Wno-missing-braces", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S",
                    str(root / "mp3rgain_amd" / "csrc" / "rg_albums.hip"), "-o", str(out)], check=True, capture_output=True, timeout=600)
    isa = out.read_text()
    for name in ("rg_album_fold_kernel", "rg_album_results_kernel"):
        assert name in isa
    sizes = [int(x) for x in re.findall(r"\.private_segment_fixed_size:\s+(\d+)", isa)]
    assert sizes and all(x == 0 for x in sizes)
    assert "scratch_" not in isa
