"""Many R 128 albums in one call, the parts a machine without a GPU can check: the precondition of the comparisons against
the float64 checkers in tests/test_gpu_r128_albums.py (no block of any album's union near a gate), the kernel descriptors
of mp3rgain_amd/csrc/rg_r128_albums.hip, the exports and struct sizes, and the host rule that assigns an album its form
(one workgroup or wide passes), its counting workgroups and its round."""
import ctypes as C
import re
import shutil
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import r128albums_cases as ac  # noqa: E402
import r128cases  # noqa: E402
import r128range_cases  # noqa: E402
import r128range_ref  # noqa: E402
import r128ref  # noqa: E402

ROOT = Path(__file__).resolve().parent.parent
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
TOL = 100.0 * r128cases.load_measured()["worst_relative_block_error"]
ST_TOL = 100.0 * r128range_cases.load_measured()["worst_relative_st_error"]


def test_no_block_of_any_album_is_near_a_gate():
    """On the checkers alone: in the partitions the GPU tests use, no momentary block of an album's union lies within relative
    10 x TOL of either of that album's gates, and no short-term block within 10 x ST_TOL of either loudness-range gate.  So no
    block changes sides of a gate within the tolerance, and every album is compared (none is left out)."""
    sig = ac.signals()
    per_track = [(r128ref.block_z(ch, rate), r128range_ref.short_term(ch, rate)) for _, ch, rate in sig]
    worst_z, worst_st = np.inf, np.inf
    for seed in ac.SEEDS:
        albums = ac.albums(seed)
        assert sorted(i for a in albums for i in a) == list(range(62))
        for a in albums:
            if not a:
                continue
            z = np.concatenate([per_track[i][0] for i in a])
            st = np.concatenate([per_track[i][1] for i in a])
            _, _, thr = r128ref.gate(z)
            for gate in (r128ref.ABS_GATE, thr):
                if len(z):
                    d = float(np.min(np.abs(z - gate) / gate))
                    worst_z = min(worst_z, d)
                    assert d > 10.0 * TOL, (seed, a, gate, d)
            thr = r128range_ref.loudness_range(st)["thr"]
            for gate in (r128range_ref.ABS_GATE, thr):
                if len(st):
                    d = float(np.min(np.abs(st - gate) / gate))
                    worst_st = min(worst_st, d)
                    assert d > 10.0 * ST_TOL, (seed, a, gate, d)
    print(f"nearest momentary block {worst_z:.2e} (bar {10.0 * TOL:.2e}), nearest short-term block {worst_st:.2e} (bar {10.0 * ST_TOL:.2e})")


KERNELS = ("rg_r128a_gate_kernel", "rg_r128a_select_kernel", "rg_r128a_wide_gate_kernel", "rg_r128a_wide_count_kernel",
           "rg_r128a_wide_finish_kernel")


def test_albums_kernels_use_no_scratch(tmp_path):
    if not Path(HIPCC).exists():
        pytest.skip("no hipcc")
    out = tmp_path / "rg_r128_albums.s"
    subprocess.run([HIPCC, "-O3", "-std=c++17", "-Wno-missing-braces", "--offload-arch=gfx950", "--cuda-device-only", "-S",
                    str(ROOT / "mp3rgain_amd" / "csrc" / "rg_r128_albums.hip"), "-o", str(out)], check=True, capture_output=True, timeout=1500)
    isa = out.read_text()
    kernels = re.findall(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", isa, re.S)
    names = [k for k, _ in kernels]
    for want in KERNELS:
        assert sum(want in k for k in names) == 1, (want, names)
    assert len(kernels) == len(KERNELS), names
    for name, body in kernels:
        m = re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", body)
        assert m and int(m.group(1)) == 0, name
        assert re.search(r"\.amdhsa_uses_dynamic_stack 0", body), name
        lds = re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", body)
        assert lds and int(lds.group(1)) <= 64 * 1024, name
    assert not re.search(r"atomic_(add|pk_add|fadd|fmax|fmin|max|min)_f", isa)


def test_albums_entry_points_and_layout(capi):
    from mp3rgain_amd import _capi

    for name in ("rg_r128_analyze_albums_pcm", "rg_r128_analyze_albums_pcm_dynamics", "rg_r128_analyze_albums",
                 "rg_r128_analyze_albums_dynamics", "rg_r128_analyze_tracks_node", "rg_r128_analyze_albums_node"):
        assert hasattr(capi, name), name
    assert C.sizeof(_capi.R128Dynamics) == 48 and C.sizeof(_capi.R128TrackResult) == 48 and C.sizeof(_capi.R128AlbumResult) == 40
    assert capi.rg_abi_version() == 5


def test_album_form_counting_workgroups_and_rounds(capi):
    """The host rule: an album is selected by wide passes from 16384 short-term blocks on (key 2 = 0), always (2) or never
    (1); a wide counting pass gives every workgroup at least 4096 values and uses 256 workgroups at most; the wide albums
    of a call are taken 64 at a time and their selection states never hold more than 64 x 203264 bytes."""
    form = capi.rg_r128_album_select_form
    assert [form(0, n) for n in (0, 1, 16383, 16384, 16385, 1 << 31)] == [1, 1, 1, 2, 2, 2]
    assert [form(1, n) for n in (0, 16383, 16384, 1 << 31)] == [1, 1, 1, 1]
    assert [form(2, n) for n in (0, 1, 16383, 16384)] == [2, 2, 2, 2]
    wgs = capi.rg_r128_albums_count_workgroups
    assert [wgs(n) for n in (0, 1, 4096, 4097, 16384, 21000, 256 * 4096, 256 * 4096 + 1, 1 << 31)] == [1, 1, 1, 1, 4, 5, 256, 256, 256]
    for n in (1, 4097, 16384, 21000, 69029, 1 << 20, (1 << 31) - 1):  # the workgroups' chunks cover the album, none is empty
        w = wgs(n)
        chunk = -(-n // w)
        assert chunk * w >= n > chunk * (w - 1) and (n < 4096 or n - chunk * (w - 1) >= 4096 or w == 256)
    b = C.c_size_t()
    state = 203264
    for albums, rounds, held in ((0, 0, 0), (1, 1, 1), (63, 1, 63), (64, 1, 64), (65, 2, 64), (128, 2, 64), (129, 3, 64), (10000, 157, 64)):
        assert capi.rg_r128_albums_wide_rounds(albums, C.byref(b)) == rounds and b.value == held * state, albums
    assert capi.rg_r128_albums_wide_rounds(5, None) == 1
