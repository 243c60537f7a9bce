"""The loudness-range kernels (mp3rgain_amd/csrc/rg_r128_range.hip) compile for gfx950, use no scratch memory and no dynamic
stack (read from the kernel descriptors; hipcc cross-compiles without a GPU) and no floating-point atomics, and the library
exports the entry points of include/mp3rgain_amd_r128.h."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def test_range_kernels_use_no_scratch(tmp_path):
    if not Path(HIPCC).exists():
        pytest.skip("no hipcc")
    out = tmp_path / "rg_r128_range.s"
    subprocess.run([HIPCC, "-O3", "-std=c++17", "-Wno-missing-braces", "--offload-arch=gfx950", "--cuda-device-only", "-S",
                    str(ROOT / "mp3rgain_amd" / "csrc" / "rg_r128_range.hip"), "-o", str(out)], check=True, capture_output=True, timeout=1500)
    isa = out.read_text()
    kernels = re.findall(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", isa, re.S)
    names = [k for k, _ in kernels]
    for want in ("rg_r128r_blocks_kernel", "rg_r128r_select_kernel"):
        assert sum(want in k for k in names) == 1, (want, names)
    assert len(kernels) == 2, names
    for name, body in kernels:
        m = re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", body)
        assert m and int(m.group(1)) == 0, name
        assert re.search(r"\.amdhsa_uses_dynamic_stack 0", body), name
        lds = re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", body)
        assert lds and int(lds.group(1)) <= 64 * 1024, name
    # integer atomics only (the maxima are an integer max on the bits of non-negative doubles): no floating-point atomics
    assert not re.search(r"atomic_(add|pk_add|fadd|fmax|fmin|max|min)_f", isa)
    assert re.search(r"atomic_u?max_(x2|u64)", isa)


def test_range_entry_points_are_exported(capi):
    import ctypes as C

    for name in ("rg_r128_short_term_count", "rg_r128_analyze_pcm_batch_dynamics", "rg_r128_analyze_album_pcm_dynamics",
                 "rg_r128_analyze_tracks_dynamics", "rg_r128_analyze_album_dynamics"):
        assert hasattr(capi, name), name
    assert capi.rg_r128_short_term_count(44100, 4410 * 40) == 11
    from mp3rgain_amd import _capi

    assert C.sizeof(_capi.R128Dynamics) == 48
