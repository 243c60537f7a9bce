"""The EBU R 128 kernels (mp3rgain_amd/csrc/rg_r128.hip) compile for gfx950, use no scratch memory and no dynamic stack
(read from the kernel descriptors; hipcc cross-compiles without a GPU), and the pure helpers of
include/mp3rgain_amd_r128.h need no context."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def test_r128_kernels_use_no_scratch(tmp_path):
    if not Path(HIPCC).exists():
        pytest.skip("no hipcc")
    out = tmp_path / "rg_r128.s"
    subprocess.run([HIPCC, "-O3", "-std=c++17", "-Wno-missing-braces", "--offload-arch=gfx950", "--cuda-device-only", "-S",
                    str(ROOT / "mp3rgain_amd" / "csrc" / "rg_r128.hip"), "-o", str(out)], check=True, capture_output=True, timeout=1500)
    isa = out.read_text()
    kernels = re.findall(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", isa, re.S)
    names = [k for k, _ in kernels]
    for want, count in (("rg_r128_main_kernel", 3), ("rg_r128_gate_kernel", 1), ("rg_r128_truepeak_kernel", 6)):
        assert sum(want in k for k in names) == count, (want, names)
    for name, body in kernels:
        m = re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", body)
        assert m and int(m.group(1)) == 0, name
        assert re.search(r"\.amdhsa_uses_dynamic_stack 0", body), name
    # plain vector stores and vector atomics only: no floating-point atomics (results must not depend on scheduling)
    assert not re.search(r"atomic_(add|pk_add|fadd|fmax|fmin)_f", isa)


def test_r128_helpers_need_no_context(capi):
    assert capi.rg_r128_supported_rate(44100) == 1
    assert capi.rg_r128_block_count(44100, 4410 * 10) == 7
    assert capi.rg_r128_design_info(44100, None, None, None, None, None, None) == 0
