"""The null-test kernels (mp3rgain_amd/csrc/rg_compare.hip) keep a lane's vectors, its sums, its window of the b side and its lag
accumulators out of scratch: compiled for gfx950 here (hipcc cross-compiles without a GPU), every kernel descriptor of the file
shows no private segment and no dynamic stack, and the instantiations the launcher uses are there."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def test_compare_kernels_use_no_scratch(tmp_path):
    if not Path(HIPCC).exists():
        pytest.skip("no hipcc")
    out = tmp_path / "rg_compare.s"
    subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S",
                    str(ROOT / "mp3rgain_amd" / "csrc" / "rg_compare.hip"), "-o", str(out)], check=True, capture_output=True, timeout=600)
    kernels = re.findall(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", out.read_text(), re.S)
    assert sum("rg_cmp_moments_kernel" in k for k, _ in kernels) == 3
    for name in ("rg_cmp_lags_kernel", "rg_cmp_mixed_kernel", "rg_cmp_fold_kernel"):
        assert any(name in k for k, _ in kernels), name
    for name, body in kernels:
        m = re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", body)
        assert m and int(m.group(1)) == 0, name
        assert re.search(r"\.amdhsa_uses_dynamic_stack 0", body), name
