"""The FLAC device kernels (mp3rgain_amd/csrc/rg_flacdev.hip) use no scratch memory: compiled for gfx950 here
(hipcc cross-compiles without a GPU) and read from the kernel descriptors."""
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def test_flac_kernels_use_no_scratch(tmp_path):
    if not Path(HIPCC).exists():
        pytest.skip("no hipcc")
    out = tmp_path / "rg_flacdev.s"
    subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "--cuda-device-only", "-S",
                    str(ROOT / "mp3rgain_amd" / "csrc" / "rg_flacdev.hip"), "-o", str(out)], check=True, capture_output=True, timeout=1500)
    isa = out.read_text()
    kernels = re.findall(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", isa, re.S)
    names = {k for k, _ in kernels}
    for want in ("rg_flac_check_kernel", "rg_flac_layout_kernel", "rg_flac_decode_kernel"):
        assert any(want in k for k in names), want
    for name, body in kernels:
        m = re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", body)
        assert m and int(m.group(1)) == 0, name
        assert re.search(r"\.amdhsa_uses_dynamic_stack 0", body), name
