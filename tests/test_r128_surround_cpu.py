"""BS.1770 channel weights of the EBU R 128 path, the parts that need no GPU: the layout rule (rg_r128_layout_weights)
against its restatement in tests/r128surround_ref.py, the channel mode's validation, the checker itself on EBU Tech 3341
case 6, the Python and command-line surface, and the fold kernel's translation unit (mp3rgain_amd/csrc/rg_r128_surround.hip):
it compiles for gfx950, uses no scratch memory, no dynamic stack and no floating-point atomics."""
import ctypes as C
import io
import re
import shutil
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import r128ref  # noqa: E402
import r128surround_ref as sref  # noqa: E402

ROOT = Path(__file__).resolve().parent.parent
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"


def _weights(capi, channels, mask=0):
    from mp3rgain_amd import _capi

    w = _capi.R128ChannelWeights()
    assert capi.rg_r128_layout_weights(channels, mask, C.byref(w)) == 0
    return [w.w[i] for i in range(8)]


def test_layout_defaults_follow_the_flac_channel_order(capi):
    want = {1: [1.0], 2: [1.0, 1.0], 3: [1.0, 1.0, 1.0], 4: [1.0, 1.0, 1.41, 1.41], 5: [1.0, 1.0, 1.0, 1.41, 1.41],
            6: [1.0, 1.0, 1.0, 0.0, 1.41, 1.41], 7: [1.0, 1.0, 1.0, 0.0, 1.0, 1.41, 1.41],
            8: [1.0, 1.0, 1.0, 0.0, 1.0, 1.0, 1.41, 1.41]}
    for n, w in want.items():
        got = _weights(capi, n)
        assert got[:n] == w and got[n:] == [0.0] * (8 - n), (n, got)
        assert sref.layout_weights(n) == w
        assert _weights(capi, n, sref.DEFAULT_MASK[n]) == got


def test_layout_masks(capi):
    cases = [
        (6, 0x3F, [1.0, 1.0, 1.0, 0.0, 1.41, 1.41]),   # FL FR FC LFE BL BR: the backs stand in for the surrounds
        (6, 0x60F, [1.0, 1.0, 1.0, 0.0, 1.41, 1.41]),  # FL FR FC LFE SL SR
        (8, 0x63F, [1.0, 1.0, 1.0, 0.0, 1.0, 1.0, 1.41, 1.41]),  # 7.1: sides 1.41, backs 1.0
        (7, 0x70F, [1.0, 1.0, 1.0, 0.0, 1.0, 1.41, 1.41]),       # 6.1: FL FR FC LFE BC SL SR
        (2, 0x600, [1.41, 1.41]),
        (1, 0x8, [0.0]),
    ]
    for n, mask, w in cases:
        assert _weights(capi, n, mask)[:n] == w, hex(mask)
        assert sref.layout_weights(n, mask) == w, hex(mask)
    # a mask whose population count is not the channel count: the default of the count
    assert _weights(capi, 6, 0x60F | 0x30) == _weights(capi, 6)
    assert _weights(capi, 5, 0x3F) == _weights(capi, 5)
    assert _weights(capi, 2, 0x4) == _weights(capi, 2)
    # bits above the named positions are positions like any other
    assert _weights(capi, 3, 0x80000003)[:3] == [1.0, 1.0, 1.0]


def test_layout_every_mask_agrees_with_the_restatement(capi):
    rng = np.random.default_rng(0x5A)
    for _ in range(400):
        n = int(rng.integers(1, 9))
        mask = int(rng.integers(0, 1 << 18))
        assert _weights(capi, n, mask)[:n] == sref.layout_weights(n, mask), (n, hex(mask))


def test_layout_refuses_other_counts(capi):
    from mp3rgain_amd import _capi

    import mp3rgain_amd as rg

    w = _capi.R128ChannelWeights()
    for n in (0, 9, 255):
        assert capi.rg_r128_layout_weights(n, 0, C.byref(w)) == _capi.RG_ERR_INVALID_ARG
        with pytest.raises(rg.ReplayGainError):
            rg.r128_layout_weights(n)
    assert capi.rg_r128_layout_weights(2, 0, None) == _capi.RG_ERR_INVALID_ARG
    assert rg.r128_layout_weights(6) == [1.0, 1.0, 1.0, 0.0, 1.41, 1.41]
    assert rg.r128_layout_weights(6, 0x60F) == rg.r128_layout_weights(6, mask=0x3F)


def test_set_channel_mode_validates(capi):
    from mp3rgain_amd import _capi

    assert capi.rg_r128_set_channel_mode(None, 0) == _capi.RG_ERR_INVALID_ARG
    assert (_capi.R128_CHANNELS_PAIR, _capi.R128_CHANNELS_LAYOUT) == (0, 1)
    header = (ROOT / "include" / "mp3rgain_amd_r128.h").read_text()
    assert re.search(r"#define RG_R128_CHANNELS_PAIR 0\b", header) and re.search(r"#define RG_R128_CHANNELS_LAYOUT 1\b", header)
    assert C.sizeof(_capi.R128ChannelWeights) == 64
    from mp3rgain_amd import replaygain

    assert replaygain._r128_mode("pair") == 0 and replaygain._r128_mode("layout") == 1
    with pytest.raises(ValueError):
        replaygain._r128_mode("stereo")


def test_pcm_track_carries_weights():
    import mp3rgain_amd as rg

    x = np.zeros(16, dtype=np.float32)
    assert rg.PcmTrack([x, x], 48000).channel_weights is None
    assert rg.PcmTrack([x, x, x], 48000, channel_weights=(1, 1, 0)).channel_weights == [1.0, 1.0, 0.0]
    with pytest.raises(ValueError):
        rg.PcmTrack([x], 48000, channel_weights=[1.0] * 9)


def test_cli_surround_needs_r128():
    from mp3rgain_amd import cli

    out, err = io.StringIO(), io.StringIO()
    assert cli.parse_args(["--r128", "--surround", "a.wav"], out, err).surround
    assert not cli.parse_args(["--r128", "a.wav"], out, err).surround
    with pytest.raises(cli.CliError):
        cli.parse_args(["--surround", "a.wav"], out, err)
    cli.print_usage(out)
    assert "--surround" in out.getvalue()


def test_checker_reads_tech3341_case6():
    """Guards the checker: the 5.0 sine of EBU Tech 3341 case 6 reads -23.0 +- 0.1 LUFS with the layout's weights, and about
    -28 as a stereo pair."""
    rate = 48000
    chans = sref.tech3341_case6(rate)
    got = sref.analyze(chans, rate, sref.layout_weights(5))
    pair = r128ref.analyze(chans, rate)
    print(f"case 6: {got['loudness_lufs']:.4f} LUFS weighted, {pair['loudness_lufs']:.4f} as a pair")
    assert abs(got["loudness_lufs"] - (-23.0)) <= 0.1
    assert abs(pair["loudness_lufs"] - (-28.0)) <= 0.1
    assert got["sample_peak"] == pytest.approx(10.0 ** (-24.0 / 20.0), rel=1e-6)  # the centre channel's


def test_checker_weights_of_one_are_the_pair():
    rate = 8000
    rng = np.random.default_rng(3)
    chans = [(0.2 * rng.standard_normal(2 * rate)).astype(np.float32) for _ in range(3)]
    a = sref.analyze(chans, rate, [1.0, 1.0, 0.0])
    b = r128ref.analyze(chans[:2], rate)
    assert np.array_equal(a["z"], b["z"]) and a["loudness_lufs"] == b["loudness_lufs"]
    assert a["sample_peak"] == max(float(np.abs(c).max()) for c in chans)
    zero = sref.analyze(chans, rate, [0.0, 0.0, 0.0])
    assert zero["loudness_lufs"] == -np.inf and zero["gain_db"] == 0.0 and not zero["z"].any() and zero["blocks"] == 17


def test_surround_kernel_uses_no_scratch(tmp_path):
    if not Path(HIPCC).exists():
        pytest.skip("no hipcc")
    out = tmp_path / "rg_r128_surround.s"
    subprocess.run([HIPCC, "-O3", "-std=c++17", "-Wno-missing-braces", "--offload-arch=gfx950", "--cuda-device-only", "-S",
                    str(ROOT / "mp3rgain_amd" / "csrc" / "rg_r128_surround.hip"), "-o", str(out)], check=True, capture_output=True, timeout=1500)
    isa = out.read_text()
    kernels = re.findall(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", isa, re.S)
    names = [k for k, _ in kernels]
    assert sum("rg_r128_fold_kernel" in k for k in names) == 1 and len(names) == 1, names
    for name, body in kernels:
        m = re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", body)
        assert m and int(m.group(1)) == 0, name
        assert re.search(r"\.amdhsa_uses_dynamic_stack 0", body), name
    # plain vector stores only: no atomics at all, and the weighted sum is not contracted into fused multiply-adds
    assert not re.search(r"atomic_(add|pk_add|fadd|fmax|fmin)_f", isa)
    assert not re.search(r"\b(global|flat|buffer|ds)_atomic", isa)
    assert "v_mul_f64" in isa and "v_add_f64" in isa and "v_fma_f64" not in isa


def test_rg1_headers_are_untouched(capi):
    """The feature lives in mp3rgain_amd_r128.h alone; the ABI version stays."""
    for name in ("rg_r128_layout_weights", "rg_r128_set_channel_mode", "rg_r128_analyze_pcm_weighted"):
        assert hasattr(capi, name), name
        for h in ("mp3rgain_amd.h", "mp3rgain_amd_node.h"):
            assert name not in (ROOT / "include" / h).read_text()
