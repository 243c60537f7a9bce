"""EBU R 128 path, CPU side: the host design (K-weighting coefficients at any rate, hop, block count, true-peak factor)
against the BS.1770 table and against the checker; the checker itself (tests/r128ref.py) against the EBU Tech 3341 signals;
the command line's --r128 switch, and its output without the switch on the fixtures of tests/test_cli.py."""
import ctypes as C
import io
import json
import math
import shutil
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import r128ref  # noqa: E402

FIX = Path(__file__).parent / "golden" / "fixtures"
RATES = [8000, 11025, 22050, 44100, 96000, 176400, 192000, 384000]


def _design(capi, rate):
    b1, a1, b2, a2 = ((C.c_double * 3)() for _ in range(4))
    hop, fac = C.c_uint32(), C.c_uint32()
    rc = capi.rg_r128_design_info(rate, b1, a1, b2, a2, C.byref(hop), C.byref(fac))
    return rc, list(b1), list(a1), list(b2), list(a2), hop.value, fac.value


def test_design_48k_is_the_bs1770_table(capi):
    rc, b1, a1, b2, a2, hop, fac = _design(capi, 48000)
    assert rc == 0
    assert np.allclose(b1, [1.53512485958697, -2.69169618940638, 1.19839281085285], rtol=0, atol=1e-13)
    assert np.allclose(a1, [1.0, -1.69065929318241, 0.73248077421585], rtol=0, atol=1e-13)
    assert b2 == [1.0, -2.0, 1.0]
    assert np.allclose(a2, [1.0, -1.99004745483398, 0.99007225036621], rtol=0, atol=1e-13)
    assert (hop, fac) == (4800, 4)


@pytest.mark.parametrize("rate", RATES)
def test_design_equals_the_checker(capi, rate):
    rc, b1, a1, b2, a2, hop, fac = _design(capi, rate)
    assert rc == 0
    (rb1, ra1), (rb2, ra2) = r128ref.coefficients(rate)
    for got, want in ((b1, rb1), (a1, ra1), (b2, rb2), (a2, ra2)):
        for g, w in zip(got, want):
            assert abs(g - float(w)) <= 1e-14 * abs(float(w)), (rate, got, list(want))
    assert hop == r128ref.hop_frames(rate) == (rate + 5) // 10
    assert fac == r128ref.tp_factor(rate)
    for frames in (0, hop - 1, 3 * hop - 1, 3 * hop, 4 * hop - 1, 4 * hop, 4 * hop + 1, 5 * hop, 100 * hop + 7):
        assert capi.rg_r128_block_count(rate, frames) == r128ref.block_count(rate, frames) == max(frames // hop - 3, 0)


def test_supported_rates(capi):
    assert [capi.rg_r128_supported_rate(r) for r in (7999, 8000, 384000, 384001)] == [0, 1, 1, 0]
    assert _design(capi, 7999)[0] == -2 and _design(capi, 384001)[0] == -2
    assert capi.rg_r128_block_count(7999, 1 << 20) == 0


# ---- the checker against EBU Tech 3341 ---------------------------------------------------------------------------------
@pytest.mark.parametrize("rate", [44100, 48000, 96000, 192000])
@pytest.mark.parametrize("name,segments,want", r128ref.TECH3341_LOUDNESS, ids=[c[0] for c in r128ref.TECH3341_LOUDNESS])
def test_checker_tech3341_loudness(rate, name, segments, want):
    got = r128ref.analyze(r128ref.sine_segments(rate, segments), rate)["loudness_lufs"]
    print(f"{name} at {rate} Hz: {got:.4f} LUFS, expected {want}")
    assert abs(got - want) <= 0.1


def test_checker_997hz_one_channel():
    x = np.sin(2.0 * np.pi * 997.0 * np.arange(20 * 48000) / 48000.0)
    got = r128ref.analyze([x, np.zeros_like(x)], 48000)["loudness_lufs"]
    print(f"997 Hz, 0 dBFS, one channel: {got:.4f} LUFS")
    assert abs(got - (-3.01)) <= 0.05


@pytest.mark.parametrize("rate", [22050, 44100, 48000, 96000])
@pytest.mark.parametrize("name,div,phase,amp", r128ref.TECH3341_TRUEPEAK, ids=[c[0] for c in r128ref.TECH3341_TRUEPEAK])
def test_checker_tech3341_truepeak(rate, name, div, phase, amp):
    x = r128ref.truepeak_signal(rate, div, phase, amp)
    got = 20.0 * math.log10(r128ref.true_peak([x], rate))
    want = 20.0 * math.log10(amp)
    print(f"{name} at {rate} Hz: {got:.3f} dBTP, expected {want:.3f}")
    assert -0.4 <= got - want <= 0.2


def test_checker_edges():
    assert r128ref.analyze([np.zeros(48000 * 2)], 48000)["loudness_lufs"] == -math.inf
    r = r128ref.analyze([0.5 * np.ones(14400, dtype=np.float32)], 48000)  # 300 ms: no block
    assert r["loudness_lufs"] == -math.inf and r["gain_db"] == 0.0 and r["blocks"] == 0
    x = np.ones(48000, dtype=np.float32)
    x[100] = np.nan
    x[200] = np.inf
    r = r128ref.analyze([x], 48000, True)
    assert math.isnan(r["loudness_lufs"]) and r["sample_peak"] == 1.0 and math.isfinite(r["true_peak"])
    # the true peak is at least the sample peak: phase 0 of the interpolator is the identity
    y = np.random.default_rng(1).uniform(-1, 1, 5000)
    assert r128ref.true_peak([y], 44100) >= r128ref.sample_peak([y]) * (1 - 1e-12)


# ---- command line -------------------------------------------------------------------------------------------------------
def _run(*args):
    from mp3rgain_amd import cli

    out, err = io.StringIO(), io.StringIO()
    rc = cli.main([str(a) for a in args], out, err)
    return rc, out.getvalue(), err.getvalue()


def test_cli_parses_r128():
    from mp3rgain_amd import cli

    o = cli.parse_args(["--r128", "--true-peak", "-r", "a.mp3"], io.StringIO(), io.StringIO())
    assert o.r128 and o.true_peak and o.track_gain and [str(f) for f in o.files] == ["a.mp3"]
    o = cli.parse_args(["-r", "a.mp3"], io.StringIO(), io.StringIO())
    assert not o.r128 and not o.true_peak
    rc, out, _ = _run("--help")
    assert rc == 0 and "--r128" in out and "--true-peak" in out


def test_cli_without_r128_is_unchanged(tmp_path, monkeypatch):
    """The byte-level commands on the fixtures of tests/test_cli.py print what they printed before the switch existed
    (tests/golden/cli_before_r128.json, recorded from the parent revision by the same command list)."""
    gold = json.loads((Path(__file__).parent / "golden" / "cli_before_r128.json").read_text())
    monkeypatch.chdir(tmp_path)
    for entry in gold:
        for f in ("test_joint_stereo.mp3", "test_stereo.mp3", "test_mono.mp3"):
            if (FIX / f).exists():
                shutil.copyfile(FIX / f, tmp_path / f)
        rc, out, err = _run(*entry["args"])
        assert (rc, out, err) == (entry["rc"], entry["out"], entry["err"]), entry["args"]
