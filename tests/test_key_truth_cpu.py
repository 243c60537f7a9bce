"""The key scan against material whose key is known (tests/key_cases.py: chord progressions I-IV-V-I-vi-IV-V-I with a bass
root, six harmonics, a scale-tone melody and a little noise, 40 s each): all 24 keys at 44100, 48000 and 96000 Hz through the
kernels' arithmetic on the host (rg_key_arena route 2) must read their generating key -- a condition, not a measurement --
with correlation, margin and stability inside the ranges tools/key_refcheck.py recorded; white noise correlates weakly and
digital silence has no key.  No GPU."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import key_cases as kc  # noqa: E402

import mp3rgain_amd as rg  # noqa: E402
from mp3rgain_amd import _capi  # noqa: E402

SLACK = 20  # per mille: what the recorded ranges are widened by, as the refcheck's margin


def _reading(planes, rate):
    arena, descs = kc.pack([kc.Case("x", [planes], rate)])
    return rg.key_arena(None, 2, descs, arena, bands=False)[0][0]


@pytest.mark.parametrize("rate", kc.TRUTH_RATES)
def test_every_key_reads_its_generating_key(rate):
    m = kc.measured()
    for key in range(24):
        r = _reading(kc.truth_planes(rate, key), rate)
        assert (r.key, r.tonic, r.mode, r.flags) == (key, key % 12, key // 12, _capi.KEY_COMPLETE), (rate, rg.key_name(key), rg.key_name(r.key))
        assert m["readings"][f"{rate}_{key}"][0] == rg.key_name(key)
        assert m[f"correlation_min_{rate}"] - SLACK <= r.correlation_permille <= min(1000, m[f"correlation_max_{rate}"] + SLACK)
        assert m["margin_min"] - SLACK <= r.margin_permille <= m["margin_max"] + SLACK
        assert r.stable_permille >= m["stable_min"] and r.segments == 3 and r.decim == rate // 5000
    assert m["right"] == m["cases"] == 72


def test_noise_correlates_weakly_and_silence_has_no_key():
    m = kc.measured()
    for rate in kc.TRUTH_RATES[:2]:
        r = _reading(kc.white_noise(rate), rate)
        assert m["noise_correlation_min"] - 2 * SLACK <= r.correlation_permille <= m["noise_correlation_max"] + 2 * SLACK
        assert r.correlation_permille < min(m[f"correlation_min_{x}"] for x in kc.TRUTH_RATES) - 300
    r = _reading(np.zeros(44100 * 10, np.int16), 44100)
    assert r.flags == m["silence_flags"] == _capi.KEY_COMPLETE | _capi.KEY_NONE and r.silent_rows == r.rows > 0
