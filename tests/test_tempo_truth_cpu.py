"""The tempo scan against the tempo its material was generated at (include/mp3rgain_amd_tempo.h): click tracks and a kick /
snare / hat pattern (tests/tempo_cases.py), 40 s each, at 44100 and 48000 Hz and nine tempi, through the kernels' arithmetic on
the host (rg_tempo_arena route 2) at the defaults.  Every reading within 2 % of the generating tempo (the nearest wrong
candidates, 3:2 and 2:1, are off by a third or more) and within twice the largest error tools/tempo_refcheck.py recorded for
the float64 restatement (tests/golden/tempo_measured.json; route 2's f32 onsets are not the tool's); 60, 170 and 200 BPM read
120, 85 and 100 (the octave convention); white noise reads a confidence below half of the lowest recorded for the rhythmic
material.  Synthetic material only: nothing here says anything about real music.  No GPU."""
import sys
from pathlib import Path

import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import tempo_cases as tc  # noqa: E402

import mp3rgain_amd as rg  # noqa: E402
from mp3rgain_amd import _capi  # noqa: E402


def _read(planes, rate):
    arena, descs = tc.pack([tc.Case("x", [planes], rate)])
    return rg.tempo_arena(None, 2, descs, arena, bands=False)[0][0]


@pytest.mark.parametrize("kind,rate,bpm", tc.truth_cases(), ids=lambda v: str(v))
def test_reading_is_the_generating_tempo(kind, rate, bpm):
    m = tc.measured()
    r = _read(tc.truth_planes(kind, rate, bpm), rate)
    got = r.bpm_milli / 1000.0
    print(f"{kind} {rate} {bpm}: {got} BPM, confidence {r.confidence_permille}, stable {r.stable_permille}, first beat {r.first_beat}")
    assert r.flags == _capi.TEMPO_COMPLETE and r.harmonics == 8 and r.windows == (r.onsets - 2048) // 256 + 1
    assert abs(got - bpm) / bpm <= 0.02
    assert abs(got - bpm) / bpm <= 2 * m["relative_error_max"]
    assert r.stable_permille == 1000 and r.confidence_permille >= m["confidence_min"] // 2
    # the beat grid: coarse, but within the spread the tool recorded around the constant, and a few hops
    period = r.period16 * 32
    off = (tc.FIRST_BEAT * rate - r.first_beat + period / 2) % period - period / 2
    assert abs(off) <= max(m["click_offset_max"] - m["beat_bias"], m["beat_bias"] - m["click_offset_min"]) + 512, off


@pytest.mark.parametrize("bpm,want", tc.OCTAVE_BPMS)
@pytest.mark.parametrize("rate", tc.TRUTH_RATES)
def test_the_octave_convention(bpm, want, rate):
    r = _read(tc.fc.as_format(tc.click_track(bpm, rate) * 32768.0 * 0.9, "s16"), rate)
    assert abs(r.bpm_milli / 1000.0 - want) / want <= 0.02, r.bpm_milli
    assert 80000 <= r.bpm_milli < 160000


@pytest.mark.parametrize("rate", tc.TRUTH_RATES)
def test_white_noise_reads_a_low_confidence(rate):
    r = _read(tc.white_noise(rate), rate)
    print(f"white noise {rate}: confidence {r.confidence_permille}")
    assert r.confidence_permille < tc.measured()["confidence_min"] / 2
