"""Stage 2 of the duplicate finder on the CPU (include/mp3rgain_amd_fingerprint.h): the serial host twin
(rg_fingerprint_match_codes route 0) on the constructed codes of tests/fingerprint_cases.py, byte for byte against the numpy
restatement (fingerprint_cases.ref_match), and what each construction is there for: planted copies found with their exact error
counts, the radius, the probe rules, the ties, the skipped pairs, the groups.  No GPU."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import fingerprint_cases as fc  # noqa: E402

import mp3rgain_amd as rg  # noqa: E402
from mp3rgain_amd import _capi  # noqa: E402

COMPARED, MATCH, SKIPPED, PROBE_J = _capi.FP_PAIR_COMPARED, _capi.FP_PAIR_MATCH, _capi.FP_PAIR_SKIPPED, _capi.FP_PAIR_PROBE_J


def _host(mc):
    return rg.fingerprint_match_codes(None, 0, list(mc.codes), mc.rates, **mc.opts)


def _case(name):
    return next(mc for mc in fc.match_cases() if mc.name == name)


@pytest.mark.parametrize("mc", fc.match_cases(), ids=lambda mc: mc.name)
def test_host_twin_equals_the_numpy_restatement(mc):
    o = mc.opts
    want = fc.ref_match(list(mc.codes), mc.rates, o["block"], o["probes"], o["radius"], o["max_ber_permille"])
    got = _host(mc)
    assert got.dtype == want.dtype and got.tobytes() == want.tobytes(), (got.tolist(), want.tolist())


def test_planted_copies_are_found_with_their_exact_error_count():
    for lag in (0, 1, -1, 8, -8):  # 5 flipped bits inside the probe blocks (one of them in two blocks' overlap counts twice)
        assert _host(_case(f"lag{lag}")).tolist() == [(5, 3 * 32 * 32, lag, COMPARED | MATCH)]
    for lag in (9, -9):  # one beyond the radius: something unrelated is the best lag, and it is no match
        (r,) = _host(_case(f"lag{lag}")).tolist()
        assert r[3] == COMPARED and 1200 < r[0] < 1900 and abs(r[2]) <= 8
    assert _host(_case("ka_is_block")).tolist() == [(0, 3072, 4, COMPARED | MATCH)]  # all three probes are the one block
    assert _host(_case("kb_is_block")).tolist() == [(0, 3072, 0, COMPARED | MATCH)]
    assert _host(_case("probe_j")).tolist()[0][3] == COMPARED | PROBE_J
    assert _host(_case("one_probe")).tolist() == [(0, 1024, 3, COMPARED | MATCH)]


def test_a_lag_needs_half_the_probes():
    assert _host(_case("half_the_probes_lag40")).tolist() == [(0, 2 * 1024, 40, COMPARED | MATCH)]
    (r,) = _host(_case("half_the_probes_lag44")).tolist()  # only one probe of four would count there
    assert r[3] == COMPARED and r[2] != 44 and r[0] > 600


def test_ties_take_the_smaller_lag_then_the_negative():
    assert _host(_case("tie_all_lags")).tolist() == [(0, 3072, 0, COMPARED | MATCH)]
    assert _host(_case("tie_periodic")).tolist() == [(0, 3072, -2, COMPARED | MATCH)]  # 0 errors at +-2 and +-6


def test_skipped_pairs_and_small_calls():
    for name in ("rates_differ", "rate_unsupported", "short"):
        assert _host(_case(name)).tolist() == [(0, 0, 0, SKIPPED)], name
    assert len(_host(_case("n1"))) == 0 and len(_host(_case("n0"))) == 0
    assert rg.fingerprint_groups(1, _host(_case("n1")))[0].tolist() == [0]


def test_groups_join_chains():
    mc = _case("chain")
    rec = _host(mc)
    flags = rec["flags"].tolist()
    # (0,1) and (1,2) match, (0,2) does not; 3 is unrelated, 4 at another rate, 5 too short
    assert flags[0] & MATCH and flags[5] & MATCH and not flags[1] & MATCH and flags[1] & COMPARED
    assert all(f == SKIPPED for k, f in enumerate(flags) if k in (3, 4, 7, 8, 10, 11, 12, 13, 14))
    groups, matches, found = rg.fingerprint_groups(len(mc.codes), rec)
    assert groups.tolist() == [0, 0, 0, 3, 4, 5] and matches.tolist() == [1, 2, 1, 0, 0, 0] and found == 2


def test_options_are_checked_and_zero_is_the_default():
    a, b = fc.planted(300, 300, 0, 90)
    dflt = rg.fingerprint_match_codes(None, 0, [a, b], [44100, 44100])
    assert dflt.tolist() == [(0, 8 * 256 * 32, 0, COMPARED | MATCH)]
    assert rg.fingerprint_match_codes(None, 0, [a, b], [44100, 44100], 256, 8, 512, _capi.FP_MAX_BER_PERMILLE).tobytes() == dflt.tobytes()
    assert rg.fingerprint_match_codes(None, 0, [a, b], [44100, 44100], 0, 0, 0, 0).tobytes() == dflt.tobytes()
    for kw in (dict(block=4097), dict(probes=65), dict(radius=2048), dict(max_ber_permille=1001)):
        with pytest.raises(rg.ReplayGainError) as e:
            rg.fingerprint_match_codes(None, 0, [a, b], [44100, 44100], **kw)
        assert e.value.code == -1 and "fingerprint:" in str(e.value)
    with pytest.raises(rg.ReplayGainError):
        rg.fingerprint_match_codes(None, 2, [a, b], [44100, 44100])


def test_the_default_threshold_is_the_measured_midpoint():
    m = fc.measured()
    assert not m["overlap"] and m["wrong_lags"] == []
    assert m["same_recording_max_ber"] < m["unrelated_min_ber"]
    assert _capi.FP_MAX_BER_PERMILLE == m["max_ber_permille"] == round(1000 * (m["same_recording_max_ber"] + m["unrelated_min_ber"]) / 2)
    import re

    header = (fc.ROOT / "include" / "mp3rgain_amd_fingerprint.h").read_text()
    assert int(re.search(r"#define RG_FP_MAX_BER_PERMILLE (\d+)u", header).group(1)) == m["max_ber_permille"]
