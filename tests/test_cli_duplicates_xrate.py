"""`--dup-any-rate` of the command line (mp3rgain_amd/cli.py) without a GPU: the option is parsed, belongs to --duplicates, and
--dup-radius is then converted at 46.4 ms per code; without it nothing about --duplicates changes."""
import io

import pytest

from mp3rgain_amd import _capi, cli


def _parse(*args):
    return cli.parse_args(list(args), io.StringIO(), io.StringIO())


def test_the_option_is_parsed_and_needs_duplicates():
    o = _parse("--duplicates", "--dup-any-rate", "--dup-radius", "2", "a.wav", "b.flac")
    assert o.duplicates and o.dup_any_rate and o.dup_radius == 2.0
    assert not _parse("--duplicates", "a.wav").dup_any_rate
    with pytest.raises(cli.CliError) as e:
        _parse("--dup-any-rate", "a.wav")
    assert "--dup-any-rate requires --duplicates" in str(e.value)


def test_the_radius_is_converted_at_the_common_rate():
    assert cli.dup_radius_codes(5.94) == 512 and cli.dup_radius_codes(5.94, _capi.RS_RATE_OUT) == 128 == _capi.XR_RADIUS
    assert cli.dup_radius_codes(2.0, _capi.RS_RATE_OUT) == round(2.0 * 11025 / 512)
    _parse("--duplicates", "--dup-radius", "23", "a.wav")  # 1981 codes at 44.1 kHz
    _parse("--duplicates", "--dup-any-rate", "--dup-radius", "90", "a.wav")  # 1938 codes of 46.4 ms
    with pytest.raises(cli.CliError) as e:
        _parse("--duplicates", "--dup-any-rate", "--dup-radius", "96", "a.wav")  # 2067 codes: beyond the match kernel's 2047
    assert "--dup-any-rate" in str(e.value)
    with pytest.raises(cli.CliError):
        _parse("--duplicates", "--dup-radius", "24", "a.wav")
