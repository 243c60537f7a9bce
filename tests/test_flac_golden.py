"""The committed FLAC fixtures (tests/golden/flac, tools/make_flac_golden.py): every stream decodes to the PCM whose
sha256 is recorded, with the recorded number of dropped frames -- on the host and on the device -- and every undamaged
stream was decoded to the same PCM by an independent decoder (ffmpeg's, recorded as "ffmpeg_equal")."""
import hashlib
import json
from pathlib import Path

import numpy as np
import pytest

from mp3rgain_amd import flacdec

GOLD = Path(__file__).resolve().parent / "golden" / "flac"
EXPECTED = json.loads((GOLD / "expected.json").read_text())
NAMES = sorted(EXPECTED)


def _sha(pcm) -> str:
    return hashlib.sha256(np.ascontiguousarray(np.asarray(pcm, dtype="<i4")).tobytes()).hexdigest()


def test_fixtures_cover_the_matrix():
    rec = EXPECTED.values()
    assert {r["bps"] for r in rec} >= {8, 12, 16, 20, 24}
    assert {r["channels"] for r in rec} >= {1, 2, 6}
    assert {r["rate"] for r in rec} >= {96000, 88200, 64000, 48000, 44100, 32000, 24000, 22050, 16000, 12000, 11025, 8000, 192000}
    undamaged = [n for n in NAMES if not n.startswith("damaged_")]
    assert len(undamaged) >= 15 and all(EXPECTED[n]["ffmpeg_equal"] is True for n in undamaged)


@pytest.mark.parametrize("name", NAMES)
def test_host_decodes_fixture(capi, name):
    r = EXPECTED[name]
    rate, bps, pcm, info = flacdec.decode((GOLD / f"{name}.flac").read_bytes())
    assert (rate, bps, pcm.shape) == (r["rate"], r["bps"], (r["channels"], r["samples"]))
    assert info.dropped_frames == r["dropped"]
    assert _sha(pcm) == r["sha256"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_device_decodes_fixture(_ctx, name):
    r = EXPECTED[name]
    pcm, info = _ctx.decode_flac_device((GOLD / f"{name}.flac").read_bytes())
    assert pcm.shape == (r["channels"], r["samples"]) and info.dropped_frames == r["dropped"]
    assert _sha(pcm) == r["sha256"]
