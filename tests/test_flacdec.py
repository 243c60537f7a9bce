"""The host FLAC decoder (include/mp3rgain_amd_flac.h) against the test encoder's input: every feature of the format,
random encoder settings, damaged streams (index / decoder agreement), STREAMINFO."""
import sys
import zlib
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import flacenc as fe  # noqa: E402

from mp3rgain_amd import flacdec  # noqa: E402

O = fe.Options

# (name, options, channels, bps, rate, samples)
MATRIX = [
    ("constant", O(subframe="constant"), 1, 16, 44100, 5000),
    ("verbatim", O(subframe="verbatim"), 2, 16, 44100, 5000),
    *[(f"fixed{o}", O(subframe="fixed", order=o), 2, 16, 44100, 9000) for o in range(5)],
    ("fixed_auto", O(subframe="auto", stereo="alternate"), 2, 16, 48000, 20000),
    *[(f"lpc{o}", O(subframe="lpc", order=o, precision=p, shift=s), 2, 16, 44100, 9000)
      for o, p, s in [(1, 15, 14), (2, 8, 5), (5, 12, 9), (8, 12, 10), (12, 15, 13), (13, 13, 11), (20, 14, 12), (32, 15, 13)]],
    ("lpc_shift0", O(order=4, precision=4, shift=0), 1, 16, 44100, 5000),
    ("rice2_escape", O(rice2=True, escape_every=2, partition_order=3), 2, 24, 96000, 9000),
    ("escape_rice", O(escape_every=1, partition_order=0), 1, 16, 44100, 3000),
    ("porder8", O(partition_order=8, block_size=4096), 2, 16, 44100, 12000),
    ("no_wasted", O(wasted=False), 2, 16, 44100, 5000),
    ("left_side", O(stereo="left_side"), 2, 16, 44100, 9000),
    ("right_side", O(stereo="right_side"), 2, 16, 44100, 9000),
    ("mid_side", O(stereo="mid_side"), 2, 16, 44100, 9000),
    ("mid_side24", O(stereo="mid_side"), 2, 24, 48000, 9000),
    ("right_side8", O(stereo="right_side", subframe="fixed", order=2), 2, 8, 22050, 5000),
    ("six_channels", O(), 6, 16, 48000, 6000),
    ("eight_channels", O(subframe="fixed", order=1), 8, 12, 32000, 3000),
    ("bps4", O(subframe="fixed", order=1), 1, 4, 8000, 3000),
    ("bps12", O(), 2, 12, 16000, 5000),
    ("bps20", O(), 2, 20, 88200, 5000),
    ("bps_streaminfo", O(ss_code="streaminfo"), 2, 16, 44100, 5000),
    ("bps17", O(), 1, 17, 44100, 5000),
    ("rate_streaminfo", O(rate_code="streaminfo"), 2, 16, 44100, 5000),
    ("rate_khz", O(rate_code="khz"), 2, 16, 64000, 5000),
    ("rate_hz", O(rate_code="hz"), 2, 16, 11025, 5000),
    ("rate_dahz", O(rate_code="dahz"), 2, 16, 12000, 5000),
    ("bs_explicit8", O(bs_code="explicit8", block_size=200), 2, 16, 44100, 3001),
    ("bs_explicit16", O(bs_code="explicit16", block_size=3000), 2, 16, 44100, 10001),
    *[(f"bs{b}", O(block_size=b, order=4), 1, 16, 44100, 3 * b + 7) for b in (192, 576, 1152, 2304, 4608, 256, 512, 1024, 2048, 8192, 16384, 32768)],
    ("variable", O(variable=True, blocks=[100, 4096, 1, 576, 2000, 3227]), 2, 16, 44100, 10000),
    ("noise16", O(), 2, 16, 44100, 5000),
]


def _pcm(name, ch, bps, n):
    rng = np.random.default_rng(zlib.crc32(name.encode()))  # the same PCM in every process
    kind = "noise" if name.startswith("noise") else "music"
    pcm = fe.test_pcm(rng, ch, n, bps, kind)
    if name == "constant":
        pcm[:] = -3 << 4
    if name in ("fixed2", "lpc5"):  # wasted bits
        pcm = (pcm >> 3) << 3
    return pcm


@pytest.mark.parametrize("name,opt,ch,bps,rate,n", MATRIX, ids=[m[0] for m in MATRIX])
def test_matrix_exact(capi, name, opt, ch, bps, rate, n):
    pcm = _pcm(name, ch, bps, n)
    data = fe.encode(pcm, rate, bps, opt)
    got_rate, got_bps, out, info = flacdec.decode(data)
    assert (got_rate, got_bps, int(info.channels)) == (rate, bps, ch)
    assert info.dropped_frames == 0
    assert np.array_equal(out, pcm)
    assert flacdec.selfcheck(data) == 0


def test_random_settings(capi):
    rng = np.random.default_rng(0xF1AC)
    for k in range(200):
        ch = int(rng.choice([1, 2, 2, 2, 3, 6]))
        bps = int(rng.choice([8, 12, 16, 16, 20, 24]))
        n = int(rng.integers(1, 6000))
        sub = str(rng.choice(["constant", "verbatim", "fixed", "lpc", "lpc", "auto"]))
        order = int(rng.integers(0, 5)) if sub == "fixed" else int(rng.integers(1, 33))
        prec = int(rng.integers(5, 16))
        opt = O(block_size=int(rng.choice([192, 256, 576, 1024, 1152, 4096])), subframe=sub, order=order, precision=prec,
                shift=int(rng.integers(0, min(prec, 15) + 1)), rice2=bool(rng.integers(2)), partition_order=int(rng.integers(0, 6)),
                escape_every=int(rng.choice([0, 0, 1, 3])), wasted=bool(rng.integers(2)),
                stereo=str(rng.choice(["independent", "left_side", "right_side", "mid_side", "alternate"])),
                variable=bool(rng.integers(2)))
        pcm = fe.test_pcm(rng, ch, n, bps, "noise" if k % 7 == 0 else "music")
        if k % 5 == 0:
            pcm = (pcm >> 2) << 2
        data = fe.encode(pcm, 44100, bps, opt)
        _, _, out, info = flacdec.decode(data)
        assert info.dropped_frames == 0, (k, opt)
        assert np.array_equal(out, pcm), (k, opt)


def test_scan_streaminfo(capi):
    pcm = fe.test_pcm(np.random.default_rng(3), 2, 10000, 20)
    data = fe.id3v2_tag(77) + fe.encode(pcm, 96000, 20, O(block_size=1152))
    info = flacdec.scan(data)
    assert (info.sample_rate, info.channels, info.bits_per_sample) == (96000, 2, 20)
    assert (info.min_block_size, info.max_block_size, info.total_samples) == (1152, 1152, 10000)
    assert info.id3v2_bytes == 87
    frames, ii = flacdec.index(data)
    assert len(frames) == ii.audio_frames == 9 and ii.frames == 10000
    assert [f.first_sample for f in frames] == [1152 * k for k in range(9)]
    assert flacdec.is_flac(data) and not flacdec.is_flac(b"RIFF....WAVE")
    with pytest.raises(flacdec.FlacError):
        flacdec.scan(b"not a flac stream at all")


def test_unsupported_bps(capi):
    pcm = fe.test_pcm(np.random.default_rng(4), 1, 1000, 28)
    data = fe.encode(pcm, 44100, 28, O(subframe="verbatim"))
    assert flacdec.scan(data).bits_per_sample == 28
    with pytest.raises(flacdec.FlacError) as e:
        flacdec.decode(data)
    assert e.value.code == flacdec.ERR_UNSUPPORTED


damaged_variants = fe.damaged_variants
DAMAGED = [d[0] for d in damaged_variants()]


@pytest.mark.parametrize("case", range(len(DAMAGED)), ids=DAMAGED)
def test_damaged(capi, case):
    name, data, want, dropped = damaged_variants()[case]
    _, _, out, info = flacdec.decode(data)
    assert np.array_equal(out, want), name
    assert info.dropped_frames == dropped, name
    assert flacdec.selfcheck(data) == 0


def test_selfcheck_fuzz(capi):
    rng = np.random.default_rng(0xDA7A)
    bases = []
    for k in range(8):
        bps = [8, 16, 24][k % 3]
        pcm = fe.test_pcm(rng, int(rng.choice([1, 2])), int(rng.integers(500, 9000)), bps)
        opt = O(block_size=int(rng.choice([256, 1152, 4096])), stereo="alternate", subframe=str(rng.choice(["lpc", "auto"])))
        bases.append(fe.encode(pcm, 44100, bps, opt))
    bad = 0
    for k in range(2000):
        b = bytearray(bases[k % len(bases)])
        for _ in range(int(rng.integers(1, 6))):
            at = int(rng.integers(0, len(b)))
            kind = int(rng.integers(3))
            if kind == 0:
                b[at] ^= 1 << int(rng.integers(8))
            elif kind == 1:
                b[at:at] = bytes(rng.integers(0, 256, int(rng.integers(1, 20)), dtype=np.uint8))
            else:
                del b[at:at + int(rng.integers(1, 50))]
        rc = flacdec.selfcheck(bytes(b))
        assert rc in (0, -2, -4), (k, rc)
        bad += rc != 0
    assert bad < 2000
