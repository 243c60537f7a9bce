"""The checks the four PCM scans share (mp3rgain_amd/csrc/rg_pcm_plane.h), through the host routes of their test seams
(rg_pcm_stats_arena, rg_spectrum_arena, rg_dr_arena, rg_ancestry_arena; route 0 and route 2 take no context): a descriptor
that is wrong in one way gives exactly this code and this text, one that is wrong in two ways reports the check that comes
first, and what just fits the arena passes with the same record on both routes.  No GPU."""
import numpy as np
import pytest

import mp3rgain_amd as rg
from mp3rgain_amd import _capi

RG_ERR_INVALID_ARG, RG_ERR_FORMAT = -1, -9
S16, S32, F32 = _capi.FMT_S16_PLANAR, _capi.FMT_S32_PLANAR, _capi.FMT_F32_PLANAR
ARENA = np.zeros(64, dtype=np.uint8)
GOOD = _capi.TrackDesc(0, 4, 44100, 2, S16)  # track 0 of every call: the track under test is track 1


# name -> (the seam as f(route, descs, arena, **its own arguments) -> records, how its texts name it)
SCANS = {
    "stats": (lambda route, descs, arena, bits=None: rg.pcm_stats_arena(None, route, descs, bits, arena), "pcm stats take"),
    "spectrum": (lambda route, descs, arena: rg.spectrum_arena(None, route, descs, arena, bands=False)[0], "the spectrum takes"),
    "dr": (lambda route, descs, arena: rg.dr_arena(None, route, descs, arena), "the dynamic range takes"),
    "ancestry": (lambda route, descs, arena: rg.ancestry_arena(None, route, descs, arena, counts=False)[0], "the ancestry scan takes"),
}
BEYOND = (RG_ERR_INVALID_ARG, "track 1: its planes reach beyond the arena (64 bytes)")


def wrong_in_one_way(takes):
    """(descriptor, code, text) of track 1 in the 64-byte arena"""
    return (
        (_capi.TrackDesc(0, 4, 44100, 2, 7), RG_ERR_FORMAT, "track 1: format 7 is not a planar PCM format"),
        (_capi.TrackDesc(0, 4, 44100, 0, S16), RG_ERR_FORMAT, f"track 1: 0 channel(s), {takes} 1 to 8"),
        (_capi.TrackDesc(0, 4, 44100, 9, S16), RG_ERR_FORMAT, f"track 1: 9 channel(s), {takes} 1 to 8"),
        (_capi.TrackDesc(0, 2 ** 32, 44100, 2, S16), RG_ERR_FORMAT, f"track 1: 4294967296 frames, {takes} fewer than 2^32"),
        (_capi.TrackDesc(1, 4, 44100, 2, S16), RG_ERR_INVALID_ARG, "track 1: offset 1 is not sample-aligned"),
        (_capi.TrackDesc(2, 4, 44100, 2, S32), RG_ERR_INVALID_ARG, "track 1: offset 2 is not sample-aligned"),
        (_capi.TrackDesc(2, 4, 44100, 2, F32), RG_ERR_INVALID_ARG, "track 1: offset 2 is not sample-aligned"),
        (_capi.TrackDesc(66, 0, 44100, 2, S16), *BEYOND),   # offset_bytes > arena_bytes
        (_capi.TrackDesc(0, 17, 44100, 2, S16), *BEYOND),   # 2 x 17 x 2 bytes: one sample per plane too many
        (_capi.TrackDesc(32, 5, 44100, 2, S32), *BEYOND),   # 32 + 2 x 5 x 4
        (_capi.TrackDesc(4, 8, 44100, 2, F32), *BEYOND),    # 4 + 2 x 8 x 4: the last plane ends one sample past the arena
        (_capi.TrackDesc(62, 2, 44100, 1, S16), *BEYOND),   # one plane, its last sample past the arena
    )


def refusal(call, route, desc, **more):
    with pytest.raises(rg.ReplayGainError) as e:
        call(route, [GOOD, desc], ARENA, **more)
    return e.value.code, str(e.value)


@pytest.mark.parametrize("route", (0, 2))
@pytest.mark.parametrize("scan", SCANS)
def test_a_descriptor_wrong_in_one_way(scan, route):
    call, takes = SCANS[scan]
    for desc, code, text in wrong_in_one_way(takes):
        assert refusal(call, route, desc) == (code, text), (desc.offset_bytes, desc.frames, desc.channels, desc.format)


@pytest.mark.parametrize("route", (0, 2))
def test_stats_report_the_bits_before_the_place(route):
    call, _ = SCANS["stats"]
    misaligned = _capi.TrackDesc(1, 4, 44100, 2, S16)
    for bits in (0, 17):
        assert refusal(call, route, misaligned, bits=[16, bits]) == (RG_ERR_INVALID_ARG, f"track 1: {bits} bits in a 16-bit container")
    # ... and the format before the bits
    assert refusal(call, route, _capi.TrackDesc(1, 4, 44100, 9, S16), bits=[16, 0]) == (RG_ERR_FORMAT, "track 1: 9 channel(s), pcm stats take 1 to 8")
    # a float track has no bits to be wrong: the place is what is left
    assert refusal(call, route, _capi.TrackDesc(2, 4, 44100, 2, F32), bits=[16, 0]) == (RG_ERR_INVALID_ARG, "track 1: offset 2 is not sample-aligned")


@pytest.mark.parametrize("route", (0, 2))
def test_dr_reports_the_block_before_the_place(route):
    call, _ = SCANS["dr"]
    for rate, block in ((0, 0), (384001, 1152003)):  # a block is three seconds; 1 .. RG_DR_MAX_BLOCK_FRAMES = 1152000 are taken
        assert refusal(call, route, _capi.TrackDesc(1, 4, rate, 2, S16)) == (
            RG_ERR_INVALID_ARG, f"track 1: a block of {block} frames (sample rate {rate}) is not in 1 .. 1152000")
    # ... and the format before the block
    assert refusal(call, route, _capi.TrackDesc(1, 2 ** 32, 0, 2, S16)) == (
        RG_ERR_FORMAT, "track 1: 4294967296 frames, the dynamic range takes fewer than 2^32")


@pytest.mark.parametrize("scan", SCANS)
def test_what_just_fits_passes_alike_on_both_routes(scan):
    call, _ = SCANS[scan]
    arena = np.arange(1, 9, dtype=np.uint8)  # 8 bytes, none of them zero
    descs = [_capi.TrackDesc(4, 1, 44100, 2, S16),   # one frame of two channels whose last byte is the arena's last
             _capi.TrackDesc(8, 0, 44100, 2, S16)]   # no frames, at the arena's end
    serial, folded = call(0, descs, arena), call(2, descs, arena)
    assert [(r.status, r.frames, r.channels, r.format) for r in serial] == [(0, 1, 2, S16), (0, 0, 2, S16)]
    assert [bytes(r) for r in serial] == [bytes(r) for r in folded]
    if scan == "stats":  # the samples read are the arena's last four bytes
        assert [(c.min, c.max) for c in serial[0].ch[:2]] == [(0x0605, 0x0605), (0x0807, 0x0807)]
