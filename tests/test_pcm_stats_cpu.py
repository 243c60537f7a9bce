"""The PCM defect scan without a GPU (include/mp3rgain_amd_stats.h): the serial host twin (route 0) and the kernels' chunking
and fold arithmetic run on the host (route 2) against the numpy restatement of the definitions (tests/pcm_stats_cases.py), field
for field and with == everywhere, the two routes byte for byte against each other, the argument checks, and tracks that alias and
abut between full-scale and NaN guard samples.  tests/test_gpu_pcm_stats.py holds the kernels (route 1) to the same cases."""
import ctypes as C
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import arena_layouts as al  # noqa: E402
import pcm_stats_cases as pc  # noqa: E402

from mp3rgain_amd import _capi  # noqa: E402
from mp3rgain_amd import replaygain as rg  # noqa: E402

RG_ERR_INVALID_ARG, RG_ERR_FORMAT = -1, -9


def _raw(recs):
    return b"".join(bytes(r) for r in recs)


def test_record_layout(capi):
    assert C.sizeof(_capi.PcmStatsChannel) == 72 and C.sizeof(_capi.PcmStatsRecord) == 48 + 8 * 72
    assert _capi.PcmStatsRecord.ch.offset == 48 and _capi.PcmStatsChannel.nonfinite.offset == 68 and _capi.PcmStatsChannel.or_mask.offset == 24


def test_kernel_shape_is_usable(capi):
    c, t, f = pc.shape()
    assert c >= 4 and t % c == 0 and t > 4 * c and f >= 2
    assert pc.long_length() > (2 * f + 2) * t and pc.long_length() * 4 < 8 << 20  # a few MB at the most


def test_the_restatement_on_a_plane_worked_by_hand():
    """16-bit: + + 0 - - - q 0 0 q 0 with q quiet -> the numbers counted by hand, so that the oracle itself is pinned."""
    x = np.array([32767, 32767, 0, -32768, -32768, -32768, 5, 0, 0, 7, 0], np.int16)
    w = pc.want_plane(x, 16, 3, 2)
    assert (w["clipped"], w["clip_runs"], w["longest_clip_run"], w["first_clip_run"]) == (5, 1, 3, 3)
    assert (w["zeros"], w["lead_zeros"], w["trail_zeros"], w["zero_runs"], w["longest_zero_run"]) == (4, 0, 1, 1, 2)
    assert (w["min"], w["max"], w["sum"], w["or_mask"], w["effective_bits"]) == (-32768.0, 32767.0, 2 * 32767 - 3 * 32768 + 12, 0xFFFF, 16)
    w = pc.want_plane(x, 16, 1, 1)
    assert (w["clip_runs"], w["first_clip_run"], w["zero_runs"]) == (2, 0, 2)
    w = pc.want_plane(np.array([0.0, -0.0, 1.0, np.nan, 1.0, 300.0, 0.5 / (1 << 23), 1.5 / (1 << 23)], np.float32), 32, 1, 1)
    assert (w["lead_zeros"], w["clip_runs"], w["longest_clip_run"], w["nonfinite"], w["max"]) == (2, 2, 2, 1, 300.0)
    assert w["sum"] == 2 * (1 << 23) + 256 * (1 << 23) + 0 + 2  # 0.5 -> 0 and 1.5 -> 2: half to even


@pytest.mark.parametrize("opts", pc.OPTIONS, ids=lambda o: f"{o[0]}-{o[1]}")
def test_host_routes_match_the_restatement(capi, opts):
    """Every case, field by field, from an arena with loud guards around sample-aligned tracks; routes 0 and 2 byte-identical."""
    tracks, wants = pc.tracks(), pc.wants(opts)
    arena, descs, guards = al.pack(tracks, al.Layout("guard", "loud", "input", 3))
    descs = list(descs)[:len(tracks)]
    assert any(d.offset_bytes % 16 for d in descs) and guards
    raws = []
    for route in (0, 2):
        out = rg.pcm_stats_arena(None, route, descs, pc.bits_of(tracks), arena, *opts)
        bad = [(tr.name, pc.differences(pc.got(r), wants[tr.name])) for tr, r in zip(tracks, out) if pc.differences(pc.got(r), wants[tr.name])]
        assert not bad, f"route {route}: {len(bad)} of {len(tracks)} records differ from the restatement: {bad[:3]}"
        raws.append(_raw(out))
    assert raws[0] == raws[1]


def test_options_null_is_the_default_and_bits_null_is_the_width(capi):
    tracks = [tr for tr in pc.tracks() if tr.bits in (16, 32) and len(tr.channels[0]) < 100]
    arena, descs, _ = al.pack(tracks, al.Layout("abut", "loud", "input"))
    descs = list(descs)[:len(tracks)]
    a = rg.pcm_stats_arena(None, 0, descs, None, arena)
    b = rg.pcm_stats_arena(None, 0, descs, pc.bits_of(tracks), arena, _capi.STATS_MIN_CLIP_RUN, _capi.STATS_MIN_ZERO_RUN)
    assert _raw(a) == _raw(b) and (_capi.STATS_MIN_CLIP_RUN, _capi.STATS_MIN_ZERO_RUN) == pc.OPTIONS[1]


def test_the_cases_show_every_flag_and_every_boundary(capi):
    """The case list does what it says: every flag appears and is absent somewhere, and stretches do cross chunks and tiles."""
    c, t, f = pc.shape()
    w = pc.wants(pc.OPTIONS[1])
    for flag in (_capi.STATS_CLIPPED, _capi.STATS_DROPOUT, _capi.STATS_PADDED, _capi.STATS_NONFINITE, _capi.STATS_SILENT):
        assert any(v["flags"] & flag for v in w.values()) and any(not v["flags"] & flag for v in w.values()), flag
    assert w[f"int32_b24_padded16_{t + 1}"]["flags"] & _capi.STATS_PADDED and w[f"int32_b24_padded16_{t + 1}"]["ch"][0]["effective_bits"] == 16
    big = pc.long_length()
    assert w[f"float32_clip_three_{big}"]["ch"][0]["longest_clip_run"] == 3 * t + 2
    assert w[f"int16_b12_zero_three_{big}"]["ch"][0]["trail_zeros"] == big - 6 * t and w[f"int16_b12_zero_three_{big}"]["ch"][0]["longest_zero_run"] == 3 * t + 2
    assert any(v["ch"][0]["longest_clip_run"] == 3 * c + 2 for k, v in w.items() if "clip_three" in k)
    assert {v["channels"] for v in w.values()} == {1, 2, 6, 8}


@pytest.mark.parametrize("layout", [al.Layout("abut", "loud", "reversed"), al.Layout("guard", "nan", "aliased", 5), al.Layout("abut", "loud", "aliased")],
                         ids=lambda l: f"{l.gap}-{l.guard}-{l.order}")
def test_aliased_and_abutting_tracks_between_guards(capi, layout):
    """Tracks that share one copy of their PCM, abut, or sit between full-scale / NaN guard samples: every descriptor gets the
    record of its own planes, and rewriting the guards changes no byte."""
    c, t, f = pc.shape()
    picked = [tr for tr in pc.tracks() if len(tr.channels[0]) in (1, c - 1, c + 1, t + 1) and len(tr.channels) <= 2]
    tracks = picked + picked[::3] if layout.order == "aliased" else picked  # (aliased: the same objects again share their bytes)
    wants = pc.wants(pc.OPTIONS[1])
    arena, descs, guards = al.pack(tracks, layout)
    descs = list(descs)[:len(tracks)]
    raws = []
    for route in (0, 2):
        out = rg.pcm_stats_arena(None, route, descs, pc.bits_of(tracks), arena)
        bad = [(tr.name, pc.differences(pc.got(r), wants[tr.name])) for tr, r in zip(tracks, out) if pc.differences(pc.got(r), wants[tr.name])]
        assert not bad, f"route {route}: {bad[:3]}"
        raws.append(_raw(out))
    assert raws[0] == raws[1]
    if guards:
        other = arena.copy()
        for a, b in guards:
            other[a:b] ^= 0x5A
        assert _raw(rg.pcm_stats_arena(None, 2, descs, pc.bits_of(tracks), other)) == raws[0]


def test_argument_errors(capi):
    L = _capi.load()
    arena = np.zeros(64, dtype=np.uint8)
    out = (_capi.PcmStatsRecord * 1)()
    d = (_capi.TrackDesc * 1)(_capi.TrackDesc(0, 16, 44100, 2, _capi.FMT_S16_PLANAR))
    S16, S32, F32 = _capi.FMT_S16_PLANAR, _capi.FMT_S32_PLANAR, _capi.FMT_F32_PLANAR
    for route in (0, 2):
        assert L.rg_pcm_stats_arena(None, route, 1, d, None, None, arena.ctypes.data, 64, out) == 0
        assert L.rg_pcm_stats_arena(None, route, 1, None, None, None, arena.ctypes.data, 64, out) == RG_ERR_INVALID_ARG
        assert L.rg_pcm_stats_arena(None, route, 1, d, None, None, arena.ctypes.data, 64, None) == RG_ERR_INVALID_ARG
        assert L.rg_pcm_stats_arena(None, route, 1, d, None, None, None, 64, out) == RG_ERR_INVALID_ARG
        assert L.rg_pcm_stats_arena(None, route, 0, None, None, None, None, 0, None) == 0
        for desc, bits, code, text in ((_capi.TrackDesc(0, 17, 44100, 2, S16), 16, RG_ERR_INVALID_ARG, "beyond the arena"),
                                       (_capi.TrackDesc(2, 16, 44100, 2, S16), 16, RG_ERR_INVALID_ARG, "beyond the arena"),
                                       (_capi.TrackDesc(66, 0, 44100, 1, S16), 16, RG_ERR_INVALID_ARG, "beyond the arena"),
                                       (_capi.TrackDesc(0, 9, 44100, 2, F32), 32, RG_ERR_INVALID_ARG, "beyond the arena"),
                                       (_capi.TrackDesc(1, 4, 44100, 2, S16), 16, RG_ERR_INVALID_ARG, "sample-aligned"),
                                       (_capi.TrackDesc(2, 4, 44100, 2, S32), 24, RG_ERR_INVALID_ARG, "sample-aligned"),
                                       (_capi.TrackDesc(6, 4, 44100, 2, F32), 0, RG_ERR_INVALID_ARG, "sample-aligned"),
                                       (_capi.TrackDesc(0, 4, 44100, 2, S16), 0, RG_ERR_INVALID_ARG, "0 bits"),
                                       (_capi.TrackDesc(0, 4, 44100, 2, S16), 17, RG_ERR_INVALID_ARG, "17 bits"),
                                       (_capi.TrackDesc(0, 4, 44100, 2, S32), 33, RG_ERR_INVALID_ARG, "33 bits"),
                                       (_capi.TrackDesc(0, 1, 44100, 9, S16), 16, RG_ERR_FORMAT, "9 channel"),
                                       (_capi.TrackDesc(0, 1, 44100, 0, S16), 16, RG_ERR_FORMAT, "0 channel"),
                                       (_capi.TrackDesc(0, 1, 44100, 2, 3), 16, RG_ERR_FORMAT, "format 3"),
                                       (_capi.TrackDesc(0, 1 << 32, 44100, 2, S16), 16, RG_ERR_FORMAT, "2^32")):
            with pytest.raises(rg.ReplayGainError) as e:
                rg.pcm_stats_arena(None, route, [desc], [bits], arena)
            assert e.value.code == code and text in str(e.value), (desc.frames, desc.channels, bits, str(e.value))
        for opts in ((0, 64), (3, 0), (0, 0)):
            with pytest.raises(rg.ReplayGainError) as e:
                rg.pcm_stats_arena(None, route, list(d), [16], arena, *opts)
            assert e.value.code == RG_ERR_INVALID_ARG and "at least 1" in str(e.value)
        # float ignores bits, whatever they say, and reports 0
        r = rg.pcm_stats_arena(None, route, [_capi.TrackDesc(0, 8, 44100, 2, F32)], [99], arena)[0]
        assert (r.status, r.bits, r.flags) == (0, 0, _capi.STATS_SILENT | _capi.STATS_COMPLETE)
    assert L.rg_pcm_stats_arena(None, 1, 1, d, None, None, arena.ctypes.data, 64, out) == RG_ERR_INVALID_ARG  # the kernels need a context
    assert L.rg_pcm_stats_arena(None, 3, 1, d, None, None, arena.ctypes.data, 64, out) == RG_ERR_INVALID_ARG
    # a track may end at the arena's last byte, and 8 channels are taken
    r = rg.pcm_stats_arena(None, 0, [_capi.TrackDesc(0, 4, 44100, 8, S16)], [16], arena)[0]
    assert (r.channels, r.lead_silence_frames, r.trail_silence_frames, r.ch[7].zeros) == (8, 4, 4, 4)
