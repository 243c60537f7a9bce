"""The cases of the batched FLAC decode tests (tests/flac_batch_cases.py) on the host alone, before a GPU sees them: the host
decoder returns exactly the PCM each case expects and drops exactly the frames it names, and it takes every fuzz variant.

And the CPU twin of the device decoder's output stage (rg_flac_decode_arena): the shared frame code writing, and for the
stereo decorrelations reading back, through the arena sink the decode kernel uses -- 16-bit planes with a left shift for
every stream of up to 16 bits per sample -- against the encoder's input in the arena's format."""
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent))
import flac_batch_cases as fb  # noqa: E402
import flacenc as fe  # noqa: E402

from mp3rgain_amd import flacdec  # noqa: E402

O = fe.Options


def _first_difference(got, want):
    """(channel, sample, got, want) of the first differing sample, or a note on the shapes."""
    if len(got) != len(want):
        return f"{len(got)} planes, want {len(want)}"
    for c, (g, w) in enumerate(zip(got, want)):
        if g.shape != w.shape or g.dtype != w.dtype:
            return f"channel {c}: {g.dtype}{g.shape}, want {w.dtype}{w.shape}"
        bad = np.flatnonzero(g != w)
        if len(bad):
            return f"channel {c} sample {int(bad[0])}: got {int(g[bad[0]])}, want {int(w[bad[0]])} ({len(bad)} differ)"
    return None


def _host_exact(cases):
    for case in cases:
        rate, bps, out, info = flacdec.decode(case.data)
        assert (rate, bps, int(info.channels)) == (case.rate, case.bps, case.channels), case.name
        assert info.dropped_frames == case.dropped, case.name
        assert out.dtype == np.int32
        diff = _first_difference(list(out), [c.astype(np.int32) for c in case.pcm])
        assert diff is None, f"{case.name}: {diff}"


def test_matrix_cases_decode_to_their_input(capi):
    assert len(fb.matrix_cases()) == 53
    _host_exact(fb.matrix_cases())


def test_extremes_cases_decode_to_their_input(capi):
    cases = fb.extremes_cases()
    assert len(cases) == 7 * 4 * 4 * 4 + 3 * 4 * 4  # the grid of 448, and the wasted-bits noise for 12, 16 and 24 bits
    # the signals are what they claim: the rails are reached, the side channel of `alt` needs all of its bps + 1 bits
    for case in cases:
        hi, lo = (1 << (case.bps - 1)) - 1, -(1 << (case.bps - 1))
        if not case.name.endswith("noise_wasted"):
            assert case.pcm.min() == lo and (case.pcm.max() == hi or case.name.endswith("-min")), case.name
        if case.name.endswith("-alt"):
            side = case.pcm[0] - case.pcm[1]
            assert side.max() == (1 << case.bps) - 1 and side.min() == -((1 << case.bps) - 1), case.name
    _host_exact(cases)


def test_many_frames_cases_decode_to_their_input(capi):
    cases = fb.many_frames_cases()
    _host_exact(cases)
    frames = {c.name: int(flacdec.index(c.data)[1].audio_frames) for c in cases}
    assert frames == {"mono16_300x192": 300, "one_sample": 1, "ms12_600x64": 600, "hundred_samples": 1, "stereo24_130x256": 130,
                      "variable": 6, "one_frame": 1, "no_frame": 0}
    assert [c.pcm.shape[1] for c in cases] == [57600, 1, 38400, 100, 33280, 10000, 4096, 0]


def test_damage_cases_decode_to_their_input_without_the_damaged_blocks(capi):
    cases = fb.damage_cases()
    _host_exact(cases)
    by_name = {c.name: c for c in cases}
    assert by_name["mono16_300x192-flip270-reserved140"].dropped == 2 and by_name["ms12_600x64-truncated_last"].dropped == 1
    assert by_name["mono16_300x192-flip270-reserved140"].pcm.shape[1] == 298 * 192
    assert by_name["ms12_600x64-truncated_last"].pcm.shape[1] == 599 * 64
    assert set(fb.TRUNCATED) <= set(by_name)
    for case in cases:
        assert flacdec.selfcheck(case.data) == 0, case.name


def test_host_decoder_takes_every_fuzz_variant(capi):
    streams = fb.fuzz_streams()
    assert len(streams) == fb.FUZZ_VARIANTS == 256
    damaged = 0
    for name, data in streams:
        _, _, out, info = flacdec.decode(data)  # raises if the decoder refuses the stream
        assert out.shape[1] == info.frames, name
        damaged += info.dropped_frames > 0
    # every flip or deletion lands in a frame and breaks its CRC-16 (or takes its header, and the frame before it then fails)
    assert damaged > len(streams) // 2


# ---- the CPU twin of the narrow sink --------------------------------------------------------------------------------------
def _arena_exact(name, data, pcm, bps):
    got, info = flacdec.decode_arena(data)
    assert info.dropped_frames == 0, name
    diff = _first_difference(got, fb.to_planes(pcm, bps))
    assert diff is None, f"{name}: {diff}"


def test_arena_sink_matrix(capi):
    for case in fb.matrix_cases():
        _arena_exact(case.name, case.data, case.pcm, case.bps)


def test_arena_sink_extremes(capi):
    for case in fb.extremes_cases():
        _arena_exact(case.name, case.data, case.pcm, case.bps)


def test_arena_sink_damage(capi):
    """Dropped frames: the plane stride is the decoded length, as on the device."""
    for case in fb.damage_cases():
        got, info = flacdec.decode_arena(case.data)
        assert info.dropped_frames == case.dropped, case.name
        diff = _first_difference(got, fb.planes(case))
        assert diff is None, f"{case.name}: {diff}"


def test_arena_sink_random_settings(capi):
    """The 200 settings of test_flacdec.test_random_settings (the same generator, draw for draw)."""
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
        _arena_exact(f"setting {k} {opt}", fe.encode(pcm, 44100, bps, opt), pcm, bps)


def test_arena_sink_reports_a_small_capacity(capi):
    import ctypes as C

    case = fb.matrix_cases()[1]
    L = flacdec._lib()
    info, eb = flacdec.FlacInfo(), C.c_uint32()
    buf = np.zeros(16, dtype=np.uint8)
    rc = L.rg_flac_decode_arena(flacdec._buf(case.data), len(case.data), buf.ctypes.data, buf.size, C.byref(eb), C.byref(info))
    assert rc == flacdec.ERR_CAPACITY and info.frames == case.pcm.shape[1] and eb.value == 2
    assert not buf.any()
