"""The FLAC encoder on the GPU (include/mp3rgain_amd_flacenc.h): the analyse, layout and write kernels through their seam
(rg_flac_encode_arena, route 1) on the shared cases (tests/flacenc_cases.py), byte for byte against the serial host twin (route
0), which tests/test_flacenc_cpu.py holds to its input and to the sizes the format gives.  One call per group of cases (the block
size and max_lpc_order are options of the call), so streams of every shape are mixed in one launch of each kernel; the same
bytes through the device decoder give the input back."""
import sys
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import flacenc_cases as fc  # noqa: E402

pytestmark = pytest.mark.gpu

_routes = {}


def routes(ctx, gname):
    """(route 1, route 0) of a group, computed once."""
    if gname not in _routes:
        g = next(g for g in fc.groups() if g.name == gname)
        arena, descs, bps = fc.packed(gname)
        _routes[gname] = (ctx.flac_encode_arena(1, descs, bps, arena, g.block, g.lpc), ctx.flac_encode_arena(0, descs, bps, arena, g.block, g.lpc))
    return _routes[gname]


@pytest.mark.parametrize("group", fc.groups(), ids=lambda g: g.name)
def test_kernels_match_the_host_twin_byte_for_byte(_ctx, group):
    (dev, drec, doffs), (host, hrec, hoffs) = routes(_ctx, group.name)
    assert doffs == hoffs
    differing = [(c.name, len(a), len(b), next((k for k in range(min(len(a), len(b))) if a[k] != b[k]), None))
                 for c, a, b in zip(group.cases, dev, host) if a != b]
    assert not differing, f"{len(differing)} of {len(group.cases)} streams differ (name, sizes, first differing byte): {differing[:5]}"
    assert [bytes(r) for r in drec] == [bytes(r) for r in hrec]


@pytest.mark.parametrize("group", fc.groups(), ids=lambda g: g.name)
def test_device_decoder_returns_the_input(_ctx, group):
    (dev, _, _), _ = routes(_ctx, group.name)
    for c, s in zip(group.cases, dev):
        pcm, info = _ctx.decode_flac_device(s)
        assert info.dropped_frames == 0 and np.array_equal(pcm, c.pcm), c.name


def test_the_same_call_twice_and_in_another_layout(_ctx):
    g = next(g for g in fc.groups() if g.name == "b256_lpc12")
    want = routes(_ctx, g.name)[0][0]
    for shift in (0, 3):
        arena, descs, bps = fc.packed(g.name, shift)
        assert _ctx.flac_encode_arena(1, descs, bps, arena, g.block, g.lpc)[0] == want
