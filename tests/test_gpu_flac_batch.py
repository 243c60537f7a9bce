"""The batched FLAC decode of the file route, sample for sample: many streams through ONE call of the staging code a file
call runs (rg_flac_stage_device_batch: load_flac, stage_loaded, one rg_flacdev_decode for all of them), the arena brought
back and every plane compared with the encoder's input in the arena's format (tests/flac_batch_cases.py).  No tolerance
anywhere.  Streams of up to 16 bits per sample land in 16-bit planes through the shifting sink, every stream at its own
arena offset, frame lanes of different streams share waves and blocks; with tuning key 14 = 0 the same hook checks the host
decoder's repacking.  tests/test_flac_batch_cases_cpu.py proves the cases on the host alone."""
import sys
from collections import namedtuple
from pathlib import Path

import numpy as np
import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent))
import flac_batch_cases as fb  # noqa: E402

pytestmark = pytest.mark.gpu

FMT_S16, FMT_S32 = 1, 2  # rg_sample_format
Entry = namedtuple("Entry", "name data planes bps rate channels dropped")


@pytest.fixture(params=[1, 0], ids=["device", "host"])
def an(_ctx, request):
    _ctx.set_tuning(14, request.param)
    _ctx.set_tuning(10, 0)
    _ctx.set_decoder_command(None)
    yield _ctx
    _ctx.set_tuning(14, 1)
    _ctx.set_tuning(10, 0)


def _entry(case):
    return Entry(case.name, case.data, fb.planes(case), case.bps, case.rate, case.channels, case.dropped)


def _first_difference(got, want):
    for c, (g, w) in enumerate(zip(got, want)):
        bad = np.flatnonzero(g != w)
        if len(bad):
            return f"first difference at channel {c} sample {int(bad[0])}: got {int(g[bad[0]])}, want {int(w[bad[0]])} ({len(bad)} samples of the plane differ)"
    return None


def _stage_and_check(an, entries):
    """One call for all `entries`; every descriptor, count and plane against the expectation.  -> the planes it found."""
    arena, descs, infos = an.stage_flac_device([e.data for e in entries])
    assert len(descs) == len(infos) == len(entries)
    end, found = 0, []
    for i, (e, d, info) in enumerate(zip(entries, descs, infos)):
        where = f"stream {i} ({e.name})"
        eb, dt, fmt = (2, np.int16, FMT_S16) if e.bps <= 16 else (4, np.int32, FMT_S32)
        frames = len(e.planes[0])
        assert d.offset_bytes % 16 == 0, where
        assert d.offset_bytes >= end, f"{where}: starts at {d.offset_bytes}, inside the stream before it (ends at {end})"
        assert d.format == fmt, where
        assert (d.channels, d.sample_rate, d.frames) == (e.channels, e.rate, frames), where
        assert (info.channels, info.sample_rate, info.bits_per_sample, info.frames) == (e.channels, e.rate, e.bps, frames), where
        assert info.dropped_frames == e.dropped, where
        end = d.offset_bytes + e.channels * frames * eb
        assert end <= arena.size, where
        got = [arena[d.offset_bytes + c * frames * eb:d.offset_bytes + (c + 1) * frames * eb].view(dt) for c in range(e.channels)]
        diff = _first_difference(got, e.planes)
        assert diff is None, f"{where}: {diff}"
        found.append(got)
    return found, infos


def _report(test, route, streams, infos):
    print(f"{test}[key14={route}]: {streams} streams, {sum(int(i.audio_frames) + int(i.dropped_frames) for i in infos)} frames walked")


def test_matrix_in_one_batch(an, request):
    """Every stream of the host decoder's matrix in one call, in list order and reversed: widths 4-24, 1-8 channels and
    predictor orders mix within waves, and every destination but the first is an offset into the arena."""
    entries = [_entry(c) for c in fb.matrix_cases()]
    for order in (entries, entries[::-1]):
        _, infos = _stage_and_check(an, order)
    _report("matrix", request.node.callspec.id, 2 * len(entries), list(infos) * 2)


def test_extremes(an, request):
    """Full scale (both rails, a side channel that needs all of its bps + 1 bits, constant minimum, white noise, wasted
    bits) x width x channel assignment x coding; a failure names them: bps<width>-<stereo>-<coding>-<signal>."""
    entries = [_entry(c) for c in fb.extremes_cases()]
    assert len(entries) == 496
    all_infos = []
    for at in range(0, len(entries), 62):  # 8 calls of 62 streams
        _, infos = _stage_and_check(an, entries[at:at + 62])
        all_infos += infos
    _report("extremes", request.node.callspec.id, len(entries), all_infos)


def test_many_frames_and_block_boundaries(an, request):
    """Streams of 300, 600 and 130 frames with one-frame, one-sample and frameless streams between them: the 128-lane decode
    blocks and the 256-lane check blocks end inside streams and between them, and the layout kernel's 256-wide scan makes
    three trips over the 600-frame stream."""
    entries = [_entry(c) for c in fb.many_frames_cases()]
    for order in (entries, entries[::-1]):
        _, infos = _stage_and_check(an, order)
    _report("many_frames", request.node.callspec.id, 2 * len(entries), list(infos) * 2)


def test_damage_inside_a_batch(an, request):
    """Every damaged stream between two good ones, all in one call: the damaged stream equals the input without exactly
    the damaged blocks, the neighbours are exact.  Behind a stream whose last frame is cut short the blob goes on with the
    next stream's bytes (the host's reader sees zeros there): the verdict is the same."""
    good = [_entry(c) for c in fb.fuzz_bookends()]
    damaged = [_entry(c) for c in fb.damage_cases()]
    assert {e.name for e in damaged} >= set(fb.TRUNCATED)
    entries = [good[0]]
    for k, e in enumerate(damaged):
        entries += [e, good[(k + 1) % 2]]
    _, infos = _stage_and_check(an, entries)
    assert sum(int(i.dropped_frames) for i in infos) == sum(e.dropped for e in damaged) == 2 + 1 + 4
    _report("damage", request.node.callspec.id, len(entries), infos)


def test_fuzz_in_batches(an, request):
    """256 damaged variants, 32 per call between two undamaged streams.  The one test whose reference is the host decoder
    (planes and dropped counts of flacdec.decode, in the arena's format): it is about the batch machinery, not the frame
    code.  No variant may be left out."""
    from mp3rgain_amd import flacdec

    first, last = [_entry(c) for c in fb.fuzz_bookends()]
    entries, skipped = [], 0
    for name, data in fb.fuzz_streams():
        try:
            rate, bps, host, hi = flacdec.decode(data)
        except flacdec.FlacError:
            skipped += 1
            continue
        entries.append(Entry(name, data, fb.to_planes(host, bps), bps, rate, int(hi.channels), int(hi.dropped_frames)))
    assert skipped == 0 and len(entries) == 256
    all_infos = []
    for at in range(0, len(entries), 32):
        _, infos = _stage_and_check(an, [first] + entries[at:at + 32] + [last])
        all_infos += infos
    _report("fuzz", request.node.callspec.id, len(entries) + 2 * 8, all_infos)
    print(f"fuzz: {skipped} variants skipped")


def test_single_stream_hook_agrees(an):
    """The one-stream hook (right-justified int32, offset 0) and the batch hook see the same PCM."""
    cases = fb.many_frames_cases()
    found, _ = _stage_and_check(an, [_entry(c) for c in cases])
    for case, planes in zip(cases, found):
        dev, info = an.decode_flac_device(case.data)
        assert info.dropped_frames == 0, case.name
        diff = _first_difference(fb.to_planes(dev, case.bps), planes)
        assert diff is None and len(dev) == len(planes) and dev.shape[1] == len(planes[0]), f"{case.name}: {diff}"
