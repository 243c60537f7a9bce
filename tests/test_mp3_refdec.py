"""The host MP3 decoder (rg_mp3dec.cpp) against a float64 reference decoder (oracle/mp3_refdec.py).

tests/test_mp3dec.py holds the decoder to ffmpeg's fixed-point decoder, whose int16 output is itself a step of 2^-15
from the truth: a synthesis-window tap off by one Q16 step, 1.33334 for 4/3, an alias coefficient or an IMDCT window
wrong in the third digit all pass there.  The device decoder is written to mirror the host one, so bit-identity of the
two cannot notice either.  Here the ARITHMETIC is pinned:

  a. the reference is right by something other than the library: it meets the ffmpeg bar on every golden stream, and
     it inverts the encoder's own forward transforms (MDCT: exactly, TDAC; polyphase filterbank: to the filterbank's
     own 84 dB);
  b. the host decoder is compared with it on the golden streams and the damaged test_stereo.mp3 (peaks of 6e8), on 63
     streams generated here (every rate row x every channel mode, block-type sequences, mixed blocks, sub-block gains,
     CRC, reservoir, linbits escapes, global_gain from 60 to 255: no int16 golden could hold those) and on one encode
     per MPEG version;
  c. in units of floor = reference(float32) - reference(float64): rms and max of the decoder's error within 4 floors over
     the stream and over every 576-sample block, exact zeros where the floor is zero (tools/mp3_refdec_check.py);
  d. every deliberate error of the reference (one digit of one table or constant, per stage) lands beyond that bar.

Measured (tools/mp3_refdec_check.py --record -> tests/golden/mp3_refdec_measured.json; nothing here reads that file):
stream rms 0.84-1.23, stream max <= 1.72, block rms <= 3.22 (a silent granule's filterbank tail; 1.8 elsewhere),
block max <= 2.87; the smallest perturbation is 10 floors in rms and 30 in max.  The module takes about 20 s.
"""
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
for _p in (ROOT, ROOT / "oracle", ROOT / "tools", ROOT / "tests"):
    if str(_p) not in sys.path:
        sys.path.insert(0, str(_p))

import make_mp3_golden as M  # noqa: E402
import mp3_bitstream as B  # noqa: E402
import mp3_encoder as E  # noqa: E402
import mp3_refdec as R  # noqa: E402
import mp3_refdec_check as C  # noqa: E402
import mp3gold  # noqa: E402
from mp3rgain_amd import mp3dec  # noqa: E402

INPUTS = C.input_names()


# ---- a. the reference ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", mp3gold.STREAMS, ids=lambda p: p.stem)
def test_reference_meets_the_ffmpeg_bar(path):
    """The float64 reference against ffmpeg's decode, same bar as the library's decoders.  Synthetic streams go in through
    the writer's own specs (no parser of the library involved) and, as a check of the two adapters, through parse_units."""
    data = path.read_bytes()
    info = mp3dec.scan(data)
    case = next((c for c in M.CASES if c[0] == path.stem and not c[6].get("sweep")), None)
    via_units = R.decode(C.reference_from_bytes(data))
    if case is not None:
        name, rate, mode, ext, n, seed, opts = case
        built, frames = M.build_case(name, rate, mode, ext, n, seed, return_specs=True, **opts)
        assert built == data
        ref = R.decode(R.from_specs(frames, rate))
        assert np.array_equal(ref, via_units), "the two adapters describe different streams"
    else:
        ref = via_units
    gold = mp3gold.load_gold(path)
    assert ref.shape[0] == gold.shape[0]
    mx, rms, _, _ = mp3gold.compare_with_gold(ref, info.info_frame, gold)
    print(f"{path.stem}: float64 reference vs ffmpeg max {mx:.3f} rms {rms:.3f} steps")
    assert mx <= mp3gold.MAX_STEPS and rms <= mp3gold.RMS_STEPS


def test_reference_imdct_inverts_the_encoders_mdct():
    """mp3_encoder.mdct_granules, then the reference IMDCT + overlap-add: the subband samples come back one granule
    later.  Time-domain alias cancellation is exact for these window pairs, so the only error is float64 rounding of two
    18-term (6-term) cosine sums and the window products: a few 1e-16 of the peak per term, 1e-12 of the peak is generous
    and still nine orders below a wrong window."""
    rng = np.random.default_rng(1)
    bts = [0, 1, 2, 2, 3, 0, 1, 2, 3, 1, 2, 2, 2, 3, 0, 0]  # every legal transition of the state machine
    sub = rng.standard_normal((18 * len(bts), 32))
    xr = E.mdct_granules(sub, bts)
    back = R.imdct_overlap(xr, np.array(bts), np.zeros(len(bts), dtype=bool), np.float64)
    err = float(np.abs(back[18:] - sub[:-18]).max() / np.abs(sub).max())
    print(f"MDCT -> reference IMDCT: max error {err:.3g} of the peak")
    assert err <= 1e-12


def test_reference_synthesis_inverts_the_encoders_analysis():
    """mp3_encoder.polyphase_analysis, then the reference synthesis (matrixing, FIFO, window D, 16 partial sums): the
    input at a delay of 481 samples, to the accuracy of the standard's filterbank itself -- near-perfect reconstruction,
    measured 84.4 dB on noise and on the synthetic piece; asserted with 3 dB to spare."""
    import make_mp3_dense as MD

    for src in ("noise", "piece"):
        x = np.random.default_rng(3).standard_normal(32 * 2000) * 0.2 if src == "noise" else MD.piece(44100, 1.5, 1, 5)[0][:32 * 2000]
        y = R.synthesis(E.polyphase_analysis(x), np.float64)
        err = y[481:] - x[:len(x) - 481]
        snr = 10 * np.log10((x[:len(x) - 481] ** 2).sum() / (err ** 2).sum())
        print(f"analysis -> reference synthesis ({src}): {snr:.2f} dB at delay 481")
        assert snr >= 81.4
        for d in (480, 482):  # and at no other delay
            e2 = y[d:] - x[:len(x) - d]
            assert (e2 ** 2).sum() > 100 * (err ** 2).sum()


# ---- b. what the decoders are held on ----------------------------------------------------------------------------------
def _walk(data):
    """(main_data_begin, crc?, padding) per frame of a bare stream, from the header fields alone."""
    pos, out = 0, []
    while pos + 4 <= len(data):
        h = data[pos:pos + 4]
        ver = (h[1] >> 3) & 3
        lsf = ver != 3
        br = (B.BITRATES_V2 if lsf else B.BITRATES_V1)[h[2] >> 4]
        rate = [44100, 48000, 32000][(h[2] >> 2) & 3] >> (0 if ver == 3 else (1 if ver == 2 else 2))
        crc = (h[1] & 1) == 0
        pad = (h[2] >> 1) & 1
        side = data[pos + 4 + (2 if crc else 0):]
        mdb = side[0] if lsf else (side[0] << 1) | (side[1] >> 7)
        out.append((mdb, crc, pad))
        pos += (72 if lsf else 144) * br * 1000 // rate + pad
    return out


def test_generated_streams_cover_what_the_goldens_could_not():
    cases = C.generated_cases()
    assert len(cases) >= 60 and len({c["name"] for c in cases}) == len(cases)
    rates, modes, gains, seqs = set(), set(), set(), set()
    bts, mixed, sbg, crc, reservoir, escapes, spikes, illegal, padded = set(), 0, 0, 0, 0, 0, 0, 0, 0
    for c in cases:
        data, st = C.load_input("generated", c["name"])
        info = mp3dec.scan(data)
        assert info.audio_frames == C.FRAMES >= 20 and info.skipped_frames == 0 and info.sample_rate == c["rate"]
        rates.add(c["rate"])
        modes.add((c["mode"], c["mode_ext"]))
        gg = [g.global_gain for p in st.granules for g in p.chans]
        assert c["opts"]["gg"][0] <= min(gg) and max(gg) <= c["opts"]["gg"][1]
        gains.add(c["opts"]["gg"])
        seq = [p.chans[0].block_type for p in st.granules]
        for a, b in zip(seq, seq[1:]):  # normal -> start -> short ... -> stop -> normal | start
            assert b in {0: (0, 1), 1: (2,), 2: (2, 3), 3: (0, 1)}[a], (c["name"], a, b)
        seqs.add(c["opts"]["block_types"])
        for p in st.granules:
            for g in p.chans:
                bts.add(g.block_type)
                mixed += g.mixed
                sbg += any(g.subblock_gain)
                escapes += int(np.abs(g.values).max()) >= 15
                spikes += int(np.abs(g.values).max()) > 1728  # beyond the device kernels' table of x^(4/3)
            if p.intensity and st.lsf:
                illegal += any(p.chans[1].illegal)
        w = _walk(data)
        assert len(w) == C.FRAMES
        crc += all(x[1] for x in w)
        reservoir += any(x[0] > 0 for x in w)
        padded += any(x[2] for x in w)
    assert rates == set(C.RATES) and len(modes) == 7 and len(gains) == 3 and len(seqs) == len(C.SEQUENCES)
    assert gains == {(60, 110), (120, 200), (200, 255)}
    assert bts == {0, 1, 2, 3} and mixed > 50 and sbg > 50 and crc >= 10 and reservoir >= 30 and padded >= 5
    assert escapes > 500 and spikes > 200 and illegal > 20


def test_encoded_streams_switch_windows_and_use_mid_side():
    versions = set()
    for enc in C.ENCODED:
        data, st = C.load_input("encoded", enc[0])
        info = mp3dec.scan(data)
        versions.add(info.mpeg_version)
        assert info.frames / info.sample_rate >= 3.0 and info.skipped_frames == 0
        assert {p.chans[0].block_type for p in st.granules} == {0, 1, 2, 3}
        ms = sum(p.ms for p in st.granules)
        assert 0 < ms < len(st.granules) or ms > len(st.granules) // 2
    assert versions == {1, 2, 25}


# ---- c. the bar ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,name", INPUTS, ids=[n for _, n in INPUTS])
def test_host_decoder_is_within_the_float32_floor_of_the_reference(kind, name):
    """2c, and 2e: output length, channel count and StreamInfo agree with the reference's count of decoded granules."""
    data, st = C.load_input(kind, name)
    r64, r32 = C.references(kind, name)
    dec, info = mp3dec.decode(data)
    ngr = 1 if st.lsf else 2
    assert dec.shape == (st.channels, 576 * len(st.granules)) == r64.shape
    assert (info.channels, info.sample_rate, info.frames) == (st.channels, st.rate, 576 * len(st.granules))
    assert info.audio_frames * ngr == len(st.granules)  # decoded frames; dropped ones are in skipped_frames
    assert info.samples_per_frame == 576 * ngr
    m = C.measure(dec, r64, r32)
    print(f"{name}: peak {m['peak']:.3g}; in floors: stream rms {m['stream_rms']:.2f} max {m['stream_max']:.2f}, "
          f"block rms {m['block_rms']:.2f} max {m['block_max']:.2f} (worst block {m['worst_block']}), "
          f"{m['zero_floor_blocks']} blocks with a zero floor")
    if name == "test_stereo":
        assert m["peak"] > 1e6  # global_gain 255: nothing else in the suite judges samples this far above full scale
    assert not m["bad"], (m["bad"], C.name_stage(st, dec, r64))


# ---- d. the bar can see --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("perturb", R.PERTURBATIONS)
def test_the_bar_catches_a_wrong_digit(perturb):
    """The unperturbed decoder output against a reference with one deliberate error, floors from the unperturbed
    reference: beyond the bar on the named stream, at the stream level already.  Keeps a later loosening of the bar honest."""
    sname = C.PERTURB_STREAMS[perturb]
    data, st = C.load_input("golden", sname)
    r64, r32 = C.references("golden", sname)
    dec, _ = mp3dec.decode(data)
    mut = R.decode(st, np.float64, perturb=perturb)
    m = C.measure(dec, mut, mut + (r32.astype(np.float64) - r64))
    print(f"{perturb} on {sname}: stream rms {m['stream_rms']:.1f} max {m['stream_max']:.1f}, block max {m['block_max']:.1f} floors")
    assert m["stream_rms"] > C.MARGIN and m["stream_max"] > C.MARGIN and m["block_rms"] > C.MARGIN and m["block_max"] > C.MARGIN
    if perturb == "intensity_ratio":  # the LSF form of the ratios as well
        data, st = C.load_input("golden", "v2_16k_intensity")
        r64, r32 = C.references("golden", "v2_16k_intensity")
        mut = R.decode(st, np.float64, perturb=perturb)
        m = C.measure(mp3dec.decode(data)[0], mut, mut + (r32.astype(np.float64) - r64))
        print(f"{perturb} on v2_16k_intensity: stream rms {m['stream_rms']:.1f} max {m['stream_max']:.1f} floors")
        assert m["stream_rms"] > C.MARGIN and m["stream_max"] > C.MARGIN


def test_every_perturbation_is_named_and_the_float32_run_rounds_everything():
    assert set(C.PERTURB_STREAMS) == set(R.PERTURBATIONS)
    assert {"window_tap", "exponent", "imdct_window", "alias", "ms_scale", "short_window", "intensity_ratio"} <= set(R.PERTURBATIONS)
    _, st = C.load_input("golden", "v1_44k_ms_mixed")
    stages = {}
    out = R.decode(st, np.float32, stages=stages)
    assert out.dtype == np.float32 and all(v.dtype == np.float32 for v in stages.values())
    assert R.decode(st, np.float64).dtype == np.float64
