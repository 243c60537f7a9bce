"""The parity signals of the EBU R 128 tests, in one place: tests/test_gpu_r128.py runs them through the library and
tools/r128_refcheck.py measures the float64 checker's own error on exactly these (tests/golden/r128_measured.json).
Not part of the product."""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

RATES = [8000, 11025, 22050, 44100, 48000, 96000, 176400, 192000]
KINDS = ["music", "noise", "sine30", "dc_noise", "loud_quiet"]


def _f64(kind, rate, frames, nch, seed):
    """`nch` float64 channels in [-1, 1]."""
    rng = np.random.default_rng(seed)
    t = np.arange(frames) / rate
    out = []
    for c in range(nch):
        if kind == "music":
            from oracle import pyoracle

            x = pyoracle.synth_f32(seed, c, rate, frames).astype(np.float64)
        elif kind == "noise":
            x = 0.25 * rng.standard_normal(frames)
        elif kind == "sine30":
            x = np.sin(2.0 * np.pi * 30.0 * t + 0.4 * c)
        elif kind == "dc_noise":
            x = 0.9 + 1e-3 * rng.standard_normal(frames)
        elif kind == "loud_quiet":
            # three seconds of full-scale noise, then noise at about -65 LUFS: the energy in front of a lane that starts in
            # the quiet part is 10^6.5 times its blocks'
            x = rng.uniform(-1.0, 1.0, frames)
            cut = min(frames, 3 * rate)
            x[cut:] *= 10.0 ** (-66.4 / 20.0)
        else:
            raise ValueError(kind)
        out.append(np.clip(x, -1.0, 1.0))
    return out


def make(kind, rate, frames, nch, fmt, seed):
    """-> list of `nch` arrays of dtype float32 / int16 / int32."""
    chans = _f64(kind, rate, frames, nch, seed)
    if fmt == "f32":
        return [c.astype(np.float32) for c in chans]
    if fmt == "s16":
        return [np.clip(np.round(c * 32767.0), -32768, 32767).astype(np.int16) for c in chans]
    return [np.clip(np.round(c * 2147483647.0), -2147483648, 2147483647).astype(np.int32) for c in chans]


def hop(rate):
    return (rate + 5) // 10


def parity_cases():
    """[(id, kind, rate, frames, channels, format, seed)]"""
    cases = []
    for i, rate in enumerate(RATES):  # every rate: music, stereo, the three formats in turn
        cases.append((f"music-{rate}", "music", rate, int(2.5 * rate) + 17, 2, ["f32", "s16", "s32"][i % 3], 100 + i))
    for rate in (44100, 48000):  # every kind
        for k, kind in enumerate(KINDS):
            secs = 5.0 if kind == "loud_quiet" else 3.0
            cases.append((f"{kind}-{rate}", kind, rate, int(secs * rate) + 3, 2, "f32", 200 + k))
    for kind in ("noise", "dc_noise"):  # integer formats, mono
        cases.append((f"{kind}-s16-44100", kind, 44100, 3 * 44100, 2, "s16", 300))
        cases.append((f"{kind}-s32-48000-mono", kind, 48000, 3 * 48000 + 1, 1, "s32", 301))
    cases.append(("music-mono-f32-48000", "music", 48000, 3 * 48000, 1, "f32", 302))
    cases.append(("loud_quiet-192000", "loud_quiet", 192000, 5 * 192000, 2, "f32", 303))
    cases.append(("loud_quiet-8000-s16", "loud_quiet", 8000, 5 * 8000, 2, "s16", 304))
    cases.append(("sine30-176400-mono", "sine30", 176400, 2 * 176400, 1, "f32", 305))
    for rate, nch, fmt in ((48000, 2, "f32"), (44100, 1, "s16")):  # tracks around the shortest that has a block
        h = hop(rate)
        for name, frames in (("empty", 0), ("hop-1", h - 1), ("3hops", 3 * h), ("4hops", 4 * h), ("4hops+1", 4 * h + 1)):
            cases.append((f"noise-{name}-{rate}-{fmt}", "noise", rate, frames, nch, fmt, 400))
    return cases


def load_measured():
    import json

    return json.loads((Path(__file__).resolve().parent / "golden" / "r128_measured.json").read_text())
