"""bench.py's plain line, its `--full` legs and `--dump-outputs DIR`: the dump is what the timed path computed in its last
step, bin for bin the oracle's on the same synthetic input, and stays within its 64 MB by a fixed seeded sample."""
import json
import subprocess
import sys
from pathlib import Path
from types import SimpleNamespace

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
RATE = 44100
LEGS = ("one_shot", "configs1", "mp3_end_to_end", "parity", "cpu_baseline")


def _fake_results(n):
    return [SimpleNamespace(loudness_db=60.0 + i / 100, gain_db=29.0 - 60.0 - i / 100, peak=0.5, sample_rate=RATE, windows=3600,
                            flags=0) for i in range(n)]


def test_dump_outputs_keeps_every_track_when_it_fits(tmp_path):
    import bench

    n = 5
    hists = np.arange(n * 12000, dtype=np.uint32).reshape(n, 12000)
    bench.dump_outputs(str(tmp_path), [10, 11, 12, 13, 14], _fake_results(n), hists, None)
    assert np.array_equal(np.load(tmp_path / "histograms.npy"), hists.astype(np.float32))
    assert np.load(tmp_path / "histograms.npy").dtype == np.float32
    assert np.array_equal(np.load(tmp_path / "histogram_track_index.npy"), [10, 11, 12, 13, 14])
    assert np.array_equal(np.load(tmp_path / "track_loudness_db.npy"), [60.0, 60.01, 60.02, 60.03, 60.04])
    assert not list(tmp_path.glob("album_*.npy"))
    for f in tmp_path.glob("*.npy"):
        assert np.load(f).dtype in (np.float32, np.float64), f.name


def test_dump_outputs_samples_histograms_within_the_budget(tmp_path):
    import bench

    n = 1500  # 1500 x 12 000 x 4 B = 72 MB of histograms: more than the budget
    hists = np.zeros((n, 12000), dtype=np.uint32)
    hists[:, 0] = np.arange(n)
    album = SimpleNamespace(album_loudness_db=61.0, album_gain_db=-32.0, album_peak=0.9, album_gain_steps=-21, windows=n * 3600)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), list(range(n)), _fake_results(n), hists, album)
    total = sum(f.stat().st_size for f in (tmp_path / "a").glob("*.npy"))
    assert total <= bench.DUMP_BUDGET_BYTES
    pick = np.load(tmp_path / "a" / "histogram_track_index.npy")
    assert 0 < len(pick) < n and np.all(np.diff(pick) > 0)
    h = np.load(tmp_path / "a" / "histograms.npy")
    assert np.array_equal(h[:, 0], pick)  # row k is the histogram of track pick[k]
    assert len(np.load(tmp_path / "a" / "track_peak.npy")) == n  # the per-track records are never sampled
    assert np.load(tmp_path / "a" / "album_gain_steps.npy").tolist() == [-21.0]
    for f in (tmp_path / "a").glob("*.npy"):  # the same sample every run
        assert np.array_equal(np.load(f), np.load(tmp_path / "b" / f.name)), f.name


def _bench(*args, timeout=600):
    p = subprocess.run([sys.executable, str(ROOT / "bench.py"), *args], cwd=str(ROOT), capture_output=True, text=True, timeout=timeout)
    assert p.returncode == 0, p.stderr[-3000:]
    return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("{")][-1])


@pytest.mark.gpu
def test_plain_line_and_dump_are_the_last_timed_step(tmp_path, oracle):
    tracks, minutes = 3, 0.1
    line = _bench("--gpus", "1", "--steps", "5", "--warmup", "1", "--tracks-per-rank", str(tracks), "--minutes", str(minutes),
                  "--pre-roll", "0.001", "--dump-outputs", str(tmp_path))
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "roofline"):
        assert key in line, key
    assert line["steps"] == 5 and line["warmup"] == 1
    frames = int(round(minutes * 60 * RATE))
    assert line["value"] == pytest.approx(tracks * frames * 5 / (line["ms_per_step"] * 5e-3), rel=1e-9)
    assert all(line[k] is None for k in LEGS), "a plain run measures the headline alone"
    assert np.array_equal(np.load(tmp_path / "track_index.npy"), np.arange(tracks))
    loud = np.load(tmp_path / "track_loudness_db.npy")
    assert loud.dtype == np.float64 and loud[0] == line["result"]["loudness_db"]
    hists = np.load(tmp_path / "histograms.npy")
    assert hists.shape == (tracks, 12000)
    peaks, flags = np.load(tmp_path / "track_peak.npy"), np.load(tmp_path / "track_flags.npy")
    for t in range(tracks):
        l, r = oracle.synth_f32(0x5EED0000 + t, 0, RATE, frames), oracle.synth_f32(0x5EED0000 + t, 1, RATE, frames)
        want, want_hist = oracle.analyze_pcm(l, r, RATE)
        if not int(flags[t]) & 2:  # a track flagged imprecise may have windows a few bins off on this (asynchronous) path
            assert np.array_equal(hists[t], want_hist.astype(np.float32)), t
        assert peaks[t] == want["peak"] and abs(loud[t] - want["loudness_db"]) <= 0.1


@pytest.mark.gpu
def test_full_line_carries_every_leg():
    line = _bench("--gpus", "1", "--steps", "3", "--warmup", "1", "--tracks-per-rank", "2", "--minutes", "0.1", "--pre-roll", "0.001",
                  "--full", "--cpu-seconds", "0.2", "--parity-tracks", "2", "--mp3-files", "2", "--configs1-steps", "3")
    for k in LEGS:
        assert line[k] is not None, k
    assert line["parity"]["differing_histogram_bins"] == 0 and line["parity"]["peaks_equal"]
    assert line["one_shot"]["same_results_as_pipelined"] and line["mp3_end_to_end"]["routes_agree"]
    assert line["configs1"]["steps"] == 3 and line["cpu_baseline"]["value"] > 0
