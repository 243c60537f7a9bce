#!/usr/bin/env python3
"""The spectrum kernels against torch.stft on the same device and against their own host arithmetic (MI355X): BASELINE
configs[2]-sized data, 1000 tracks of three minutes of 44.1 kHz 16-bit stereo filled on the device (rg_spectrum_rate), and the
same frames as 32-bit float.

    tools/spectrum_rate.py [--tracks 1000] [--seconds 180] [--host-tracks 4] [--threads 16] [--reps 7] [--warm-ms 400]
                           [--torch-planes 0] [--json profiles/spectrum_rate.json]

After a warm-up, every one of `reps` rounds runs three things one after the other:
  1. the tile + fold kernels over all planes, 16-bit and float (HIP events around the launches alone);
  2. the same transform written with torch: torch.stft (periodic Hann, n_fft 4096, hop 2048, center=False) over `torch-planes`
     planes of float PCM already resident on the device, abs() ** 2 and the band sums in float64, between two events.  The PCM
     need not be converted, which favours torch; the batch (`torch-planes` = 0) is the largest that fits beside its
     spectrogram: half of the free device memory less the kernels' arenas, at ten times a plane's PCM per plane (the frame
     matrix, the complex spectrogram, its magnitudes and their squares), halved until the pipeline runs; the time is
     scaled per sample;
  3. route 2 (the kernels' arithmetic on the host) on `threads` threads over a host copy of the first `host-tracks` tracks, scaled
     to the count.  Every host record must equal the kernels' byte for byte.
Medians and the spread (min .. max) are reported, as milliseconds for the whole workload, samples per second and GB/s of PCM.
The bar: the kernels' median time per sample below the torch pipeline's, and the slowest kernel round still faster than the
fastest torch round."""
import argparse
import ctypes as C
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tracks", type=int, default=1000)
    ap.add_argument("--seconds", type=float, default=180.0)
    ap.add_argument("--host-tracks", type=int, default=4)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warm-ms", type=float, default=400.0)
    ap.add_argument("--torch-planes", type=int, default=0, help="planes per torch batch; 0 = the largest that fits")
    ap.add_argument("--no-torch", action="store_true", help="the kernels alone (for a counter pass)")
    ap.add_argument("--json", default=str(ROOT / "profiles" / "spectrum_rate.json"))
    a = ap.parse_args()
    import torch

    import mp3rgain_amd as rg
    from mp3rgain_amd import _capi

    L = _capi.load()
    n, frames = a.tracks, int(44100 * a.seconds)
    samples = n * 2 * frames
    host_n = min(n, a.host_tracks)
    fr, hop, bands, tile = rg.spectrum_kernel_shape()

    dev = torch.device("cuda", 0)
    tp = a.torch_planes
    if tp <= 0 and not a.no_torch:
        free, _ = torch.cuda.mem_get_info(dev)
        arenas = n * 2 * frames * 4 + (1 << 30)  # the float leg's arena and the kernels' records stay allocatable beside torch's
        tp = int((free // 2 - arenas) // (10 * frames * 4))
    tp = max(1, min(tp, 2 * n))
    x = None
    win = torch.hann_window(fr, periodic=True, device=dev, dtype=torch.float32)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def torch_input():
        return torch.rand((tp, frames), device=dev, dtype=torch.float32) - 0.5

    def torch_pass():
        s = torch.stft(x, n_fft=fr, hop_length=hop, window=win, center=False, return_complex=True)  # [planes, 2049, K]
        p = s.abs() ** 2
        return p[:, 1:fr // 2 + 1, :].reshape(tp, bands, 8, -1).sum(dim=(2, 3), dtype=torch.float64)

    def torch_ms():
        e0.record()
        e = torch_pass()
        e1.record()
        torch.cuda.synchronize()
        del e
        return e0.elapsed_time(e1)

    kernel = {"s16": [], "f32": []}
    host_ms, torch_all, mismatches = [], [], 0
    with rg.Analyzer(0) as an:
        while not a.no_torch:  # warm up; a batch that does not fit is halved
            try:
                x = torch_input()
                for _ in range(3):
                    torch_ms()
                break
            except torch.cuda.OutOfMemoryError:
                if tp == 1:
                    raise
                x = None
                torch.cuda.empty_cache()
                tp = max(1, tp // 2)
        torch_samples = tp * frames
        print(f"torch batch: {tp} planes", flush=True)
        for r in range(a.reps):
            for fmt, name in ((_capi.FMT_S16_PLANAR, "s16"), (_capi.FMT_F32_PLANAR, "f32")):
                ms, hm, bad = (C.c_double * 1)(), (C.c_double * 1)(), C.c_size_t()
                hn = host_n if name == "s16" else 0
                an._check(L.rg_spectrum_rate(an.handle, n, frames, fmt, hn, a.threads, 1, a.warm_ms, ms, hm, C.byref(bad)))
                kernel[name].append(ms[0])
                if hn:
                    host_ms.append(hm[0] * n / hn)
                    mismatches += bad.value
            if not a.no_torch:
                torch_all.append(torch_ms() * samples / torch_samples)
            print(f"round {r}: kernels s16 {kernel['s16'][-1]:.2f} ms, f32 {kernel['f32'][-1]:.2f} ms"
                  + (f", torch.stft scaled {torch_all[-1]:.2f} ms" if torch_all else "")
                  + (f", host x{a.threads} scaled {host_ms[-1]:.0f} ms" if host_ms else ""), flush=True)

    def timing(ms_all, bytes_per_sample):
        ms = statistics.median(ms_all)
        return {"ms": ms, "ms_min": min(ms_all), "ms_max": max(ms_all), "ms_all": list(ms_all), "samples_per_s": samples / (ms / 1e3),
                "ns_per_sample": ms * 1e6 / samples, "pcm_gb_per_s": samples * bytes_per_sample / 1e9 / (ms / 1e3)}

    result = {"tool": "spectrum_rate", "rate": 44100, "channels": 2, "tracks": n, "seconds_per_track": a.seconds, "samples": samples,
              "frame": fr, "hop": hop, "frames_per_tile": tile, "reps": a.reps, "warm_ms": a.warm_ms,
              "kernels_s16": timing(kernel["s16"], 2), "kernels_f32": timing(kernel["f32"], 4), "host_mismatches": mismatches}
    if host_ms:
        result["host_route2"] = dict(timing(host_ms, 2), threads=a.threads, tracks_transformed=host_n, scaled=True)
    if torch_all:
        result["torch_stft_f32"] = dict(timing(torch_all, 4), planes=tp, scaled=True, torch=torch.__version__)
        k, t = result["kernels_s16"], result["torch_stft_f32"]
        result["kernels_over_torch_time"] = k["ms"] / t["ms"]
        result["bar_median_below_torch"] = k["ms"] < t["ms"]
        result["bar_slowest_kernel_round_below_fastest_torch_round"] = k["ms_max"] < t["ms_min"]
        result["f32_kernels_over_torch_time"] = result["kernels_f32"]["ms"] / t["ms"]
    for key in ("kernels_s16", "kernels_f32", "torch_stft_f32", "host_route2"):
        if key in result:
            t = result[key]
            print(f"{key}: {t['ms']:.2f} ms ({t['ms_min']:.2f} .. {t['ms_max']:.2f}), {t['samples_per_s']:.3e} samples/s, {t['pcm_gb_per_s']:.1f} GB/s of PCM")
    print(f"host mismatches {mismatches}" + (f"; bar: median {result['bar_median_below_torch']}, outside the spread "
                                             f"{result['bar_slowest_kernel_round_below_fastest_torch_round']}" if torch_all else ""))
    if a.json != "-":
        Path(a.json).parent.mkdir(parents=True, exist_ok=True)
        Path(a.json).write_text(json.dumps(result, indent=1) + "\n")
    if mismatches:
        raise SystemExit(f"{mismatches} host records differ from the kernels'")


if __name__ == "__main__":
    main()
