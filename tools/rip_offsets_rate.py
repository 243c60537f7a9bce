#!/usr/bin/env python3
"""The offsets kernel (rg_rip_offsets.hip: a disc's AccurateRip signatures at every drive offset) against the definition on the
host (MI355X): a synthetic disc of 12 tracks of five minutes of 44.1 kHz 16-bit stereo, filled on the device, at radius 2939
(rg_rip_offsets_rate).

    tools/rip_offsets_rate.py [--tracks 12] [--seconds 300] [--radius 2939] [--host-offsets 64] [--threads 16] [--reps 10]
                              [--warm-ms 400] [--plain-reps 3] [--out profiles/rip_offsets_rate.json]

After a warm-up (a fresh process runs slower for a while after a large allocation: the kernel is launched for `warm-ms`
milliseconds first), `reps` rounds of the table's zeroing and the kernel (HIP events around them); median and spread (min ..
max) are reported, and products per second.  The host twin runs the definition for every track at `host-offsets` offsets
spread evenly over the window on `threads` threads; its time is scaled to the whole window by the number of products (every
product costs the same).  Every host value must equal the kernel's.  The same disc is then run `plain-reps` rounds through the
kernel's plain form -- a lane per offset, every product reading its word from LDS, instead of 23 consecutive offsets per lane
in registers -- with its values checked at three offsets; 0 skips it.

The kernel's second yardstick is its own instruction count: VALU_PER_PRODUCT vector instructions per product in the inner
loop (one v_mad_u64_u32 and two v_add_u32, plus one ds_read_b32 per 23 products, as counted in the gfx950 ISA), against the
chip's issue rate for full-rate vector instructions."""
import argparse
import ctypes as C
import json
import statistics
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

VALU_PER_PRODUCT = 3.0
# MI355X: 256 CUs of 4 SIMDs at about 2.4 GHz; a SIMD issues a full-rate wave64 vector instruction every 2 cycles
ISSUE_PEAK_WAVE_INSTR_PER_S = 256 * 4 * 2.4e9 / 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tracks", type=int, default=12)
    ap.add_argument("--seconds", type=float, default=300.0)
    ap.add_argument("--radius", type=int, default=2939)
    ap.add_argument("--host-offsets", type=int, default=64)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warm-ms", type=float, default=400.0)
    ap.add_argument("--plain-reps", type=int, default=3)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "rip_offsets_rate.json"))
    a = ap.parse_args()
    import torch  # noqa: F401  (torch first: one HIP runtime per process)

    import mp3rgain_amd as rg
    from mp3rgain_amd import _capi

    L = _capi.load()
    frames = int(44100 * a.seconds)
    dev = (C.c_double * a.reps)()
    host_ms, bad = C.c_double(), C.c_size_t()
    host_products, disc_products = C.c_uint64(), C.c_uint64()
    with rg.Analyzer(0) as an:
        an._check(L.rg_rip_offsets_rate(an.handle, a.tracks, frames, a.radius, 23, a.host_offsets, a.threads, a.reps, a.warm_ms, dev, C.byref(host_ms),
                                        C.byref(host_products), C.byref(disc_products), C.byref(bad)))
        if bad.value:
            raise SystemExit(f"{bad.value} host values differ from the kernel's")
        plain = None
        if a.plain_reps:
            pdev = (C.c_double * a.plain_reps)()
            pms, pbad, pprod = C.c_double(), C.c_size_t(), C.c_uint64()
            an._check(L.rg_rip_offsets_rate(an.handle, a.tracks, frames, a.radius, 1, min(3, 2 * a.radius + 1), a.threads, a.plain_reps, 0.0, pdev,
                                            C.byref(pms), C.byref(pprod), None, C.byref(pbad)))
            if pbad.value:
                raise SystemExit(f"{pbad.value} host values differ from the plain kernel's")
            plain = {"lane_offsets": 1, "device_ms": statistics.median(pdev), "device_ms_all": list(pdev)}
    ms = statistics.median(dev)
    products = disc_products.value
    per_s = products / (ms / 1e3)
    wave_instr_per_s = per_s * VALU_PER_PRODUCT / 64
    result = {"tool": "rip_offsets_rate", "tracks": a.tracks, "seconds_per_track": a.seconds, "frames_per_track": frames, "radius": a.radius,
              "offsets": 2 * a.radius + 1, "products": products, "reps": a.reps, "warm_ms": a.warm_ms,
              "device_ms": ms, "device_ms_min": min(dev), "device_ms_max": max(dev), "device_ms_all": list(dev),
              "device_products_per_s": per_s, "valu_per_product": VALU_PER_PRODUCT,
              "issue_peak_wave_instr_per_s": ISSUE_PEAK_WAVE_INSTR_PER_S, "fraction_of_issue_peak": wave_instr_per_s / ISSUE_PEAK_WAVE_INSTR_PER_S,
              "mismatches": bad.value, "lane_offsets": 23, "plain_kernel": plain}
    line = (f"{a.tracks} tracks x {a.seconds:.0f} s at radius {a.radius}: {products:.3e} products, device {ms:.1f} ms "
            f"({min(dev):.1f} .. {max(dev):.1f}) = {per_s:.3e} products/s = {100 * result['fraction_of_issue_peak']:.1f} % of the full-rate "
            f"issue peak at {VALU_PER_PRODUCT:.0f} vector instructions per product")
    if a.host_offsets:
        scaled = host_ms.value * products / host_products.value
        result.update(host_threads=a.threads, host_offsets=a.host_offsets, host_products=host_products.value, host_ms_measured=host_ms.value,
                      host_ms_scaled_to_the_disc=scaled, host_products_per_s=host_products.value / (host_ms.value / 1e3), device_over_host=scaled / ms)
        line += (f"; host x{a.threads} {host_ms.value:.0f} ms for {a.host_offsets} offsets = {scaled / 1e3:.1f} s for the disc "
                 f"({result['host_products_per_s']:.3e} products/s): the device is {scaled / ms:.0f} times as fast; 0 mismatches")
    print(line)
    if plain:
        print(f"one offset per lane (every product reads LDS): {plain['device_ms']:.1f} ms = {plain['device_ms'] / ms:.2f} times the time")
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)
    Path(a.out).write_text(json.dumps(result, indent=1) + "\n")


if __name__ == "__main__":
    main()
