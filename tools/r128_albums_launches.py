#!/usr/bin/env python3
"""One rg_r128_analyze_albums_pcm_dynamics call (true peak on) over N small albums of two tracks and one album of 17971
short-term blocks, which the library selects by wide passes.  Run it under `rocprofv3 --kernel-trace --stats` with two values
of N: the number of kernel launches is the same.

    rocprofv3 --kernel-trace --stats --output-format csv -d out -o t -- python tools/r128_albums_launches.py 4"""
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))


def main():
    import torch  # noqa: F401

    import mp3rgain_amd as rg

    n_albums = int(sys.argv[1]) if len(sys.argv) > 1 else 4
    rng = np.random.default_rng(1)
    rate = 48000
    albums = [[rg.PcmTrack([(0.1 * rng.standard_normal(5 * rate)).astype(np.float32)] * 2, rate) for _ in range(2)]
              for _ in range(n_albums)]
    long = (3000.0 * rng.standard_normal(1800 * 8000)).astype(np.int16)
    albums.insert(n_albums // 2, [rg.PcmTrack([long], 8000)])
    with rg.Analyzer(0) as an:
        res = an.analyze_albums_r128(albums, true_peak=True, dynamics=True)
    print(f"{len(res)} albums, the long one {res[n_albums // 2].dynamics.st_blocks} short-term blocks, LRA {res[n_albums // 2].dynamics.loudness_range_lu:.3f} LU")


if __name__ == "__main__":
    main()
