"""The tracks and the album partitions that tests/test_gpu_r128_albums.py and tests/test_r128_albums_cpu.py share: the 34
parity signals of tests/r128cases.py and the 28 range signals of tests/r128range_cases.py, cut into albums by the rule of
tests/test_gpu_albums.py (a seeded permutation, albums of 1 to 6, one empty album at a random place and one at the end).
Not part of the product."""
import sys
from pathlib import Path

import numpy as np

sys.path.insert(0, str(Path(__file__).resolve().parent))
import r128cases  # noqa: E402
import r128range_cases  # noqa: E402

SEEDS = (1, 2)
_CACHE = {}


def signals():
    """[(id, channels, rate)]: 62 tracks, eight rates, three formats, mono and stereo, from no hop at all to 260 s."""
    if "signals" not in _CACHE:
        out = [(c[0], r128cases.make(*c[1:]), c[2]) for c in r128cases.parity_cases()]
        out += [(c[0], r128range_cases.make(*c[1:]), c[2]) for c in r128range_cases.range_cases()]
        _CACHE["signals"] = out
    return _CACHE["signals"]


def partition(items, seed, max_album=6, empty=True):
    rng = np.random.default_rng(seed)
    order = list(rng.permutation(len(items)))
    albums = []
    while order:
        k = int(rng.integers(1, max_album + 1))
        albums.append([items[i] for i in order[:k]])
        order = order[k:]
    if empty:
        albums.insert(int(rng.integers(0, len(albums) + 1)), [])
        albums.append([])
    return albums


def albums(seed):
    """The 62 tracks as albums of track indices."""
    return partition(list(range(len(signals()))), seed)
