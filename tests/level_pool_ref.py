"""Numpy model of the level pool's draw (include/npp_amd.h, npp_set_level_pool; nclone_amd/csrc/npp_pool.hpp).

Env e with draw count c (0 for its first draw, +1 per draw):
    mix(z) = splitmix64 round; u = mix(mix((e << 32) | c) ^ seed)
    t      = (u >> 11) * 2^-53 * cdf[-1], cdf = cumsum(weights) (f64, index order)
    level  = searchsorted(cdf, t, side="right"), or the last level of non-zero weight when that is len(weights)
The reference draws with Python's `random` (env_map_loader.py:210-234); this stream is the project's own.
"""
import numpy as np

_U = np.uint64


def _mix(z):
    with np.errstate(over="ignore"):
        z = z + _U(0x9E3779B97F4A7C15)
        z = (z ^ (z >> _U(30))) * _U(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> _U(27))) * _U(0x94D049BB133111EB)
        return z ^ (z >> _U(31))


def draw(weights, seed, envs, counts):
    """int64 [len(envs)]: the level env envs[i] draws at draw count counts[i]."""
    w = np.asarray(weights, dtype=np.float64)
    cdf = np.cumsum(w)
    key = (np.asarray(envs).astype(np.uint64) << _U(32)) | np.asarray(counts).astype(np.uint64)
    u = _mix(_mix(key) ^ _U(int(seed) & (2**64 - 1)))
    t = (u >> _U(11)).astype(np.float64) * (2.0 ** -53) * cdf[-1]
    lv = np.searchsorted(cdf, t, side="right")
    last = int(np.nonzero(w > 0)[0][-1])
    return np.where(lv < len(w), lv, last)


class PoolModel:
    """Per-env draw counts of one pool: draw(mask) returns the levels the masked envs draw now (and counts them)."""

    def __init__(self, n, weights, seed):
        self.n, self.w, self.seed = int(n), np.asarray(weights, dtype=np.float64), int(seed)
        self.count = np.zeros(self.n, dtype=np.uint64)

    def draw(self, mask):
        idx = np.nonzero(np.asarray(mask, dtype=bool))[0]
        lv = draw(self.w, self.seed, idx, self.count[idx])
        self.count[idx] += _U(1)
        return idx, lv
