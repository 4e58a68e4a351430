"""The level pool's draw on the host (no GPU): the numpy model in tests/level_pool_ref.py against the native hash
(npp_level_pool_draw_host, the code the device kernel compiles), the distribution of the draws, the weight checks, and the
Python helpers around the pool."""
import numpy as np
import pytest

from tests.level_pool_ref import draw


def _native():
    from nclone_amd.engine import level_pool_draw

    return level_pool_draw


def test_model_matches_native_hash():
    native = _native()
    rng = np.random.default_rng(12)
    w = rng.random(37)
    w[[0, 5, 6, 36]] = 0.0   # zero weights at both ends and inside
    w[17] = 1e-9             # a tiny one
    for k in range(8):       # 8 seeds x 125 000 = 10^6 (seed, env, count) triples
        seed = int(rng.integers(0, 2**63)) * 2 + k % 2
        envs = rng.integers(0, 1 << 20, size=125_000)
        counts = rng.integers(0, 2**32, size=125_000, dtype=np.uint64)
        counts[:1000] = np.arange(1000)   # small counts, where a training run lives
        want = draw(w, seed, envs, counts)
        got = native(w, seed, envs, counts)
        assert np.array_equal(got, want), k


def test_zero_weight_never_drawn_and_frequencies():
    from scipy.stats import chi2

    native = _native()
    w = np.array([3.0, 0.0, 1.0, 0.5, 0.0, 2.5, 1.0, 0.0])
    envs = np.repeat(np.arange(1000), 1000)
    counts = np.tile(np.arange(1000), 1000)
    got = native(w, 2026, envs, counts)
    assert np.array_equal(got, draw(w, 2026, envs, counts))
    hist = np.bincount(got, minlength=len(w))
    assert hist[w == 0].sum() == 0
    exp = w[w > 0] / w.sum() * len(got)
    stat = float((((hist[w > 0] - exp) ** 2) / exp).sum())
    p = float(chi2.sf(stat, df=int((w > 0).sum()) - 1))
    assert p > 1e-3, (hist, stat, p)


def test_single_level_and_uniform():
    native = _native()
    e = np.arange(5000)
    c = np.zeros(5000, dtype=np.uint32)
    assert np.all(native([0.0, 0.0, 4.0, 0.0], 1, e, c) == 2)
    assert np.array_equal(native(np.ones(512), 7, e, c), draw(np.ones(512), 7, e, c))


@pytest.mark.parametrize("w, msg", [
    ([1.0, float("nan")], "weight 1 is nan"),
    ([1.0, -0.5, 2.0], "weight 1 is -0.5"),
    ([0.0, 0.0], "every weight is zero"),
    ([1.0, float("inf")], "weight 1 is inf"),
    ([], "0 weights"),
])
def test_bad_weights_raise(w, msg):
    native = _native()
    with pytest.raises(ValueError, match="level pool: .*" + msg.split(" is ")[0]) as ei:
        native(w, 0, [0], [0])
    assert msg.split(" is ")[-1] in str(ei.value)


def test_expand_category_weights():
    from nclone_amd.levels import curriculum0_levels
    from nclone_amd.vec_env import expand_category_weights, level_category

    _, tags = curriculum0_levels()
    cats = [level_category(t) for t in tags]
    assert set(cats) == {"replay", "maze:tiny", "hills:simple"}
    w = expand_category_weights({"replay": 2.0, "maze:tiny": 1.0}, cats)
    cats = np.array(cats)
    assert np.all(w[cats == "hills:simple"] == 0)
    assert np.isclose(w[cats == "replay"].sum(), 2.0) and np.isclose(w[cats == "maze:tiny"].sum(), 1.0)
    assert len(set(w[cats == "replay"])) == 1
    with pytest.raises(ValueError):
        expand_category_weights({"nope": 1.0}, cats)


def test_async_env_refuses_a_pool():
    from nclone_amd.async_env import NppAsyncVecEnvironment

    with pytest.raises(NotImplementedError):
        NppAsyncVecEnvironment([np.zeros(1)], 64, level_weights=[1.0])
