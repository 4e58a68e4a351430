"""Frame augmentation on the host (no GPU): the numpy model in tests/frame_aug_ref.py against the native draw
(npp_frame_augment_params_host) and the native per-pixel function (npp_frame_augment_apply_host) -- the code the device kernel
compiles (npp_augment.hpp) --, the ranges and distribution of the draws, the model's transforms on hand-made frames, and the
argument handling of the host classes.  Parity with albumentations' pixels is unpinned: the model is the definition."""
import itertools

import numpy as np
import pytest

from tests import frame_aug_ref as ref

INTENSITIES = ("light", "medium", "strong")


def _native():
    from nclone_amd.engine import frame_augment_params

    return frame_augment_params


def test_model_matches_native_draw():
    native = _native()
    rng = np.random.default_rng(15)
    cases = list(itertools.product(INTENSITIES, (0.3, 0.5, 1.0)))[:8]
    for k, (intensity, p) in enumerate(cases):   # 8 seeds x 125 000 = 10^6 (seed, env, count, target) draws
        seed = int(rng.integers(0, 2**63)) * 2 + k % 2
        envs = rng.integers(0, 1 << 20, size=125_000)
        counts = rng.integers(0, 2**32, size=125_000, dtype=np.uint64)
        counts[:1000] = np.arange(1000)   # small counts, where a training run lives
        envs[:1000] = np.arange(1000) % 130
        targets = rng.integers(0, 2, size=125_000)
        want = ref.draw(seed, envs, counts, targets, p, intensity)
        got = native(seed, envs, counts, targets, p, intensity)
        assert got.dtype == np.int32 and got.shape == (125_000, ref.WORDS)
        assert np.array_equal(got, want), (k, intensity, p)


@pytest.mark.parametrize("intensity", INTENSITIES)
@pytest.mark.parametrize("target", (0, 1))
def test_ranges_and_their_ends(intensity, target):
    """Every parameter inside its range, every range end reached (so the GPU corner cases are reachable values)."""
    native = _native()
    H, W = ref.SHAPES[target]
    L = ref.limits(intensity, H, W)
    s = {"light": 0.7, "medium": 1.0, "strong": 1.3}[intensity]
    assert L["qx"] == int(np.floor(32 * 4 * s * W / 84 + 1e-9)) and L["qy"] == int(np.floor(32 * 4 * s * H / 84 + 1e-9))
    assert (L["hole_lo"], L["hole_hi"]) == (int(6 * s), int(12 * s))
    assert L["A"] == int(np.floor(25.6 * s + 0.5)) and L["B"] == int(np.floor(6528 * s + 0.5))
    n = 400_000
    envs, counts = np.arange(n) % 1000, np.arange(n) // 1000
    q = native(77, envs, counts, np.full(n, target), 0.5, intensity).astype(np.int64)
    assert np.array_equal(q, ref.draw(77, envs, counts, np.full(n, target), 0.5, intensity))

    def ends(col, lo, hi):
        assert col.min() == lo and col.max() == hi, (col.min(), col.max(), lo, hi)

    ends(q[:, 1], -L["qx"], L["qx"])
    ends(q[:, 2], -L["qy"], L["qy"])
    ends(q[:, 3], 1, 2)
    for i in range(2):
        h, w, y0, x0 = (q[:, 4 + 4 * i + j] for j in range(4))
        ends(h, L["hole_lo"], L["hole_hi"])
        ends(w, L["hole_lo"], L["hole_hi"])
        assert y0.min() == 0 and x0.min() == 0
        assert np.all(y0 <= H - h) and np.all(x0 <= W - w)
        assert np.any(y0 == H - h) and np.any(x0 == W - w)
    ends(q[:, 12], 256 - L["A"], 256 + L["A"])
    ends(q[:, 13], -L["B"], L["B"])
    assert q[:, 0].min() >= 0 and q[:, 0].max() <= 15


def _chi2_p(table):
    from scipy.stats import chi2

    table = np.asarray(table, dtype=np.float64)
    exp = table.sum(1, keepdims=True) * table.sum(0, keepdims=True) / table.sum()
    stat = float((((table - exp) ** 2) / exp).sum())
    return float(chi2.sf(stat, df=(table.shape[0] - 1) * (table.shape[1] - 1)))


@pytest.mark.parametrize("p", (0.3, 0.5, 1.0))
def test_gate_frequencies(p):
    from scipy.stats import chi2

    native = _native()
    n = 1_000_000
    envs, counts = np.arange(n) % 1000, np.arange(n) // 1000
    for target in (0, 1):
        mask = native(2026, envs, counts, np.full(n, target), p, "medium")[:, 0]
        for bit, gp in zip((ref.TRANSLATE, ref.FLIP, ref.DROPOUT, ref.BC), ref.GATE_P):
            hits = int(((mask & bit) != 0).sum())
            exp = np.array([gp * p * n, (1 - gp * p) * n])
            obs = np.array([hits, n - hits])
            stat = float((((obs - exp) ** 2) / exp).sum())
            pv = float(chi2.sf(stat, df=1))
            assert pv > 1e-3, (target, bit, hits, exp, pv)


def test_gates_and_targets_are_independent():
    native = _native()
    n = 1_000_000
    envs, counts = np.arange(n) % 1000, np.arange(n) // 1000
    m0 = native(5, envs, counts, np.zeros(n, dtype=np.int32), 0.5, "medium")[:, 0]
    m1 = native(5, envs, counts, np.ones(n, dtype=np.int32), 0.5, "medium")[:, 0]
    bits = (ref.TRANSLATE, ref.FLIP, ref.DROPOUT, ref.BC)
    for m in (m0, m1):   # the four gates of one draw, pairwise
        for a, b in itertools.combinations(bits, 2):
            ga, gb = (m & a) != 0, (m & b) != 0
            table = [[int((ga & gb).sum()), int((ga & ~gb).sum())], [int((~ga & gb).sum()), int((~ga & ~gb).sum())]]
            assert _chi2_p(table) > 1e-3, (a, b, table)
    for a in bits:   # the player_frame and global_view draws of the same (env, count)
        for b in bits:
            ga, gb = (m0 & a) != 0, (m1 & b) != 0
            table = [[int((ga & gb).sum()), int((ga & ~gb).sum())], [int((~ga & gb).sum()), int((~ga & ~gb).sum())]]
            assert _chi2_p(table) > 1e-3, (a, b, table)
    assert np.mean(m0 == m1) < 0.5   # (and the two masks are not the same stream)


def test_p_zero_never_gates():
    native = _native()
    n = 200_000
    for target in (0, 1):
        q = native(9, np.arange(n) % 500, np.arange(n) // 500, np.full(n, target), 0.0, "strong")
        assert not q[:, 0].any()


def _frames(rng, n, target):
    H, W = ref.SHAPES[target]
    f = rng.integers(0, 256, size=(n, H, W), dtype=np.uint8)
    f[0] = 0
    f[1] = 255
    return f


@pytest.mark.parametrize("target", (0, 1))
def test_model_apply_on_hand_made_frames(target):
    rng = np.random.default_rng(3)
    H, W = ref.SHAPES[target]
    f = _frames(rng, 4, target)[3]
    L = ref.limits("strong", H, W)
    assert np.array_equal(ref.apply(f, ref.make_params(mask=ref.TRANSLATE)), f)   # a zero shift is the identity
    assert np.array_equal(ref.apply(f, ref.make_params(mask=0, sx=50, sy=-70, holes=2, hole0=(5, 5, 1, 1), a=300, b=900)), f)   # no gate: nothing
    for kx, ky in ((1, 0), (-2, 3), (3, -1), (-1, -4), (0, 2)):   # +-32 k units: an integer shift with zero fill
        got = ref.apply(f, ref.make_params(mask=ref.TRANSLATE, sx=32 * kx, sy=32 * ky))
        want = np.zeros_like(f)
        ys, xs = slice(max(ky, 0), H + min(ky, 0)), slice(max(kx, 0), W + min(kx, 0))
        yd, xd = slice(max(-ky, 0), H + min(-ky, 0)), slice(max(-kx, 0), W + min(-kx, 0))
        want[ys, xs] = f[yd, xd]
        assert np.array_equal(got, want), (kx, ky)
    flip = ref.make_params(mask=ref.FLIP)
    assert np.array_equal(ref.apply(f, flip), f[:, ::-1])
    assert np.array_equal(ref.apply(ref.apply(f, flip), flip), f)   # flipping twice is the identity
    assert np.array_equal(ref.apply(f, ref.make_params(mask=ref.BC, a=256, b=0)), f)   # a = 256, b = 0 is the identity
    white, black = np.full((H, W), 255, dtype=np.uint8), np.zeros((H, W), dtype=np.uint8)
    assert np.all(ref.apply(white, ref.make_params(mask=ref.BC, a=256 + L["A"], b=L["B"])) == 255)
    assert np.all(ref.apply(black, ref.make_params(mask=ref.BC, a=256 - L["A"], b=-L["B"])) == 0)
    # a half-pixel shift averages neighbours; a hole is black after the flip, and brightness / contrast comes last
    half = ref.apply(f, ref.make_params(mask=ref.TRANSLATE, sx=16)).astype(np.int64)
    left = np.concatenate([np.zeros((H, 1), dtype=np.int64), f[:, :-1].astype(np.int64)], axis=1)
    assert np.array_equal(half, (16 * 32 * left + 16 * 32 * f.astype(np.int64) + 512) >> 10)
    got = ref.apply(f, ref.make_params(mask=ref.FLIP | ref.DROPOUT | ref.BC, holes=1, hole0=(7, 9, 2, 3), a=256, b=5 * 256))
    want = np.clip(f[:, ::-1].astype(np.int64) + 5, 0, 255)
    want[2:9, 3:12] = 5
    assert np.array_equal(got, want)


@pytest.mark.parametrize("target", (0, 1))
def test_model_apply_matches_native_pixel_function(target):
    """The per-pixel function the kernel compiles, run on the host, against the model: drawn parameters at every intensity with
    p = 1 (every gate on) and p = 0.5, and the corners of the ranges."""
    from nclone_amd.engine import frame_augment_apply, frame_augment_params

    rng = np.random.default_rng(4)
    H, W = ref.SHAPES[target]
    n = 96
    f = _frames(rng, n, target)
    for intensity, p in itertools.product(INTENSITIES, (0.5, 1.0)):
        q = frame_augment_params(31, np.arange(n), np.arange(n) % 7, np.full(n, target), p, intensity)
        assert np.array_equal(frame_augment_apply(f, q), ref.apply(f, q)), (intensity, p)
    L = ref.limits("strong", H, W)
    rows = [ref.make_params(mask=15, sx=sx * L["qx"], sy=sy * L["qy"], holes=2, hole0=(15, 15, 0, 0), hole1=(15, 15, H - 15, W - 15),
                            a=a, b=b)
            for sx, sy in itertools.product((-1, 1), repeat=2) for a, b in ((256 + L["A"], L["B"]), (256 - L["A"], -L["B"]))]
    q = np.stack(rows)
    assert np.array_equal(frame_augment_apply(f[:len(q)], q), ref.apply(f[:len(q)], q))
    with pytest.raises(ValueError):
        frame_augment_apply(f[:1], ref.make_params(mask=4, holes=1, hole0=(10, 10, H - 5, 0))[None])


def test_argument_errors_need_no_device():
    from nclone_amd.async_env import NppAsyncVecEnvironment
    from nclone_amd.vec_env import NppEnvironment, NppVecEnvironment

    lvl = [np.zeros(1)]
    for make in (lambda **kw: NppVecEnvironment(lvl, 64, **kw), lambda **kw: NppEnvironment(map_data=lvl[0], **kw)):
        with pytest.raises(ValueError) as ei:
            make(enable_visual_observations=True, enable_augmentation=True, augmentation_intensity="heavy")
        assert str(ei.value) == "intensity must be one of ['light', 'medium', 'strong']"
        for bad in (-0.1, 1.5, float("nan")):
            with pytest.raises(ValueError) as ei:
                make(enable_visual_observations=True, enable_augmentation=True, augmentation_p=bad)
            assert str(ei.value) == "p must be between 0.0 and 1.0"
        with pytest.raises(ValueError, match="observation_mode='minimal' conflicts with enable_augmentation"):
            make(observation_mode="minimal", enable_augmentation=True)
    with pytest.raises(NotImplementedError, match="frame augmentation"):
        NppAsyncVecEnvironment(lvl, 64, enable_augmentation=True)


def test_exports_and_header():
    import os

    from nclone_amd import _native as nat

    names = {"npp_set_frame_augmentation", "npp_frame_augment", "npp_frame_augment_view", "npp_frame_augment_params_host"}
    assert names <= set(nat.EXPORTS)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "npp_amd.h")).read()
    assert "PARITY WITH ALBUMENTATIONS' PIXELS IS UNPINNED" in hdr and "frame_augmentation.py:56-103" in hdr
