"""Frame augmentation on the device (npp_augment.hip) against the numpy model of its definition (tests/frame_aug_ref.py, pinned to
the native draw and per-pixel function by test_frame_aug_host.py; parity with albumentations' pixels is unpinned):
an augmented env and a twin with the feature off on the same levels, actions and level seed; the model applied to the twin's
clean frames with the model's draw for (seed, env, observation count, key) must give the augmented env's player_frame and
global_view bit for bit, and every other output must equal the twin's.

With the feature off the observations are the parent's: the existing suite pins that and was run unchanged; here only the
C entry's refusal is checked."""
import ctypes as C
import functools
import itertools

import numpy as np
import pytest
import torch

from tests import frame_aug_ref as ref

pytestmark = pytest.mark.gpu

SEED = 20261018
STEPS = 6
TRUNC = 12   # frames: 3 actions of 4 ticks, so every env is auto-reset (and its stack re-padded) at steps 3 and 6


def _levels():
    from nclone_amd.levels import door_levels, mine_levels

    return mine_levels()[0][:6] + door_levels()[0][:6]


def _np(x):
    return x.cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def _copy(x):
    if isinstance(x, dict):
        return {k: _copy(v) for k, v in x.items()}
    return _np(x).copy() if isinstance(x, (torch.Tensor, np.ndarray)) else x


def _close(*envs):
    for e in envs:
        e.close()
    torch.cuda.synchronize()


def _make(n, k, pad, output, aug, pool=False, **extra):
    from nclone_amd.vec_env import NppVecEnvironment

    kw = dict(enable_visual_observations=True, truncation_limit=TRUNC, output=output, enable_visual_frame_stacking=k > 0,
              visual_stack_size=max(k, 1), frame_stack_padding_type=pad)
    if pool:
        kw.update(level_weights=np.ones(len(_levels())), level_seed=3)
    if aug:
        kw.update(enable_augmentation=True, augmentation_seed=SEED)
    kw.update(extra)
    return NppVecEnvironment(_levels(), n, **kw)


def _actions(n, steps=STEPS):
    return np.random.default_rng(7).integers(0, 6, size=(steps, n)).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def _twin_run(n, k, pad, pool=False):
    """The clean run every augmented run of the same shape is compared with: [(obs, reward, terminated, truncated, info)] of
    reset() and STEPS steps, as host copies (computed once per shape)."""
    twin = _make(n, k, pad, "numpy", False, pool)
    try:
        obs, info = twin.reset()
        out = [(_copy(obs), None, None, None, _copy(info))]
        for a in _actions(n):
            out.append(tuple(_copy(x) for x in twin.step(a)))
        return out
    finally:
        _close(twin)


def _expect(clean_obs, n, count, p=0.5, intensity="medium", seed=SEED):
    """(player_frame, global_view) the model makes of the clean observation at augmentation call `count`."""
    envs, counts = np.arange(n), np.full(n, count)
    pf = clean_obs["player_frame"][..., 0]
    q0 = ref.draw(seed, envs, counts, np.zeros(n, dtype=int), p, intensity)
    q1 = ref.draw(seed, envs, counts, np.ones(n, dtype=int), p, intensity)
    want_pf = ref.apply_stack(pf, q0) if pf.ndim == 4 else ref.apply(pf, q0)
    return want_pf[..., None], ref.apply(clean_obs["global_view"][..., 0], q1)[..., None]


def _same(a, b, tag):
    if isinstance(a, dict):
        assert set(a) == set(b), tag
        for k in a:
            _same(a[k], b[k], (tag, k))
    elif isinstance(a, (np.ndarray, torch.Tensor)):
        assert np.array_equal(_np(a), _np(b), equal_nan=True), tag
    else:
        assert a == b, tag


def _check_obs(obs, clean, n, count, tag, **draw_kw):
    want_pf, want_gv = _expect(clean, n, count, **draw_kw)
    got_pf, got_gv = _np(obs["player_frame"]), _np(obs["global_view"])
    assert got_pf.shape == clean["player_frame"].shape and got_pf.dtype == np.uint8
    assert got_gv.shape == clean["global_view"].shape and got_gv.dtype == np.uint8
    bad = np.nonzero((got_pf != want_pf).reshape(n, -1).any(axis=1))[0]
    assert bad.size == 0, (tag, "player_frame", bad[:8])
    bad = np.nonzero((got_gv != want_gv).reshape(n, -1).any(axis=1))[0]
    assert bad.size == 0, (tag, "global_view", bad[:8])
    for k in clean:
        if k not in ("player_frame", "global_view"):
            assert np.array_equal(_np(obs[k]), clean[k], equal_nan=True), (tag, k)


def _run_drawn(n, k, pad, output, pool=False):
    twin = _twin_run(n, k, pad, pool)
    env = _make(n, k, pad, output, True, pool)
    try:
        assert tuple(env.observation_space["player_frame"].shape) == ((k, 84, 84, 1) if k else (84, 84, 1))
        assert tuple(env.observation_space["global_view"].shape) == (176, 100, 1)
        obs, info = env.reset()
        _check_obs(obs, twin[0][0], n, 0, "reset")
        _same(info, twin[0][4], "reset info")
        changed = resets = 0
        for t, a in enumerate(_actions(n)):
            obs, rew, term, trunc, info = env.step(a)
            c_obs, c_rew, c_term, c_trunc, c_info = twin[t + 1]
            if output == "numpy":
                assert isinstance(obs["player_frame"], np.ndarray) and isinstance(obs["global_view"], np.ndarray)
            _check_obs(obs, c_obs, n, t + 1, t)
            _same(rew, c_rew, (t, "reward"))
            _same(term, c_term, (t, "terminated"))
            _same(trunc, c_trunc, (t, "truncated"))
            _same(info, c_info, (t, "info"))
            changed += int((_np(obs["player_frame"]) != c_obs["player_frame"]).reshape(n, -1).any(axis=1).sum())
            resets += int((c_term | c_trunc).sum())
        assert resets >= n   # every env was auto-reset (truncation after 3 actions at the latest): padded stacks under one draw
        if n >= 65:
            assert changed > n   # (and the augmentation did something: at p = 0.5 about 71 % of the frames change)
    finally:
        _close(env)


@pytest.mark.parametrize("output", ("torch", "numpy"))
@pytest.mark.parametrize("pad", ("zero", "repeat"))
@pytest.mark.parametrize("k", (0, 1, 4, 12))
def test_drawn_path_130_envs(k, pad, output):
    _run_drawn(130, k, pad, output)   # two full 64-env blocks and a tail of 2


def test_drawn_path_single_env():
    _run_drawn(1, 4, "zero", "torch")


def test_drawn_path_65_envs_level_pool():
    _run_drawn(65, 4, "repeat", "numpy", pool=True)


def test_single_environment_adapter():
    from nclone_amd.vec_env import NppEnvironment

    lvl = _levels()[0]
    kw = dict(enable_visual_observations=True, truncation_limit=TRUNC, enable_visual_frame_stacking=True, visual_stack_size=4)
    env = NppEnvironment(map_data=lvl, enable_augmentation=True, augmentation_p=1.0, augmentation_intensity="strong",
                         augmentation_seed=SEED, **kw)
    twin = NppEnvironment(map_data=lvl, **kw)
    try:
        obs, _ = env.reset()
        tw, _ = twin.reset()
        for count in range(3):
            clean = {"player_frame": tw["player_frame"][None], "global_view": tw["global_view"][None]}
            want_pf, want_gv = _expect(clean, 1, count, p=1.0, intensity="strong")
            assert obs["player_frame"].shape == (4, 84, 84, 1) and np.array_equal(obs["player_frame"], want_pf[0])
            assert obs["global_view"].shape == (176, 100, 1) and np.array_equal(obs["global_view"], want_gv[0])
            obs = env.step(2)[0]
            tw = twin.step(2)[0]
    finally:
        _close(env, twin)


def _batch(n=65):
    """A bare batch whose two visual outputs hold synthetic frames: the sources of an augmentation call are plain buffers, so
    the forced-parameter cases run on every grey level (random bytes, an all-0 and an all-255 frame) instead of on a render."""
    from nclone_amd.engine import NppBatch

    b = NppBatch(n, outputs=("player_frame", "global_view"))
    b.load_levels(_levels())
    b.assign_levels((np.arange(n) // 64) % len(_levels()))
    b.reset()
    b.observe()
    b.render_player_frame()
    b.render_global_view()
    g = torch.Generator().manual_seed(5)
    clean = []
    with b._ctx():
        for k in ("player_frame", "global_view"):
            t = b.out.t[k]
            f = torch.randint(0, 256, tuple(t.shape), dtype=torch.uint8, generator=g)
            f[n - 1] = 0
            f[n - 2] = 255
            t.copy_(f.to(b.device))
            clean.append(f.numpy()[..., 0])
    b.sync()
    return b, clean


def _forced_cases(target):
    H, W = ref.SHAPES[target]
    L = ref.limits("strong", H, W)
    assert L["qx"] % 32 and L["qy"] % 32   # the fractional weights are live
    hi = L["hole_hi"]
    cases = [ref.make_params(mask=ref.TRANSLATE, sx=sx * L["qx"], sy=sy * L["qy"]) for sx, sy in itertools.product((-1, 1), repeat=2)]
    cases.append(ref.make_params(mask=ref.FLIP | ref.DROPOUT, holes=2, hole0=(hi, hi, 0, 0), hole1=(hi, hi, H - hi, W - hi)))   # opposite corners
    cases.append(ref.make_params(mask=ref.FLIP | ref.DROPOUT, holes=2, hole0=(hi, hi, 20, 30), hole1=(hi, hi, 20 + hi // 2, 30 + hi // 2)))   # overlapping
    cases.append(ref.make_params(mask=ref.DROPOUT, holes=1, hole0=(hi, hi, 3, 5), hole1=(hi, hi, 40, 40)))   # the second hole is not drawn
    cases.append(ref.make_params(mask=ref.BC, a=256 + L["A"], b=L["B"]))
    cases.append(ref.make_params(mask=ref.BC, a=256 - L["A"], b=-L["B"]))
    cases.append(ref.make_params(mask=ref.BC, a=256 + L["A"], b=-L["B"]))
    cases.append(ref.make_params(mask=ref.BC, a=256 - L["A"], b=L["B"]))
    cases.append(ref.make_params(mask=15, sx=L["qx"], sy=-L["qy"], holes=2, hole0=(hi, L["hole_lo"], H - hi, 0),
                                 hole1=(L["hole_lo"], hi, 0, W - hi), a=256 + L["A"], b=-L["B"]))   # every gate at once
    cases.append(ref.make_params(mask=0, sx=L["qx"], sy=L["qy"], holes=2, hole0=(hi, hi, 0, 0), a=300, b=999))   # empty mask: the copy path
    return cases


def test_forced_parameters():
    from nclone_amd import _native as nat

    n = 65
    b, clean = _batch(n)
    try:
        b.set_frame_augmentation(True, 1.0, "strong", seed=1)
        params = np.zeros((n, 2, ref.WORDS), dtype=np.int32)
        params[:, :, 12] = 256   # every env without a case: an empty mask
        n_cases = 0
        for target in (0, 1):
            cases = _forced_cases(target)
            n_cases = len(cases)
            for rep in range(n // n_cases):   # one env per case (repeated over the batch: the all-0 / all-255 frames get cases too)
                params[rep * n_cases:(rep + 1) * n_cases, target] = np.stack(cases)
            params[n - n_cases:, target] = np.stack(cases)
        b.frame_augment(params)
        got = [_np(v)[..., 0] for v in b.frame_augment_views()]
        assert got[0].shape == (n, 1, 84, 84) and got[1].shape == (n, 176, 100)
        for target, g in enumerate((got[0][:, 0], got[1])):
            want = ref.apply(clean[target], params[:, target])
            bad = np.nonzero((g != want).reshape(n, -1).any(axis=1))[0]
            assert bad.size == 0, (target, bad, params[bad[:4], target])
            empty = params[:, target, 0] == 0
            assert empty.any() and np.array_equal(g[empty], clean[target][empty])   # the copy path: the clean frame
            L = ref.limits("strong", *ref.SHAPES[target])
            v = clean[target].astype(np.int64)
            assert (((256 + L["A"]) * v + L["B"]) >> 8).max() > 255 and (((256 - L["A"]) * v - L["B"]) >> 8).min() < 0   # both clamps fire
        # the sources were only read
        assert np.array_equal(_np(b.out.t["player_frame"])[..., 0], clean[0]) and np.array_equal(_np(b.out.t["global_view"])[..., 0], clean[1])
        # parameters outside the image are refused, and the call count still advanced once per accepted call
        bad = params.copy()
        bad[3, 1, 4:8] = (10, 10, 170, 0)
        with pytest.raises(ValueError, match="env 3, target 1"):
            b.frame_augment(bad)
        b.frame_augment()   # drawn, call count 1
        got = [_np(v)[..., 0] for v in b.frame_augment_views()]
        envs = np.arange(n)
        for target, g in enumerate((got[0][:, 0], got[1])):
            q = ref.draw(1, envs, np.ones(n, dtype=int), np.full(n, target), 1.0, "strong")
            assert np.array_equal(g, ref.apply(clean[target], q)), target
        # switching it off frees the buffers; the view is refused
        b.set_frame_augmentation(False)
        base, nbytes = C.c_void_p(), C.c_int64()
        assert b.lib.npp_frame_augment_view(b.h, 0, C.byref(base), C.byref(nbytes)) == nat.NPP_ERR_STATE
    finally:
        b.close()
        torch.cuda.synchronize()


def test_feature_off_refuses_the_view_and_bad_arguments():
    from nclone_amd import _native as nat
    from nclone_amd.engine import NppBatch

    b = NppBatch(8, outputs=("player_frame", "global_view"))
    try:
        b.load_levels(_levels())
        base, nbytes = C.c_void_p(), C.c_int64()
        for which in (0, 1):
            assert b.lib.npp_frame_augment_view(b.h, which, C.byref(base), C.byref(nbytes)) == nat.NPP_ERR_STATE
        assert b.lib.npp_frame_augment(b.h, None) == nat.NPP_ERR_STATE
        # a handle without visual outputs (nothing rendered or stacked yet), a bad p, a bad scale
        assert b.lib.npp_set_frame_augmentation(b.h, 1, 0.5, 1.0, 0) == nat.NPP_ERR_INVALID
        assert b"no visual outputs" in b.lib.npp_last_error(b.h)
        b.reset()
        b.observe()
        b.render_player_frame()
        b.render_global_view()
        assert b.lib.npp_set_frame_augmentation(b.h, 1, 1.5, 1.0, 0) == nat.NPP_ERR_INVALID
        assert b.lib.npp_set_frame_augmentation(b.h, 1, 0.5, 0.9, 0) == nat.NPP_ERR_INVALID
        assert b.lib.npp_frame_augment_view(b.h, 0, C.byref(base), C.byref(nbytes)) == nat.NPP_ERR_STATE
        assert b.lib.npp_set_frame_augmentation(b.h, 1, 0.5, 1.0, 0) == nat.NPP_OK
        assert b.lib.npp_frame_augment_view(b.h, 1, C.byref(base), C.byref(nbytes)) == nat.NPP_OK and nbytes.value == 8 * 176 * 100
    finally:
        b.close()
        torch.cuda.synchronize()


def test_ring_stays_clean():
    n = 130
    env = _make(n, 4, "repeat", "torch", True)
    twin = _make(n, 4, "repeat", "torch", False)
    try:
        env.reset()
        twin.reset()
        for a in _actions(n, 8):
            env.step(a)
            twin.step(a)
        pf, _ = env.batch.frame_stack_views()
        tw, _ = twin.batch.frame_stack_views()
        assert np.array_equal(_np(pf), _np(tw))
        assert np.array_equal(_np(env.batch.out.t["global_view"]), _np(twin.batch.out.t["global_view"]))
    finally:
        _close(env, twin)


def _rollout(env, n, steps=3, seed=None):
    out = [_copy({k: v for k, v in env.reset(seed=seed)[0].items() if k in ("player_frame", "global_view")})]
    for a in _actions(n, steps):
        out.append(_copy({k: v for k, v in env.step(a)[0].items() if k in ("player_frame", "global_view")}))
    return out


def test_determinism_and_reseeding():
    n = 130
    a = _make(n, 4, "zero", "torch", True)
    b = _make(n, 4, "zero", "numpy", True)
    c = _make(n, 4, "zero", "torch", True, augmentation_seed=SEED + 1)
    try:
        ra, rb, rc = _rollout(a, n), _rollout(b, n), _rollout(c, n)
        for x, y in zip(ra, rb):   # the same augmentation_seed twice: identical bytes
            _same(x, y, "same seed")
        differs = np.zeros(n, dtype=bool)
        for x, y in zip(ra, rc):   # another seed differs
            differs |= (x["player_frame"] != y["player_frame"]).reshape(n, -1).any(axis=1)
        assert differs.any()
        r1, r2 = _rollout(a, n, seed=99), _rollout(a, n, seed=99)   # reset(seed=s) restarts the stream
        for x, y in zip(r1, r2):
            _same(x, y, "reseeded")
        obs, _ = a.reset(seed=99)   # ... from s: the ring and the output block hold the clean frames of this observation
        clean = {"player_frame": _np(a.batch.frame_stack_views()[0]), "global_view": _np(a.batch.out.t["global_view"])}
        _check_obs(obs, clean, n, 0, "reseeded reset", seed=99)
        assert any((x["global_view"] != y["global_view"]).any() for x, y in zip(ra, r1))
    finally:
        _close(a, b, c)


def test_obs_overlap_gives_the_same_bytes():
    n = 130
    a = _make(n, 4, "repeat", "torch", True)
    b = _make(n, 4, "repeat", "torch", True, obs_overlap=2)
    try:
        for x, y in zip(_rollout(a, n, 6), _rollout(b, n, 6)):
            _same(x, y, "obs_overlap")
    finally:
        _close(a, b)


def test_snapshot_reset_is_augmented_with_the_next_count():
    n = 130
    env = _make(n, 4, "zero", "torch", True)
    twin = _make(n, 4, "zero", "numpy", False)
    try:
        env.reset()
        twin.reset()
        acts = _actions(n, 5)
        for a in acts[:2]:
            env.step(a)
            twin.step(a)
        env.snapshot()
        twin.snapshot()
        for a in acts[2:]:
            env.step(a)
            twin.step(a)
        obs, info = env.reset(options={"checkpoint": "snapshot"})
        tw, _ = twin.reset(options={"checkpoint": "snapshot"})
        assert info.get("restored_snapshot")
        _check_obs(obs, _copy(tw), n, 6, "snapshot")   # calls 0 (reset) and 1 .. 5 came before: the restore leaves the count alone
        obs = env.step(acts[0])[0]
        tw = twin.step(acts[0])[0]
        _check_obs(obs, _copy(tw), n, 7, "after snapshot")
    finally:
        _close(env, twin)
