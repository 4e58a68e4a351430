"""Frame stacking on the device (npp_stack.hip + the render kernel's ring output) against the numpy model of the reference's
FrameStackWrapper (tests/frame_stack_ref.py, pinned to the wrapper by test_frame_stack_host.py): a stacked env and an unstacked
twin on the same levels and actions; the model applied to the twin's outputs, with the twin's flags as the reset mask, must give
the stacked env's player_frame, game_state and terminal_game_state_stack byte for byte at every step."""
import numpy as np
import pytest
import torch

from tests.frame_stack_ref import StackModel

pytestmark = pytest.mark.gpu

STEPS = 300


def _levels():
    from nclone_amd.levels import door_levels, mine_levels

    return mine_levels()[0][:6] + door_levels()[0][:6]   # mines and doors: deaths, wins and auto-resets


def _np(x):
    return x.cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def _close(*envs):
    for e in envs:
        e.close()
    torch.cuda.synchronize()


def _check_step(t, obs, info, tw_obs, tw_info, mv, ms, reset, stacked_keys):
    for k in tw_obs:
        if k in stacked_keys:
            continue
        assert np.array_equal(_np(obs[k]), _np(tw_obs[k]), equal_nan=True), (t, k)
    if mv is not None:
        want = mv.push(_np(tw_obs["player_frame"]), reset)
        got = obs["player_frame"]
        assert tuple(got.shape) == want.shape and _np(got).dtype == np.uint8
        assert np.array_equal(_np(got), want), (t, "player_frame")
    if ms is not None:
        term = _np(tw_info["terminal_observation"]) if tw_info is not None else None
        r = ms.push(_np(tw_obs["game_state"]), reset, terminal=term)
        want, want_term = r if term is not None else (r, None)
        got = obs["game_state"]
        assert tuple(got.shape) == want.shape
        assert np.array_equal(_np(got), want), (t, "game_state")
        if want_term is not None:
            assert np.array_equal(_np(info["terminal_game_state_stack"]), want_term), (t, "terminal_game_state_stack")
            assert np.array_equal(_np(info["terminal_observation"]), term), t


def _run(n, vk, sk, pad, output="torch", autoreset=True, obs_overlap=0, steps=STEPS, seed=0):
    from nclone_amd.vec_env import NppVecEnvironment

    levels = _levels()
    kw = dict(enable_visual_observations=True, truncation_limit=60, autoreset=autoreset, obs_overlap=obs_overlap)
    env = NppVecEnvironment(levels, n, output=output, enable_visual_frame_stacking=vk > 0, visual_stack_size=max(vk, 1),
                            enable_state_stacking=sk > 0, state_stack_size=max(sk, 1), frame_stack_padding_type=pad, **kw)
    twin = NppVecEnvironment(levels, n, output="numpy", **kw)
    try:
        sp = env.observation_space
        assert tuple(sp["player_frame"].shape) == ((vk, 84, 84, 1) if vk else (84, 84, 1))
        assert tuple(sp["game_state"].shape) == ((sk, 41) if sk else (41,))
        mv = StackModel(vk, pad) if vk else None
        ms = StackModel(sk, pad) if sk else None
        stacked = {"player_frame"} if vk else set()
        stacked |= {"game_state"} if sk else set()
        obs, _ = env.reset(seed=1)
        tw, _ = twin.reset(seed=1)
        _check_step(-1, obs, {}, tw, None, mv, ms, np.ones(n, dtype=bool), stacked)
        acts = np.random.default_rng(seed).integers(0, 6, size=(steps, n)).astype(np.uint8)
        n_reset = 0
        for t in range(steps):
            obs, _r, _te, _tr, info = env.step(acts[t])
            tw, _r2, te2, tr2, info2 = twin.step(acts[t])
            reset = (te2 | tr2) if autoreset else np.zeros(n, dtype=bool)
            n_reset += int(reset.sum())
            if output == "numpy":
                for k in stacked:
                    assert isinstance(obs[k], np.ndarray) and obs[k].flags.c_contiguous
            _check_step(t, obs, info, tw, info2, mv, ms, reset, stacked)
            if sk:
                assert tuple(info["terminal_game_state_stack"].shape) == (n, sk, 41)
        if autoreset:
            assert n_reset > n   # won / dead / truncated envs were re-padded many times over
        wins = info2["player_won"]   # (the last step's flags: a level set with wins and deaths is what the levels are for)
        assert wins.dtype == bool
    finally:
        _close(env, twin)


def test_stack_k4_torch_8192():
    _run(8192, 4, 4, "zero", output="torch")


def test_stack_k4_torch_1000_repeat_overlap():
    _run(1000, 4, 4, "repeat", output="torch", obs_overlap=45)


def test_stack_k12_visual_k1_state_numpy_1000():
    _run(1000, 12, 1, "zero", output="numpy")


def test_stack_k1_visual_k12_state_repeat_numpy_overlap():
    _run(1000, 1, 12, "repeat", output="numpy", obs_overlap=50)


def test_stack_no_autoreset_keeps_stacking():
    _run(1000, 4, 12, "repeat", output="torch", autoreset=False)


def test_stack_state_only_and_visual_only():
    _run(1000, 0, 4, "zero", output="numpy", steps=120)
    _run(1000, 4, 0, "repeat", output="torch", steps=120)


def test_stack_visual_ignored_without_visual_observations():
    from nclone_amd.vec_env import NppVecEnvironment

    env = NppVecEnvironment(_levels(), 256, enable_visual_frame_stacking=True, enable_state_stacking=True, state_stack_size=3)
    try:
        obs, _ = env.reset()
        assert "player_frame" not in obs and tuple(obs["game_state"].shape) == (256, 3, 41)
        assert "player_frame" not in env.observation_space.spaces
    finally:
        _close(env)


def test_single_env_stacking():
    from nclone_amd.vec_env import NppEnvironment

    lvl = _levels()[0]
    kw = dict(enable_visual_observations=True, truncation_limit=60)
    env = NppEnvironment(map_data=lvl, enable_visual_frame_stacking=True, visual_stack_size=4, enable_state_stacking=True,
                         state_stack_size=4, frame_stack_padding_type="repeat", **kw)
    twin = NppEnvironment(map_data=lvl, **kw)
    try:
        assert tuple(env.observation_space["player_frame"].shape) == (4, 84, 84, 1)
        mv, ms = StackModel(4, "repeat"), StackModel(4, "repeat")

        def check(obs, tw, reset, t):
            assert obs["player_frame"].shape == (4, 84, 84, 1) and obs["game_state"].shape == (4, 41)
            assert np.array_equal(obs["player_frame"], mv.push(tw["player_frame"][None], [reset])[0]), t
            assert np.array_equal(obs["game_state"], ms.push(tw["game_state"][None], [reset])[0]), t
            for k in tw:
                if k not in ("player_frame", "game_state"):
                    assert np.array_equal(np.asarray(obs[k]), np.asarray(tw[k])), (t, k)

        obs, _ = env.reset()
        tw, _ = twin.reset()
        reset_now = True
        rng = np.random.default_rng(3)
        resets = 0
        for t in range(STEPS):
            check(obs, tw, reset_now, t)
            a = int(rng.integers(0, 6))
            obs, _r, te, tr, _i = env.step(a)
            tw, _r2, te2, tr2, _i2 = twin.step(a)
            assert (te, tr) == (te2, tr2)
            reset_now = False
            if te or tr:   # autoreset is off for the single env: the terminal observation is stacked, then the user resets
                check(obs, tw, False, t)
                obs, _ = env.reset()
                tw, _ = twin.reset()
                reset_now = True
                resets += 1
        assert resets > 0
    finally:
        _close(env, twin)


def test_resets_repad_every_env():
    """reset(), reset(options={"checkpoint": "snapshot"}) and reset(options={"checkpoint": seq}) re-pad every env from the
    observation after the reset / restore / replay (frame_stack_wrapper.py:183-264)."""
    from nclone_amd.vec_env import NppVecEnvironment

    n = 1000
    levels = _levels()
    kw = dict(enable_visual_observations=True, truncation_limit=60)
    env = NppVecEnvironment(levels, n, enable_visual_frame_stacking=True, visual_stack_size=4, enable_state_stacking=True,
                            state_stack_size=5, frame_stack_padding_type="repeat", **kw)
    twin = NppVecEnvironment(levels, n, output="numpy", **kw)
    try:
        mv, ms = StackModel(4, "repeat"), StackModel(5, "repeat")
        rng = np.random.default_rng(11)
        all_reset = np.ones(n, dtype=bool)

        def check(obs, tw, reset, tag):
            assert np.array_equal(_np(obs["player_frame"]), mv.push(tw["player_frame"], reset)), tag
            assert np.array_equal(_np(obs["game_state"]), ms.push(tw["game_state"], reset)), tag

        def steps(k, tag):
            for t in range(k):
                a = rng.integers(0, 6, size=n).astype(np.uint8)
                obs, _r, _te, _tr, _i = env.step(a)
                tw, _r2, te2, tr2, _i2 = twin.step(a)
                check(obs, tw, te2 | tr2, (tag, t))

        obs, _ = env.reset()
        tw, _ = twin.reset()
        check(obs, tw, all_reset, "reset")
        steps(7, "a")
        env.snapshot()
        twin.snapshot()
        steps(9, "b")
        obs, _ = env.reset()
        tw, _ = twin.reset()
        check(obs, tw, all_reset, "reset 2")
        steps(5, "c")
        obs, info = env.reset(options={"checkpoint": "snapshot"})
        tw, _ = twin.reset(options={"checkpoint": "snapshot"})
        assert info.get("restored_snapshot")
        check(obs, tw, all_reset, "snapshot")
        steps(6, "d")
        seq = rng.integers(0, 6, size=(n, 9)).astype(np.uint8)
        obs, info = env.reset(options={"checkpoint": seq})
        tw, _ = twin.reset(options={"checkpoint": seq})
        assert info["checkpoint_replay"]
        check(obs, tw, all_reset, "replay")
        steps(6, "e")
    finally:
        _close(env, twin)
