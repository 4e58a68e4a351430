"""The level pool on the device (npp_pool.hip + the masked reset / observe launches) against a twin without a pool.

The pool env draws its next level whenever an episode ends.  The twin is the existing stepper: it steps the same actions, and
after every step it assigns the levels tests/level_pool_ref.py predicts to the envs whose draw changed level (npp_assign_levels),
observes them (npp_observe into scratch rows, copied over the changed rows only) and runs the observation kernels.  Every
observation key, the flags, info["level_id"], the state dump and the entity checksums must match byte for byte at every step."""
import ctypes as C

import numpy as np
import pytest
import torch

from nclone_amd import _native as nat

from tests.frame_stack_ref import StackModel
from tests.level_pool_ref import PoolModel

pytestmark = pytest.mark.gpu

STEPS = 300
SEED = 4242


def _levels(zoo=True):
    from nclone_amd.levels import curriculum0_levels, door_levels, mine_levels, zoo_levels

    out = mine_levels()[0][:5] + door_levels()[0][:5] + curriculum0_levels()[0][:5]
    return out + (zoo_levels()[0][:5] if zoo else [])


def _weights(n_levels):
    w = np.linspace(1.0, 3.0, n_levels)
    w[1] = 0.0   # a level no draw may pick (it is still played by the envs of the initial assignment)
    return w


def _np(x):
    return x.cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def _close(*envs):
    for e in envs:
        e.close()
    torch.cuda.synchronize()


class Twin:
    """NppVecEnvironment without a pool, driven by hand through the draws the model predicts."""

    def __init__(self, levels, n, w, **kw):
        from nclone_amd.vec_env import NppVecEnvironment

        self.env = NppVecEnvironment(levels, n, output="numpy", **kw)
        self.b = self.env.batch
        self.n = n
        self.w = w
        self.cur = self.b.env_levels()

    def _assign(self, idx, lv):
        ch = idx[lv != self.cur[idx]]
        if len(ch):
            self.b.assign_levels(lv[lv != self.cur[idx]], env_ids=ch)
            self.cur[ch] = lv[lv != self.cur[idx]]
        return ch

    def reset(self, seed):
        self.model = PoolModel(self.n, self.w, seed)
        self._assign(*self.model.draw(np.ones(self.n, dtype=bool)))
        return self.env.reset(seed=seed)

    def step(self, acts):
        env, b = self.env, self.b
        with b._ctx():
            env._actions.copy_(torch.as_tensor(acts))
        b.step(env._actions, env.frame_skip, want_terminal=True)
        flags = b.flags.cpu().numpy()
        ended = (flags & 11) != 0
        ch = self._assign(*self.model.draw(ended))
        if len(ch):   # npp_observe's rows for the envs that changed level, the others as the step left them
            t = b.out.t
            keys = [k for k in ("game_state", "action_mask", "entity_pos", "spatial_context", "positions") if k in t]
            with b._ctx():
                scratch = {k: torch.empty_like(t[k]) for k in keys}

                def p(k):
                    return scratch[k].data_ptr() if k in scratch else None

                o = nat.StepOut(p("game_state"), p("action_mask"), p("entity_pos"), None, None, None, None, p("spatial_context"),
                                p("positions"), None)
                nat.check(b.h, b.lib.npp_observe(b.h, C.byref(o)))
                sel = torch.from_numpy(ch).to(b.device)
                for k in keys:
                    t[k][sel] = scratch[k][sel]
        env._produce()
        obs, rew, te, tr, info = env.step_wait()
        return obs, rew, te, tr, info, ch


def _compare(t, obs, info, tw_obs, tw_info, pool_b, twin_b, skip=()):
    for k in tw_obs:
        if k in skip:
            continue
        assert np.array_equal(_np(obs[k]), _np(tw_obs[k]), equal_nan=True), (t, k)
    if tw_info is not None:
        for k in ("player_won", "player_dead", "switch_activated", "frames_executed", "terminal_observation"):
            assert np.array_equal(_np(info[k]), _np(tw_info[k]), equal_nan=True), (t, k)
    assert np.array_equal(_np(info["level_id"]) if info else pool_b.env_levels(), twin_b.env_levels()), t
    f1, i1 = pool_b.dump_state()
    f2, i2 = twin_b.dump_state()
    assert np.array_equal(f1, f2, equal_nan=True) and np.array_equal(i1, i2), (t, "dump_state")
    assert np.array_equal(pool_b.entity_checksum(), twin_b.entity_checksum(), equal_nan=True), (t, "entity_checksum")


def _run(n, output="torch", fast_reset=True, truncation_limit=60, zoo=True, steps=STEPS, **obs_kw):
    from nclone_amd.vec_env import NppVecEnvironment

    levels = _levels(zoo)
    w = _weights(len(levels))
    kw = dict(truncation_limit=truncation_limit, fast_reset=fast_reset, **obs_kw)
    env = NppVecEnvironment(levels, n, output=output, level_weights=w, level_seed=99, **kw)
    twin = Twin(levels, n, w, **kw)
    try:
        obs, _ = env.reset(seed=SEED)
        tw, _ = twin.reset(SEED)
        _compare(-1, obs, {}, tw, None, env.batch, twin.b)
        acts = np.random.default_rng(n).integers(0, 6, size=(steps, n)).astype(np.uint8)
        changed = same = 0
        for t in range(steps):
            obs, rew, te, tr, info = env.step(acts[t])
            tw, rew2, te2, tr2, info2, ch = twin.step(acts[t])
            if output == "numpy":
                assert isinstance(info["level_id"], np.ndarray)
            else:
                assert isinstance(info["level_id"], torch.Tensor) and info["level_id"].is_cuda
            assert np.array_equal(_np(rew), rew2) and np.array_equal(_np(te), te2) and np.array_equal(_np(tr), tr2), t
            _compare(t, obs, info, tw, info2, env.batch, twin.b)
            ended = int((te2 | tr2).sum())
            changed += len(ch)
            same += ended - len(ch)
        assert changed > 0 and same > 0, (changed, same)   # both kinds of draw happened
        assert not np.any(env.batch.env_levels() == 1)      # weight 0: reset() drew every env off it, and no draw picks it
    finally:
        _close(env, twin.env)


def test_pool_twin_1000_torch_fast():
    _run(1000)


def test_pool_twin_8192_numpy_full_reset():
    _run(8192, output="numpy", fast_reset=False)


def test_pool_twin_8192_torch_fast():
    _run(8192, steps=120)


def test_pool_twin_reachability_switch_states():
    _run(1000, zoo=False, enable_reachability=True, enable_switch_states=True)


def test_pool_twin_spatial_context_numpy():
    _run(1000, output="numpy", enable_spatial_context=True)


def test_pool_twin_visual():
    _run(1000, enable_visual_observations=True, steps=150)


def test_pool_twin_dynamic_truncation():
    _run(1000, truncation_limit="dynamic", fast_reset=False)


def test_pool_frame_stack_k4():
    """A stacked pool env against tests/frame_stack_ref.py applied to an unstacked pool env with the same seed."""
    from nclone_amd.vec_env import NppVecEnvironment

    levels = _levels()
    w = _weights(len(levels))
    kw = dict(enable_visual_observations=True, truncation_limit=60, level_weights=w, level_seed=5)
    n = 1000
    env = NppVecEnvironment(levels, n, enable_visual_frame_stacking=True, visual_stack_size=4, enable_state_stacking=True,
                            state_stack_size=4, **kw)
    plain = NppVecEnvironment(levels, n, output="numpy", **kw)
    try:
        mv, ms = StackModel(4), StackModel(4)
        obs, _ = env.reset(seed=8)
        tw, _ = plain.reset(seed=8)
        assert np.array_equal(_np(obs["player_frame"]), mv.push(tw["player_frame"], np.ones(n, bool)))
        assert np.array_equal(_np(obs["game_state"]), ms.push(tw["game_state"], np.ones(n, bool)))
        acts = np.random.default_rng(3).integers(0, 6, size=(150, n)).astype(np.uint8)
        for t in range(150):
            obs, _r, _te, _tr, info = env.step(acts[t])
            tw, _r2, te2, tr2, info2 = plain.step(acts[t])
            reset = te2 | tr2
            assert np.array_equal(_np(info["level_id"]), info2["level_id"]), t
            assert np.array_equal(_np(obs["player_frame"]), mv.push(tw["player_frame"], reset)), (t, "player_frame")
            gs, term = ms.push(tw["game_state"], reset, terminal=info2["terminal_observation"])
            assert np.array_equal(_np(obs["game_state"]), gs), (t, "game_state")
            assert np.array_equal(_np(info["terminal_game_state_stack"]), term), (t, "terminal stack")
    finally:
        _close(env, plain)


def _batch(levels, n=256, **kw):
    from nclone_amd.engine import NppBatch

    b = NppBatch(n, **kw)
    b.load_levels(levels)
    b.assign_levels((np.arange(n) // 64) % len(levels))
    b.set_truncation_limit(60)
    return b


def _acts(n, seed=0):
    return torch.from_numpy(np.random.default_rng(seed).integers(0, 6, size=n).astype(np.uint8)).cuda()


def test_weight_change_takes_effect_at_next_draw():
    levels = _levels()
    n = 512
    b = _batch(levels, n, fast_reset=True)
    try:
        w = _weights(len(levels))
        b.set_level_pool(w, seed=11)
        model = PoolModel(n, w, 11)
        for t in range(40):
            b.step(_acts(n, t))
            model.draw((b.flags.cpu().numpy() & 11) != 0)
        w2 = np.zeros(len(levels))
        w2[7] = 1.0
        b.set_level_pool(w2, seed=11)   # same seed: a curriculum update, the counts go on
        model.w = w2
        before = b.env_levels()
        b.step(_acts(n, 99))
        ended = (b.flags.cpu().numpy() & 11) != 0
        assert ended.any()
        idx, lv = model.draw(ended)
        after = b.env_levels()
        assert np.all(after[ended] == 7) and np.array_equal(after[~ended], before[~ended])
        with pytest.raises(ValueError, match="weights for"):
            b.set_level_pool(np.ones(len(levels) + 1), seed=1)
        with pytest.raises(ValueError, match="every weight is zero"):
            b.set_level_pool(np.zeros(len(levels)), seed=1)
    finally:
        b.close()


def test_snapshot_draw_restore_brings_back_level_and_state():
    levels = _levels()
    n = 512
    b = _batch(levels, n, fast_reset=True)
    try:
        b.set_level_pool(_weights(len(levels)), seed=3)
        for t in range(30):
            b.step(_acts(n, t))
        b.snapshot()
        lv0, (f0, i0), cs0 = b.env_levels(), b.dump_state(), b.entity_checksum()
        for t in range(60):
            b.step(_acts(n, 100 + t))
        assert np.any(b.env_levels() != lv0)
        b.restore()
        assert np.array_equal(b.env_levels(), lv0)
        f1, i1 = b.dump_state()
        assert np.array_equal(f1, f0, equal_nan=True) and np.array_equal(i1, i0)
        assert np.array_equal(b.entity_checksum(), cs0, equal_nan=True)
        # the draw counts came back too: the same actions draw the same levels again
        seq = []
        for rep in range(2):
            for t in range(20):
                b.step(_acts(n, 500 + t))
            seq.append(b.env_levels())
            b.restore()
        assert np.array_equal(seq[0], seq[1])
    finally:
        b.close()


def test_checkpoint_replay_keeps_level():
    from nclone_amd.vec_env import NppVecEnvironment

    levels = _levels()
    env = NppVecEnvironment(levels, 256, truncation_limit=60, level_weights=_weights(len(levels)), level_seed=1)
    try:
        env.reset(seed=2)
        for t in range(50):
            env.step(np.random.default_rng(t).integers(0, 6, 256))
        lv = env.batch.env_levels()
        obs, info = env.reset(options={"checkpoint": [2, 2, 0, 3]})
        assert info["checkpoint_replay"] and np.array_equal(env.batch.env_levels(), lv)
        env.snapshot()
        obs, info = env.reset(options={"checkpoint": "snapshot"})
        assert np.array_equal(env.batch.env_levels(), lv)
        env.reset()   # a plain reset draws
        assert np.any(env.batch.env_levels() != lv)
    finally:
        env.close()


def test_step_many_does_not_draw():
    levels = _levels()
    n = 256
    b = _batch(levels, n, fast_reset=True)
    try:
        b.set_level_pool(_weights(len(levels)), seed=8)
        lv = b.env_levels()
        acts = torch.from_numpy(np.random.default_rng(0).integers(0, 6, size=(40, n)).astype(np.uint8)).cuda()
        flags, _r, _f = b.step_many(acts)
        assert ((flags.cpu().numpy() & 11) != 0).any()   # episodes did end (and restarted on the spot)
        assert np.array_equal(b.env_levels(), lv)
    finally:
        b.close()


def test_pool_off_is_byte_identical():
    """A handle whose pool was switched on and off again, and a vector env without level_weights, against plain handles."""
    from nclone_amd.vec_env import NppVecEnvironment

    levels = _levels()
    n = 512
    outs = []
    for toggle in (False, True):
        b = _batch(levels, n, fast_reset=True, outputs=("spatial_context", "positions"))
        if toggle:
            b.set_level_pool(_weights(len(levels)), seed=1)
            b.set_level_pool(None)
        rows = []
        for t in range(100):
            b.step(_acts(n, t))
            rows.append(b.out.dev.cpu().numpy().copy())
        rows.append(b.dump_state()[0])
        outs.append(rows)
        b.close()
    for a, c in zip(*outs):
        assert np.array_equal(a, c, equal_nan=True)
    e1 = NppVecEnvironment(levels, n, output="numpy", truncation_limit=60)
    e2 = NppVecEnvironment(levels, n, output="numpy", truncation_limit=60, level_weights=None)
    try:
        o1, _ = e1.reset(seed=0)
        o2, _ = e2.reset(seed=0)
        for t in range(60):
            a = np.random.default_rng(t).integers(0, 6, n)
            o1, r1, _, _, i1 = e1.step(a)
            o2, r2, _, _, i2 = e2.step(a)
            for k in o1:
                assert np.array_equal(o1[k], o2[k], equal_nan=True), (t, k)
            assert np.array_equal(i1["level_id"], (np.arange(n) // 64) % len(levels))
    finally:
        _close(e1, e2)
