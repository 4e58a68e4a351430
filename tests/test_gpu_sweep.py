"""The evaluation sweep on the device (npp_sweep.hip behind the step and behind the episode accumulation).

Twin run, as tests/test_gpu_level_pool.py does it: the sweep env runs beside a twin that never had a sweep.  After every step the
twin is given the levels tests/sweep_ref.py predicts (npp_assign_levels for the envs whose level changed) and is observed; every
observation key, the flags, info["level_id"], the state dump and the entity checksums must match byte for byte, and env_job, next,
done and the result rows must equal the model, whose rows Python collects from the info["episode"] stream."""
import ctypes as C

import numpy as np
import pytest
import torch

from nclone_amd import _native as nat

from tests.sweep_ref import SweepModel
from tests.test_gpu_level_pool import Twin, _close, _compare, _np

pytestmark = pytest.mark.gpu

TRUNC = 60   # frames: an episode lasts 15 steps at the most, so jobs end often


def _levels():
    """mines, doors and one zoo level"""
    from nclone_amd.levels import door_levels, mine_levels, zoo_levels

    return mine_levels()[0][:3] + door_levels()[0][:3] + zoo_levels()[0][:1]


class _Draws:
    """what Twin.step asks its model: the envs that change level after this step, and the levels they go to"""

    def __init__(self, model):
        self.m = model

    def draw(self, ended):
        ch = np.flatnonzero(self.m.assign(ended.astype(np.uint8), bits=1))
        return ch, self.m.env_level[ch].copy()


class _Expected:
    """the result planes as Python builds them from the info["episode"] stream"""

    def __init__(self, J):
        self.i = {k: np.zeros(J, dtype=np.int64) for k in ("steps", "frames", "switch", "switch_frames", "level", "won", "status")}
        self.i["env"] = np.full(J, -1, dtype=np.int64)
        self.r = np.zeros(J, dtype=np.float64)

    def take(self, model, info):
        ended = _np(info["_episode"])
        ep = {k: _np(v) for k, v in info["episode"].items()}
        for e in np.flatnonzero(model.prev_job >= 0):
            assert ended[e], ("an env ended a job without reporting an episode", int(e))
            j = int(model.prev_job[e])
            self.i["steps"][j], self.i["frames"][j] = ep["steps"][e], ep["l"][e]
            self.i["switch"][j] = bool(ep["switch_activated"][e])
            self.i["switch_frames"][j] = ep["switch_activation_frame"][e]
            self.i["level"][j], self.i["won"][j], self.i["env"][j], self.i["status"][j] = ep["level_id"][e], bool(ep["is_success"][e]), e, 1
            self.r[j] = ep["r"][e]
        model.collect(lambda e: True)

    def check(self, t, env, model, info=None):
        s = env.batch.sweep_state()
        i32, f64 = s["i32"].cpu().numpy().astype(np.int64), s["f64"].cpu().numpy()
        assert np.array_equal(s["env_job"].cpu().numpy(), model.env_job), (t, "env_job")
        assert s["counters"].cpu().numpy().tolist() == [model.next, model.done, model.J], (t, "counters")
        if info is not None:
            assert np.array_equal(_np(info["evaluation"]["job"]), model.env_job), (t, "info job")
            assert np.array_equal(_np(info["evaluation"]["active"]), model.env_job >= 0), (t, "info active")
        steps, frames, sw_step, sw_frames, level, _bits, flags, who, status = i32
        x = self.i
        assert np.array_equal(status, x["status"]), (t, "status")
        assert np.array_equal(who, x["env"]), (t, "env")
        assert np.array_equal(steps, x["steps"]) and np.array_equal(frames, x["frames"]), (t, "lengths")
        assert np.array_equal(sw_step != 0, x["switch"] != 0), (t, "switch")
        assert np.array_equal(np.where(sw_step != 0, sw_frames, -1)[status != 0], x["switch_frames"][status != 0]), (t, "switch frames")
        assert np.array_equal(level, x["level"]) and np.array_equal(flags & 1, x["won"]), (t, "level / won")
        assert np.array_equal(level[status != 0], model.jobs[status != 0]), (t, "the episode ran on the job's level")
        assert np.array_equal(f64[0].view(np.int64), self.r.view(np.int64)), (t, "return")


def _twin_run(n, n_list, K, after_stop=0):
    from nclone_amd.vec_env import NppVecEnvironment

    levels = _levels()
    rng = np.random.default_rng(1000 + n)
    lv_list = rng.integers(0, len(levels), size=n_list).astype(np.int32)
    if n == 1:
        lv_list = np.array([0, 6, 6], dtype=np.int32)   # the env's own level, then the zoo level, then the zoo level again
    jobs = np.tile(lv_list, K)
    J = len(jobs)
    init = (np.arange(n) % len(levels)).astype(np.int32)
    kw = dict(truncation_limit=TRUNC, level_ids=init)
    env = NppVecEnvironment(levels, n, output="torch", episode_stats=True, **kw)
    twin = Twin(levels, n, None, **kw)
    try:
        model, exp = SweepModel(n, jobs, init), _Expected(J)
        obs, info0 = env.start_evaluation(lv_list, K)
        assert info0["evaluation"]["jobs"] == J
        idx = model.start()   # every env with a job is reset on its level, whether the level is another one or not
        twin.b.assign_levels(jobs[idx], env_ids=idx)
        twin.cur[idx] = jobs[idx]
        twin.model = _Draws(model)
        tw, _ = twin.env._reset_return({})
        _compare(-1, obs, {}, tw, None, env.batch, twin.b)
        exp.check(-1, env, model)
        limit = (TRUNC // 4) * (-(-J // n) + 2)
        acts = rng.integers(0, 6, size=(limit + after_stop, n)).astype(np.uint8)
        changed = same = 0
        t = 0
        while model.done < J:
            assert t < limit, "the sweep did not finish"
            obs, rew, te, tr, info = env.step(acts[t])
            tw, rew2, te2, tr2, info2, ch = twin.step(acts[t])
            assert np.array_equal(_np(rew), rew2) and np.array_equal(_np(te), te2) and np.array_equal(_np(tr), tr2), t
            _compare(t, obs, info, tw, info2, env.batch, twin.b)
            took = int((model.prev_job >= 0).sum() - (model.env_job[model.prev_job >= 0] < 0).sum())
            changed += len(ch)
            same += took - len(ch)
            exp.take(model, info)
            exp.check(t, env, model, info)
            t += 1
        if J > n:   # jobs were handed out behind steps: some landed on another level and some on the level the env played
            assert changed > 0 and same > 0, (changed, same)
        else:
            assert changed == 0 and same == 0 and model.next == J + J
        assert env.evaluation_done()
        # completeness: every job done exactly once (the model refuses a second end), by an env that held it; idle envs wrote nothing
        res = env.evaluation_results()
        assert np.array_equal(_np(res["level"]), jobs) and bool(_np(res["done"]).all())
        assert np.array_equal(_np(res["env"]), exp.i["env"]) and np.array_equal(_np(res["frames"]), exp.i["frames"])
        if J < n:
            assert _np(res["env"]).max() < J   # the envs that were idle from the start never played a job
        per = res["per_level"]
        assert np.array_equal(_np(per["episodes"]), np.full(n_list, K))
        assert np.array_equal(_np(per["success_rate"]), exp.i["won"].reshape(K, n_list).astype(np.float64).sum(axis=0) / K)
        assert np.array_equal(_np(per["mean_return"]), exp.r.reshape(K, n_list).sum(axis=0) / K)
        if after_stop:
            # life cycle: after the stop the handle steps with the bytes of one that never had a sweep, results still readable
            env.stop_evaluation()
            for k in range(after_stop):
                obs, rew, te, tr, info = env.step(acts[limit + k])
                assert "evaluation" not in info
                tw, rew2, te2, tr2, info2, ch = twin.step(np.asarray(acts[limit + k]))
                assert len(ch) == 0
                _compare(("after stop", k), obs, info, tw, info2, env.batch, twin.b)
            assert np.array_equal(_np(env.evaluation_results()["frames"]), exp.i["frames"])
    finally:
        _close(env, twin.env)


def test_sweep_twin_one_env():
    _twin_run(1, 3, 1)


def test_sweep_twin_67_queue_runs_dry_in_mid_batch():
    _twin_run(67, 103, 2)   # J = 3 n + 5: a wavefront boundary inside the batch


def test_sweep_twin_300_idle_from_the_start():
    _twin_run(300, 50, 2, after_stop=20)   # J = 100 < n: the batch crosses the 256-lane chunk


def test_sweep_twin_1100_crosses_the_round():
    _twin_run(1100, 625, 4)   # J = 2500: the batch crosses the 1024-env round


def _sweep_env(n, levels, **kw):
    from nclone_amd.vec_env import NppVecEnvironment

    return NppVecEnvironment(levels, n, output="torch", episode_stats=True, **kw)


def test_everyone_ends_at_once():
    """n = 1100 on one level with a truncation limit of two steps: all envs end in the same launch, so the ranks must be 0 .. 1099 in
    env order across wavefronts, chunks and rounds -- the smallest shape at which the carry across rounds can be wrong."""
    from nclone_amd.levels import curriculum0_levels

    n, J = 1100, 2500
    levels = curriculum0_levels()[0][:2]
    jobs = np.tile(np.array([0, 1], dtype=np.int32), J // 2)   # the jobs alternate between the two levels
    env = _sweep_env(n, levels, truncation_limit=8, level_ids=np.zeros(n, dtype=np.int32))
    try:
        env.start_evaluation([0, 1], J // 2)
        model = SweepModel(n, jobs, np.zeros(n, dtype=np.int32))
        model.start()
        rng = np.random.default_rng(5)
        rounds = 0
        for t in range(16):
            if model.done == J:
                break
            _, _, te, tr, info = env.step(rng.integers(0, 6, size=n).astype(np.uint8))
            flags = env.batch.flags.cpu().numpy()
            ended = (flags & 11) != 0
            assert ended.all() or not ended.any(), "the level was meant to be survived for two steps by every env"
            before = model.env_job.copy()
            model.assign(flags)
            model.collect(lambda e: True)
            s = env.batch.sweep_state()
            job = s["env_job"].cpu().numpy()
            assert np.array_equal(job, model.env_job), t
            assert s["counters"].cpu().numpy().tolist() == [model.next, model.done, J], t
            assert np.array_equal(env.batch.env_levels(), model.env_level), t
            if ended.all() and rounds == 0:
                assert np.array_equal(before, np.arange(n)) and np.array_equal(job, n + np.arange(n)), "ranks 0 .. n - 1 in env order"
            if ended.all() and rounds == 1:   # 300 jobs are left: the first 300 envs take them, the others find the list used up
                assert np.array_equal(job[:300], 2 * n + np.arange(300)) and (job[300:] == -1).all()
            rounds += int(ended.all())
        assert rounds >= 3 and model.done == J
        res = env.evaluation_results()
        assert bool(_np(res["done"]).all()) and bool(_np(res["truncated"]).all())
        assert np.array_equal(_np(res["env"])[:2 * n], np.tile(np.arange(n), 2)) and np.array_equal(_np(res["env"])[2 * n:], np.arange(300))
    finally:
        _close(env)


def _planes(n, lv_list, K, steps):
    levels = _levels()
    env = _sweep_env(n, levels, truncation_limit=TRUNC, level_ids=(np.arange(n) % len(levels)).astype(np.int32))
    try:
        env.start_evaluation(lv_list, K)
        acts = np.random.default_rng(77).integers(0, 6, size=(steps, n)).astype(np.uint8)
        for t in range(steps):
            env.step(acts[t])
        s = env.batch.sweep_state()
        f64, i32 = env.batch.dump_state()
        return [s["i32"].cpu().numpy(), s["f64"].cpu().numpy().view(np.int64), s["env_job"].cpu().numpy(), s["counters"].cpu().numpy(),
                env.batch.env_levels(), f64.view(np.int64), i32]
    finally:
        _close(env)


def test_sweep_reproducible():
    lv_list = np.random.default_rng(3).integers(0, 7, size=150).astype(np.int32)
    a = _planes(257, lv_list, 4, 50)
    b = _planes(257, lv_list, 4, 50)
    assert a[3][1] > 257   # (jobs did finish, beyond the first hand-out)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)


def test_second_start_begins_clean_and_load_levels_ends_the_sweep():
    levels = _levels()
    n = 67
    env = _sweep_env(n, levels, truncation_limit=TRUNC)
    try:
        rng = np.random.default_rng(11)
        env.start_evaluation([0, 3, 6], 30)
        for t in range(20):
            env.step(rng.integers(0, 6, size=n).astype(np.uint8))
        assert int(env.batch.sweep_state()["counters"][1]) > 0
        env.start_evaluation([6, 1], 2)   # J = 4 < n
        s = env.batch.sweep_state()
        assert s["counters"].cpu().numpy().tolist() == [4, 0, 4]
        assert s["env_job"].cpu().numpy().tolist() == [0, 1, 2, 3] + [-1] * (n - 4)
        assert not s["i32"][:7].cpu().numpy().any() and (s["i32"][7].cpu().numpy() == -1).all() and not s["f64"].cpu().numpy().any()
        assert not s["status"].cpu().numpy().any()
        assert env.batch.env_levels()[:4].tolist() == [6, 1, 6, 1]
        res = env.evaluate(lambda obs: rng.integers(0, 6, size=n).astype(np.uint8), [6, 1], 2, max_steps=40, check_every=4)
        assert bool(_np(res["done"]).all()) and sorted(_np(res["env"]).tolist()) == [0, 1, 2, 3]
        env.start_evaluation([2], 1)
        env.batch.load_levels(levels[:2])   # a new level set ends the sweep and drops its results
        with pytest.raises(ValueError, match="sweep_start"):
            env.batch.sweep_state()
        assert env.batch.lib.npp_sweep_view(env.batch.h, None, None, None, None, None) == nat.NPP_ERR_STATE
        env.batch.assign_levels(np.ones(n, dtype=np.int32))   # (refused while a sweep runs)
    finally:
        _close(env)


def _refused(fn, fragment, code=None):
    with pytest.raises(nat.NppError) as e:
        fn()
    assert e.value.code == (nat.NPP_ERR_STATE if code is None else code) and fragment in str(e.value), str(e.value)


def test_refusals():
    from nclone_amd.engine import NppBatch

    levels = _levels()
    jobs = np.array([0, 1, 2], dtype=np.int32)

    def batch(**kw):
        b = NppBatch(16, **kw)
        b.load_levels(levels)
        return b

    def raw_start(b, j, count):
        nat.check(b.h, b.lib.npp_sweep_start(b.h, j.ctypes.data_as(C.c_void_p), count))

    b = batch()
    try:
        _refused(lambda: b.sweep_start(jobs), "episode statistics are off")
        b.set_episode_stats(True)
        _refused(lambda: raw_start(b, jobs, 0), "n_jobs must be > 0")
        _refused(lambda: raw_start(b, np.array([0, 7], dtype=np.int32), 2), "names level 7", nat.NPP_ERR_INVALID)
        with pytest.raises(ValueError, match="names level -1"):
            b.sweep_start([0, -1])
        b.set_level_pool(np.ones(len(levels)))
        _refused(lambda: b.sweep_start(jobs), "the level pool is on")
        b.set_level_pool(None)
        b.archive_create(4)
        _refused(lambda: b.sweep_start(jobs), "a checkpoint archive exists")
        b.archive_create(0)
        b.set_entity_pos(0, 0, 100.0, 100.0)
        _refused(lambda: b.sweep_start(jobs), "repositioned")
        b.set_entity_pos(0, 0, float("nan"), float("nan"))
        b.snapshot()
        # while a sweep runs
        b.sweep_start(jobs)
        run = "an evaluation sweep is running"
        _refused(lambda: b.set_level_pool(np.ones(len(levels))), "npp_set_level_pool: " + run)
        _refused(lambda: b.set_goal_curriculum(True), "npp_set_goal_curriculum: " + run)
        _refused(lambda: b.archive_create(4), "npp_archive_create: " + run)
        _refused(lambda: b.assign_levels(np.zeros(16, dtype=np.int32)), "npp_assign_levels: " + run)
        _refused(lambda: b.set_entity_pos(0, 0, 100.0, 100.0), "npp_set_entity_pos: " + run)
        _refused(lambda: b.snapshot(), "npp_snapshot: " + run)
        _refused(lambda: b.restore(), "npp_restore: " + run)
        one, off, lv = np.zeros(4, dtype=np.uint8), np.array([0, 4], dtype=np.int64), np.zeros(1, dtype=np.int32)
        p = [x.ctypes.data_as(C.c_void_p) for x in (one, off, lv)]
        _refused(lambda: nat.check(b.h, b.lib.npp_demo_create(b.h, p[0], p[1], p[2], 1, 1, 0, 0)), "npp_demo_create: " + run)
        _refused(lambda: nat.check(b.h, b.lib.npp_archive_seed(b.h, p[0], p[1], p[2], 1, 0, None, None)), "npp_archive_seed: " + run)
        b.set_episode_stats(False)   # ends the sweep
        b.assign_levels(np.zeros(16, dtype=np.int32))
    finally:
        b.close()
    from nclone_amd.levels import curriculum0_levels

    b = NppBatch(16)
    try:
        b.load_levels(curriculum0_levels()[0][:2])
        b.set_goal_curriculum(True)   # (reloads the level set: switched on before the episode statistics)
        b.set_episode_stats(True)
        _refused(lambda: b.sweep_start(np.zeros(2, dtype=np.int32)), "the goal curriculum is on")
    finally:
        b.close()
    b = batch(autoreset=False)
    try:
        b.set_episode_stats(True)
        _refused(lambda: b.sweep_start(jobs), "NPP_FLAG_AUTORESET")
    finally:
        b.close()
        torch.cuda.synchronize()


@pytest.mark.parametrize("reward_mode", ["sparse", "pbrs"])
def test_evaluate_matches_the_episode_stream(reward_mode):
    from nclone_amd.async_env import NppAsyncVecEnvironment
    from nclone_amd.levels import curriculum0_levels, mine_levels
    from nclone_amd.vec_env import NppVecEnvironment

    n, K = 67, 3
    levels = mine_levels()[0][:3] + curriculum0_levels()[0][:2]
    L = len(levels)
    env = NppVecEnvironment(levels, n, output="numpy", episode_stats=True, truncation_limit=TRUNC, reward_mode=reward_mode)
    try:
        rng = np.random.default_rng(2024)
        model = SweepModel(n, np.tile(np.arange(L), K), np.zeros(n))
        model.start()
        stream = {}   # job -> (won, return, frames, components) as info["episode"] reported them

        # the policy sees every observation; the stream is read off the env's own step()
        inner = env.step

        def step(actions):
            out = inner(actions)
            info = out[4]
            model.assign(env.batch.flags.cpu().numpy())
            ep = info["episode"]
            for e in np.flatnonzero(model.prev_job >= 0):
                assert info["_episode"][e]
                stream[int(model.prev_job[e])] = (bool(ep["is_success"][e]), float(ep["r"][e]), int(ep["l"][e]),
                                                  float(ep["pbrs_total"][e]) if reward_mode == "pbrs" else 0.0)
            model.collect(lambda e: True)
            return out

        env.step = step
        res = env.evaluate(lambda obs: rng.integers(0, 6, size=n).astype(np.uint8), episodes_per_level=K, max_steps=200, check_every=5)
        assert res["done"].all() and sorted(stream) == list(range(L * K))
        assert np.array_equal(res["level"], np.tile(np.arange(L), K))
        won = np.array([stream[j][0] for j in range(L * K)])
        ret = np.array([stream[j][1] for j in range(L * K)], dtype=np.float64)
        frames = np.array([stream[j][2] for j in range(L * K)])
        assert np.array_equal(res["is_success"], won) and np.array_equal(res["r"], ret) and np.array_equal(res["frames"], frames)
        per = res["per_level"]
        assert np.array_equal(per["episodes"], np.full(L, K))
        assert np.array_equal(per["success_rate"], won.reshape(K, L).astype(np.float64).sum(axis=0) / K)
        assert np.array_equal(per["mean_return"], ret.reshape(K, L).sum(axis=0) / K)
        assert np.array_equal(per["mean_frames"], frames.reshape(K, L).astype(np.float64).sum(axis=0) / K)
        if reward_mode == "pbrs":
            assert res["pbrs_components"].shape == (L * K, 6)
            assert np.array_equal(res["pbrs_components"][:, 0], np.array([stream[j][3] for j in range(L * K)]))
        else:
            assert "pbrs_components" not in res
        # reset() in the middle of an evaluation is refused
        env.step = inner
        env.start_evaluation(episodes_per_level=1)
        with pytest.raises(RuntimeError, match="start_evaluation"):
            env.reset()
        env.stop_evaluation()
        env.reset()
    finally:
        _close(env)
    if reward_mode == "sparse":
        a = NppAsyncVecEnvironment(levels, 64, n_streams=2, truncation_limit=TRUNC)
        try:
            with pytest.raises(NotImplementedError, match="evaluation sweep"):
                a.start_evaluation()
            with pytest.raises(NotImplementedError, match="evaluation sweep"):
                a.evaluate(lambda obs: None)
        finally:
            a.close()
            torch.cuda.synchronize()


def test_start_evaluation_needs_episode_stats():
    from nclone_amd.vec_env import NppVecEnvironment

    env = NppVecEnvironment(_levels(), 16, truncation_limit=TRUNC)
    try:
        with pytest.raises(RuntimeError, match="episode_stats"):
            env.start_evaluation()
    finally:
        _close(env)
