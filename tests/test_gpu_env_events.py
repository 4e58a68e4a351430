"""GPU test of the per-env features that live beside the step kernel -- action routes, path-direction action masking
(19), reward mode "pbrs" (20) with its waypoints (23), episode statistics (24) -- as the events of the other entry points reach them:
reset, snapshot and archive restore, raw ticks, an injected state, npp_step_many, the level pool's redraws.  The idea is a twin:
batch A has all four on, the batches B_k exactly one each; all get the same levels, actions and events.  After every event, and
after the step and the feature's own call that follow it, each feature's visible state in A equals B_k's bit for bit, and the envs
outside the event's selection are as they were before.  Every step but the first runs without flags / frames rows in the caller's
output block, so the consumers read rows the handle owns.  It pins what the features do today, for a later change of how the
events are dispatched."""
import ctypes as C

import numpy as np
import pytest

from tests.test_gpu_episode import _cuda, _mixed_actions, _three_levels

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

FEATURES = ("routes", "mask", "reward", "episode")
# the axis of the env index in every per-env piece of visible state (the level table has none)
AXIS = {"route_act": 0, "route_hdr": 0, "observed": 0, "applied": 0, "last_observed": 0, "last_applied": 0, "action_mask": 0,
        "direction": 0, "reward": 0, "components": 0, "wp_bonus": 0, "wp_info": 0, "ep_i32": 1, "ep_f64": 1}
KEYS = {"routes": ("route_act", "route_hdr"),
        "mask": ("observed", "applied", "last_observed", "last_applied", "action_mask", "direction"),
        "reward": ("reward", "components", "wp_bonus", "wp_info"),
        "episode": ("ep_i32", "ep_f64", "ep_table")}


def _make(levels, n, ids, feats, pool):
    from nclone_amd.engine import NppBatch

    b = NppBatch(n, autoreset=True, outputs=("positions", "reward_components", "path_direction"), fast_reset=False)
    b.feats = feats
    b.load_levels(levels)
    b.assign_levels(np.asarray(ids, dtype=np.int32))
    b.set_truncation_limit(48)   # an auto-reset every 12 steps at the latest
    if "routes" in feats:
        b.set_routes(64)
    if pool:
        b.set_level_pool([1.0, 2.0], seed=5)
    else:
        b.archive_create(8)
    if "mask" in feats:
        b.set_action_masking("hard")
    if "reward" in feats:
        b.set_reward_mode("pbrs")
        b.set_reward_waypoints(True)
        b.wp_bonus = torch.zeros(n, dtype=torch.float32, device="cuda")
        b.wp_info = torch.zeros((n, 3), dtype=torch.int32, device="cuda")
    if "episode" in feats:
        b.set_episode_stats(True)
    b.reset()
    return b


def _state(b):
    b.sync()
    s = {}
    if "routes" in b.feats:
        s["route_act"], s["route_hdr"] = b.route_views()
    if "mask" in b.feats:
        s.update(b.path_mask_stats())
        s["action_mask"], s["direction"] = b.action_mask, b.out.t["path_direction"]
    if "reward" in b.feats:
        s["reward"], s["components"], s["wp_bonus"], s["wp_info"] = b.reward, b.out.t["reward_components"], b.wp_bonus, b.wp_info
    if "episode" in b.feats:
        v = b.episode_views()
        s["ep_i32"], s["ep_f64"], s["ep_table"] = v["i32"], v["f64"], v["table"]
    return {k: v.cpu().numpy().copy() for k, v in s.items()}


def _same(x, y):
    return x.shape == y.shape and np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8))


class Twin:
    def __init__(self, levels, n, ids, pool=False):
        self.n = n
        self.a = _make(levels, n, ids, FEATURES, pool)
        self.b = {k: _make(levels, n, ids, (k,), pool) for k in FEATURES}
        self.all = [self.a] + list(self.b.values())
        self.check("switch-on and reset")

    def close(self):
        for b in self.all:
            b.close()

    def check(self, what, before=None, selected=None):
        """A against every B_k; with `before` (A's state ahead of an event) the envs outside `selected` have not changed"""
        sa = _state(self.a)
        for k in FEATURES:
            sb = _state(self.b[k])
            for key in KEYS[k]:
                assert _same(sa[key], sb[key]), (what, k, key)
        if before is not None:
            keep = ~np.asarray(selected, dtype=bool)
            for key, axis in AXIS.items():
                assert _same(np.compress(keep, before[key], axis=axis), np.compress(keep, sa[key], axis=axis)), (what, key, "outside the selection")
        return sa

    def event(self, what, fn, selected):
        """`selected`: the envs the event may touch, or a function that says so once the event has run"""
        before = _state(self.a)
        for b in self.all:
            fn(b)
        return self.check(what, before, selected() if callable(selected) else selected)

    def _consume(self, b, flags, frames, reward, comps, n_steps=1):
        if "mask" in b.feats:
            b.path_action_mask()
        if "reward" in b.feats and b._reward_mode:
            b.step_reward(wp_bonus_out=b.wp_bonus, wp_info_out=b.wp_info)
        if "episode" in b.feats:
            b.episode_accumulate(flags, frames, reward, comps, n_steps=n_steps)

    def step(self, act, what, rows=False):
        """one npp_step of every batch and the calls that follow it.  B_episode steps with the block's rows (no consumer of the
        handle's rows is on there) and lends them to A's accumulation; the reward rows of both accumulations are A's."""
        from nclone_amd import _native as nat

        for b in self.all:
            if rows or b is self.b["episode"]:
                b.step(act)
                continue
            out = nat.StepOut()
            C.memmove(C.byref(out), C.byref(b._out), C.sizeof(nat.StepOut))
            out.d_flags = out.d_frames = None
            nat.check(b.h, b.lib.npp_step(b.h, C.c_void_p(act.data_ptr()), 4, C.byref(out)))
            b._reward_pending = bool(b._reward_mode)
        e = self.b["episode"]
        pbrs = bool(self.a._reward_mode)
        reward, comps = (self.a.reward, self.a.out.t["reward_components"]) if pbrs else (e.reward, None)
        for b in self.all:
            self._consume(b, e.flags, e.frames, reward, comps)
        return self.check(what)

    def step_many(self, act, what):
        """npp_step_many without rows of the caller's: the routes' append walks the handle's, grown to len(act) rows here"""
        from nclone_amd import _native as nat

        e = self.b["episode"]
        flags, reward, frames = e.step_many(act)
        for b in self.all:
            if b is e:
                continue
            out = nat.StepOut()
            C.memmove(C.byref(out), C.byref(b._out_min), C.sizeof(nat.StepOut))
            out.d_flags = out.d_frames = out.d_work = None
            b.keep = torch.zeros_like(reward)   # [len(act)][n] rows, as every row pointer of this entry
            out.d_reward = b.keep.data_ptr()
            nat.check(b.h, b.lib.npp_step_many(b.h, C.c_void_p(act.data_ptr()), len(act), 4, C.byref(out)))
        for b in self.all:
            self._consume(b, flags, frames, reward, None, n_steps=len(act))
        return self.check(what)


def _restore_lists(n, length):
    """`length` entries, the envs distinct (a list longer than the batch is padded with skipped entries, env -1); an entry names
    the slot that holds its env's level (slot l holds env l, which plays level l), every third one the empty slot 2"""
    envs = np.full(length, -1, dtype=np.int32)
    k = min(length, n)
    envs[:k] = np.random.default_rng(7).permutation(n)[:k]
    slots = np.where(envs >= 0, envs % 2, 0).astype(np.int32)
    slots[2::3] = 2
    return envs, slots


@pytest.mark.parametrize("n,length", [(1, 3), (67, 3), (300, 260)])
def test_events_reach_every_feature_alike(n, length):
    z, ks, levels = _three_levels()
    ids = np.arange(n) % 2
    t = Twin(levels, n, ids)
    act = _mixed_actions(z, ks, ids, n, 64, 11) if n >= 8 else _cuda(z["aact%d" % ks[0]][:64, None].astype(np.uint8))
    at = iter(range(64))

    def steps(count, what):
        for _ in range(count):
            i = next(at)
            t.step(act[i], (what, i))

    t.step(act[next(at)], "first step, with the caller's rows", rows=True)
    steps(3, "steps")
    # 1. masked reset
    mask = (np.arange(n) % 3 != 1).astype(np.uint8)
    mask[0], mask[-1] = 1, 0 if n > 1 else 1
    t.event("masked reset", lambda b: b.reset(mask), mask)
    steps(2, "after the reset")
    # 2. snapshot, steps, masked restore
    for b in t.all:
        b.snapshot()
    steps(3, "after the snapshot")
    mask = (np.arange(n) % 4 != 2).astype(np.uint8)
    t.event("masked restore", lambda b: b.restore(mask), mask)
    steps(2, "after the restore")
    # 3. archive store, then restores of a list with an empty slot: with the caller's status row and without
    stored = np.arange(min(2, n), dtype=np.int32)   # one env of each level
    for b in t.all:
        assert not b.archive_store(stored, stored, status=True).cpu().numpy().any()
    steps(3, "after the store")
    envs, slots = _restore_lists(n, length)
    status = []
    restored = np.zeros(n, dtype=bool)

    def took():   # only the entries with status 0 touch their env
        st = status[0].cpu().numpy()
        assert all(np.array_equal(st, s.cpu().numpy()) for s in status)
        assert (st == 0).any() and (st[slots == 2] != 0).all(), st
        restored[envs[st == 0]] = True
        return restored

    t.event("archive restore, the caller's status", lambda b: status.append(b.archive_restore(envs, slots, status=True)), took)
    steps(2, "after the archive restore with status")
    # (the same lists again: levels and slots are as they were, so the same entries restore)
    t.event("archive restore, no status", lambda b: b.archive_restore(envs, slots), restored)
    steps(2, "after the archive restore without status")
    # 4. raw ticks
    ticks = _cuda(np.zeros((3, n), dtype=np.uint8))
    t.event("tick", lambda b: b.tick(ticks), np.ones(n, dtype=bool))
    steps(2, "after the ticks")
    # 5. an injected state on a range of envs
    env0, count = n // 3, max(1, n // 2)
    xyv = t.a.dump_state()[0][env0:env0 + count, :4].copy()
    xyv[:, 0] += 0.25
    sel = np.zeros(n, dtype=bool)
    sel[env0:env0 + count] = True
    t.event("set_ninja_state", lambda b: b.set_ninja_state(xyv, env0), sel)
    steps(2, "after the injection")
    # 6. three steps in one launch: the C entry refuses it while reward mode "pbrs" is on, so that goes off and comes back
    for b in t.all:
        if "reward" in b.feats:
            b.set_reward_mode("sparse")
    i = next(at)
    t.step_many(act[i:i + 3].contiguous(), "step_many")
    next(at), next(at)
    steps(1, "after step_many, reward mode off")
    for b in t.all:
        if "reward" in b.feats:
            b.set_reward_mode("pbrs")
            b.set_reward_waypoints(True)
    steps(2, "after step_many, reward mode on again")
    sa = t.check("end")   # (the run was not vacuous)
    assert sa["route_hdr"].any() and sa["observed"].any() and np.abs(sa["components"]).sum() > 0
    if n > 1:
        assert sa["ep_table"][:, 0].sum() > 0 and sa["last_observed"].any()
    t.close()


def test_level_pool_redraws_reach_every_feature_alike():
    """the level pool in place of the archive (the archive calls are refused while a pool is on): auto-reset steps redraw behind
    the step, npp_draw_levels under a mask redraws without one"""
    z, ks, levels = _three_levels()
    n = 67
    ids = np.arange(n) % 2
    t = Twin(levels[:2], n, ids, pool=True)
    act = _mixed_actions(z, ks, ids, n, 40, 12)
    t.step(act[0], "first step, with the caller's rows", rows=True)
    for i in range(1, 16):
        t.step(act[i], ("pool step", i))
    before = t.a.env_levels()
    mask = (np.arange(n) % 3 != 0).astype(np.uint8)
    t.event("draw_levels", lambda b: b.draw_levels(mask), mask)
    after = t.a.env_levels()
    assert (before != after).any() and (before == after)[mask == 0].all()
    assert all(np.array_equal(after, b.env_levels()) for b in t.all)
    for i in range(16, 32):
        t.step(act[i], ("pool step", i))
    assert t.check("end")["ep_table"][:, 0].sum() > 0
    t.close()
