"""GPU tests of the sequential path waypoints of reward mode "pbrs" (npp_set_reward_waypoints / npp_step_reward_wp):
the device kernels along the reference's own rollouts of tests/golden/waypoints.npz and on levels the fixture never saw, against the
host build of the same rule (npp_reward_host_wp, which tests/test_waypoints_host.py pins to the fixture bit for bit) -- reward and
bonus as f32 bits, the collection state as integers --, the option off, observation overlap, restarts, the refusals and the host
classes.

The fixture's scripted rollout "e" places the ninja by assignment and is checked on the host only."""
import ctypes as C
import os

import numpy as np
import pytest

from tests.test_waypoints_host import host_reward_wp

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = ("reward", "positions", "flags", "frames")
END_ALL = 11   # won, dead, truncated: the flags bits after which the step kernel auto-resets
DEFAULT_WP = [18.0, 0.3, 2.0, 12.0]
SENTINEL_F, SENTINEL_I = -77.5, -77


@pytest.fixture(scope="module")
def lib():
    from nclone_amd import _native

    return _native.lib()


@pytest.fixture(scope="module")
def fix(lib):
    z = np.load(os.path.join(ROOT, "tests", "golden", "waypoints.npz"))
    names = bytes(z["names"]).decode().split("\n")
    ok = [k for k in range(len(names)) if not np.isinf(z["const%d" % k]).any()]   # (the reference raises on the seventh)
    assert len(ok) == 6 and z["params_wp"].tolist() == DEFAULT_WP
    return {"z": z, "names": names, "ok": ok, "levels": [z["m%d" % k] for k in range(len(names))]}


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _batch(levels, n, assign, waypoints=True, wp=None, autoreset=True, outputs=("positions",), **kw):
    from nclone_amd.engine import NppBatch

    b = NppBatch(n, autoreset=autoreset, outputs=outputs, fast_reset=False, **kw)   # the fixture resets with NPlayHeadless.reset()
    b.load_levels(levels)
    b.assign_levels(assign)
    b.set_truncation_limit(100000)
    b.reset()
    b.observe()
    b.set_reward_mode("pbrs")
    if waypoints:
        b.set_reward_waypoints(True, wp)
    return b


class Trace:
    """what the device produced per step, and the positions the host twin needs (row 0: the state before the first step)"""

    def __init__(self, b):
        self.b = b
        self.bonus = torch.full((b.n,), SENTINEL_F, dtype=torch.float32, device="cuda")
        self.info = torch.full((b.n, 3), SENTINEL_I, dtype=torch.int32, device="cuda")
        self.pos = [b.to_host(("positions",))["positions"][:, :2].copy()]
        self.rows = {k: [] for k in OUT + ("bonus", "info")}

    def step(self, act, skip=4):
        self.b.step(_cuda(act), frame_skip=skip)
        self.b.step_reward(wp_bonus_out=self.bonus, wp_info_out=self.info)
        h = self.b.to_host(OUT)
        for k in OUT:
            self.rows[k].append(h[k].copy())
        self.rows["bonus"].append(self.bonus.cpu().numpy().copy())
        self.rows["info"].append(self.info.cpu().numpy().copy())
        self.pos.append(h["positions"][:, :2].copy())

    def arrays(self):
        return {k: np.stack(v) for k, v in self.rows.items()}, np.stack(self.pos)

    def restart(self):
        """a reset / restore happened outside the step kernel: the twin starts again from here"""
        self.b.observe()   # (the block's positions are those of the last launch that wrote them)
        self.pos = [self.b.to_host(("positions",))["positions"][:, :2].copy()]
        self.rows = {k: [] for k in self.rows}


def _check_twin(lib, levels, assign, rows, pos, wp=DEFAULT_WP, end_bits=END_ALL, envs=None):
    """device == npp_reward_host_wp at the device's own positions, flags and frames: f32 bits of reward and bonus, the collection
    state as integers.  -> [in-sequence collections, out-of-sequence collections, episode ends after a collection]"""
    seen = np.zeros(3, int)
    for e in (range(pos.shape[1]) if envs is None else envs):
        fl = rows["flags"][:, e]
        rc, rew, _comp, _kind, bonus, info = host_reward_wp(lib, levels[assign[e]], pos[:, e], fl, rows["frames"][:, e].astype(np.uint16), wp,
                                                            end_bits=end_bits)
        assert rc == 0, e
        got, want = rows["reward"][:, e], rew.astype(np.float32)
        bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
        assert len(bad) == 0, (e, assign[e], bad[:5], got[bad[:5]], want[bad[:5]])
        assert np.array_equal(rows["bonus"][:, e].view(np.uint32), bonus.astype(np.float32).view(np.uint32)), e
        assert np.array_equal(rows["info"][:, e], info), (e, np.flatnonzero((rows["info"][:, e] != info).any(axis=1))[:5])
        ended = (fl & end_bits) != 0
        nxt0 = np.concatenate([[0], np.where(ended[:-1], 0, info[:-1, 1])])   # next expected before the step (within this trace)
        col = info[:, 0] >= 0
        seen += [int((col & (info[:, 0] == nxt0)).sum()), int((col & (info[:, 0] != nxt0)).sum()), int((ended & (info[:, 2] > 0)).sum())]
    return seen


def _follow(lib, fix, ks, n):
    """n envs, env e on level ks[e % len(ks)], along both recorded rollouts; every step of every env is compared"""
    z = fix["z"]
    lv = [ks[e % len(ks)] for e in range(n)]
    assign = np.arange(n) % len(ks)
    levels = [fix["levels"][k] for k in ks]
    b = _batch(levels, n, assign)
    checked = collected = 0
    for phase, skip in (("a", 4), ("b", 1)):
        steps = max(len(z["%sact%d" % (phase, k)]) for k in ks)
        act = np.zeros((n, steps), dtype=np.uint8)
        for e, k in enumerate(lv):
            a = z["%sact%d" % (phase, k)]
            act[e, :len(a)] = a
        if phase == "b":
            b.reset(mode="full")
            b.observe()
        tr = Trace(b)
        for t in range(steps):
            tr.step(act[:, t], skip)
        rows, pos = tr.arrays()
        _check_twin(lib, levels, assign, rows, pos)
        for e, k in enumerate(lv):   # hence the fixture: the device follows the recorded trajectory and returns the recorded numbers
            m = len(z["%sact%d" % (phase, k)])
            tag = (phase, fix["names"][k])
            assert np.array_equal(pos[:m + 1, e], z["%spos%d" % (phase, k)]), tag
            assert np.array_equal(rows["flags"][:m, e] & 7, z["%sflags%d" % (phase, k)]), tag
            assert np.array_equal(rows["frames"][:m, e], z["%sframes%d" % (phase, k)]), tag
            want = z["%srew%d" % (phase, k)].astype(np.float32)
            assert np.array_equal(rows["reward"][:m, e].view(np.uint32), want.view(np.uint32)), tag
            wb, wi = z["%swpb%d" % (phase, k)], z["%swpi%d" % (phase, k)]
            assert np.array_equal(rows["bonus"][:m, e].view(np.uint32), wb.astype(np.float32).view(np.uint32)), tag
            assert np.array_equal(rows["info"][:m, e], wi[:, [0, 2, 3]]), tag
            checked += m
            collected += int((wi[:, 0] >= 0).sum())
    b.close()
    return checked, collected


def test_rollouts_on_the_device_67_envs(lib, fix):
    """The six levels the mode accepts, mixed inside one wavefront, plus a three-lane tail; with in-kernel auto-reset."""
    checked, collected = _follow(lib, fix, fix["ok"], 67)
    assert checked > 67 * 300 and collected > 1000


def test_rollouts_on_the_device_single_env(lib, fix):
    k = fix["names"].index("zoo:replay:16")
    checked, collected = _follow(lib, fix, [k], 1)
    assert checked == 300 + len(fix["z"]["bact%d" % k]) and collected >= 40


def test_non_default_params(lib, fix):
    z, k = fix["z"], 0
    par = z["params_wp_c"]
    b = _batch([fix["levels"][k]], 3, [0, 0, 0], wp=dict(zip(("collection_radius", "out_of_order_scale", "progress_scale", "progress_spacing"), par)))
    tr = Trace(b)
    for a in z["aact%d" % k]:
        tr.step(np.full(3, a, dtype=np.uint8))
    rows, pos = tr.arrays()
    _check_twin(lib, [fix["levels"][k]], [0, 0, 0], rows, pos, wp=par)
    for e in range(3):
        assert np.array_equal(rows["reward"][:, e].view(np.uint32), z["crew%d" % k].astype(np.float32).view(np.uint32))
        assert np.array_equal(rows["bonus"][:, e].view(np.uint32), z["cwpb%d" % k].astype(np.float32).view(np.uint32))
        assert np.array_equal(rows["info"][:, e], z["cwpi%d" % k][:, [0, 2, 3]])
    assert (z["cwpi%d" % k][:, 0] >= 0).sum() > 20 and not np.array_equal(z["cwpb%d" % k], z["awpb%d" % k])
    b.set_waypoint_params(None)   # back to the defaults from the next step on: the twin from here with the default numbers
    b.reset()
    tr.restart()
    for a in z["aact%d" % k][:60]:
        tr.step(np.full(3, a, dtype=np.uint8))
    rows, pos = tr.arrays()
    seen = _check_twin(lib, [fix["levels"][k]], [0, 0, 0], rows, pos)
    assert seen[0] > 0
    b.close()


# ---- twin: levels the fixture never saw; one 64-step run shared by the tests below ------------------------------------------------
N_TWIN, STEPS_TWIN = 259, 64
# The action seed was chosen on the CPU: the oracle's "mul" variant (the step kernel's bit-exact twin) played these actions on these
# levels with resets at episode ends, and npp_reward_host_wp on its trajectories counted 784 in-sequence collections, 146
# out-of-sequence ones and 99 episode ends after a collection.
TWIN_SEED = 4243


@pytest.fixture(scope="module")
def twin(lib, fix):
    from tests.test_gpu_reward import _twin_levels

    levels = _twin_levels(lib, fix)
    assign = (np.arange(N_TWIN) * 7) % len(levels)   # levels mixed inside every wavefront
    acts = np.random.default_rng(TWIN_SEED).integers(0, 6, size=(STEPS_TWIN, N_TWIN)).astype(np.uint8)
    b = {"on": _batch(levels, N_TWIN, assign), "overlap": _batch(levels, N_TWIN, assign)}
    b["overlap"].set_obs_overlap(40)
    tr = {m: Trace(b[m]) for m in b}
    for t in range(STEPS_TWIN):
        for m in tr:
            tr[m].step(acts[t])
    out = {"levels": levels, "assign": assign}
    for m in tr:
        out[m] = tr[m].arrays()
        b[m].close()
    return out


def test_twin_device_equals_host_rule(lib, twin):
    rows, pos = twin["on"]
    seen = _check_twin(lib, twin["levels"], twin["assign"], rows, pos)
    print("twin: in-sequence collections, out-of-sequence collections, episode ends after a collection:", seen.tolist(), "levels", len(twin["levels"]))
    assert seen[0] > 0 and seen[1] > 0 and seen[2] > 0
    assert (rows["bonus"] > 0).any()


def test_obs_overlap_same_bits(twin):
    a, b = twin["on"], twin["overlap"]
    for k in a[0]:
        assert np.array_equal(a[0][k].view(np.uint8), b[0][k].view(np.uint8)), k
    assert np.array_equal(a[1], b[1])


# ---- off ------------------------------------------------------------------------------------------------------------------------
def test_waypoints_off_gives_the_rewards_of_reward_npz(lib, fix):
    """Mode "pbrs" with the waypoints never switched on, and switched on then off before the first step: the rewards of reward.npz's
    rollout "a" bit for bit, and neither waypoint output is written."""
    z = np.load(os.path.join(ROOT, "tests", "golden", "reward.npz"))
    ks = fix["ok"]
    n = len(ks)
    levels = [fix["levels"][k] for k in ks]
    never = _batch(levels, n, np.arange(n), waypoints=False)
    off = _batch(levels, n, np.arange(n), waypoints=True)
    off.set_reward_waypoints(False)
    traces = [Trace(never), Trace(off)]
    steps = 300
    for t in range(steps):
        act = np.array([z["aact%d" % k][t] for k in ks], dtype=np.uint8)
        for tr in traces:
            tr.step(act)
    for tr in traces:
        rows, pos = tr.arrays()
        for e, k in enumerate(ks):
            assert np.array_equal(pos[:, e], z["apos%d" % k]), fix["names"][k]
            assert np.array_equal(rows["reward"][:, e].view(np.uint32), z["arew%d" % k].astype(np.float32).view(np.uint32)), fix["names"][k]
        assert (rows["bonus"] == np.float32(SENTINEL_F)).all() and (rows["info"] == SENTINEL_I).all()
        tr.b.close()
    # the fixture's own rewards differ: the bonus is part of them
    assert any(not np.array_equal(z["arew%d" % k], fix["z"]["arew%d" % k]) for k in ks)


# ---- restarts -------------------------------------------------------------------------------------------------------------------
def test_reset_restore_and_assign_restart_the_waypoint_state(lib, fix):
    """A waypoint collected by an env is collectable again after npp_reset, after an archive restore into the env, and after
    npp_assign_levels; the host twin, restarted at that point, agrees from there on."""
    z = fix["z"]
    k = fix["names"].index("doors:replay:127")
    levels, n = [fix["levels"][k]], 4
    act = z["aact%d" % k]
    first = int(np.flatnonzero(z["awpi%d" % k][:, 0] >= 0)[0])
    idx = int(z["awpi%d" % k][first, 0])
    steps = first + 3
    assert not (z["aflags%d" % k][:steps] & 3).any()   # no episode end on the way
    b = _batch(levels, n, [0] * n)
    b.archive_create(4)
    envs = np.arange(n, dtype=np.int32)
    assert (b.archive_store(envs[:1], np.array([0], dtype=np.int32), status=True).cpu().numpy() == 0).all()   # the spawn state
    tr = Trace(b)
    for t in range(steps):
        tr.step(np.full(n, act[t], dtype=np.uint8))
    rows, pos = tr.arrays()
    _check_twin(lib, levels, [0] * n, rows, pos)
    assert (rows["info"][first, :, 0] == idx).all() and (rows["info"][-1, :, 2] >= 1).all()
    # env 0: from the archive; env 1: reset; env 2: its level assigned again; env 3 goes on
    b.archive_restore(envs[:1], np.array([0], dtype=np.int32))
    b.reset(mask=np.array([0, 1, 0, 0], dtype=np.uint8))
    b.assign_levels([0], [2])
    tr.restart()
    assert np.array_equal(tr.pos[0][:3], pos[0, :3]) and np.array_equal(tr.pos[0][3], pos[-1, 3])
    for t in range(steps):
        tr.step(np.full(n, act[t], dtype=np.uint8))
    rows2, pos2 = tr.arrays()
    _check_twin(lib, levels, [0] * n, rows2, pos2, envs=[0, 1, 2])
    assert (rows2["info"][first, :3, 0] == idx).all()   # the same waypoint, collected again
    assert (rows2["bonus"][first, :3] > 0).all()
    # the untouched env went on with its state: the twin over the whole run, and it does not collect the waypoint twice
    whole = {c: np.concatenate([rows[c][:, 3:], rows2[c][:, 3:]]) for c in rows}
    _check_twin(lib, levels, [0], whole, np.concatenate([pos[:, 3:], pos2[1:, 3:]]))
    assert (whole["info"][:, 0, 0] == idx).sum() == 1
    b.close()


# ---- refusals -------------------------------------------------------------------------------------------------------------------
def _serpentine(base):
    """a level whose only way from the spawn (top left) to the exit switch (bottom) runs through twelve corridors of 42 tiles: more
    than 1000 path nodes"""
    m = np.asarray(base, dtype=np.float64)[:1230].copy()
    m[1150:1230] = 0
    tiles = np.zeros((23, 42))
    for r in range(1, 23, 2):
        tiles[r, :] = 1
        tiles[r, 41 if (r // 2) % 2 == 0 else 0] = 0
    m[184:1150] = tiles.reshape(-1)
    m[1156] = 1
    # records of 5 values in units of 6 px: the ninja, the exit door (bottom corridor, left end), its switch 7 tiles to the right
    return np.concatenate([m, [0, 6, 6, 0, 0], [3, 6, 94, 0, 0], [4, 34, 94, 0, 0]])


def test_refusals(lib, fix):
    from nclone_amd import _native as nat
    from nclone_amd.engine import NppBatch

    k = fix["names"].index("c0:replay:0")
    levels = [fix["levels"][k]]
    b = _batch(levels, 4, [0] * 4, waypoints=False)
    b.set_reward_mode("sparse")
    with pytest.raises(nat.NppError) as e:   # without the mode
        b.set_reward_waypoints(True)
    assert e.value.code == nat.NPP_ERR_STATE
    assert lib.npp_set_reward_waypoints(b.h, 0, None) == nat.NPP_ERR_STATE
    b.set_reward_mode("pbrs")
    with pytest.raises(nat.NppError) as e:
        b.set_reward_waypoints(True, {"collection_radius": 24.5})
    assert e.value.code == nat.NPP_ERR_INVALID
    with pytest.raises(ValueError):
        b.set_reward_waypoints(True, {"no_such": 1.0})
    with pytest.raises(nat.NppError):
        b.level_waypoints(0)   # off
    b.set_reward_waypoints(True, {"collection_radius": 24.0})
    with pytest.raises(nat.NppError) as e:
        b.set_waypoint_params({"collection_radius": 30.0})
    assert e.value.code == nat.NPP_ERR_INVALID
    acts = _cuda(np.zeros((2, 4), dtype=np.uint8))
    out = nat.StepOut()
    assert lib.npp_step_many(b.h, C.c_void_p(acts.data_ptr()), 2, 4, C.byref(out)) == nat.NPP_ERR_STATE   # as with the mode alone
    with pytest.raises(ValueError):
        b.step_many(acts)
    # a repositioned entity: switching on is refused, and so is the launch
    b.set_reward_waypoints(False)
    b.set_entity_pos(3, 0, 400.0, 300.0)
    with pytest.raises(nat.NppError) as e:
        b.set_reward_waypoints(True)
    assert e.value.code == nat.NPP_ERR_UNSUPPORTED and "npp_set_entity_pos" in str(e.value)
    b.set_entity_pos(3, 0, float("nan"), float("nan"))
    b.set_reward_waypoints(True)
    b.step(acts[0])
    b.set_entity_pos(3, 0, 400.0, 300.0)
    with pytest.raises(nat.NppError) as e:
        b.step_reward()
    assert e.value.code == nat.NPP_ERR_UNSUPPORTED
    # switching the mode off switches the waypoints off; loading levels too
    b.set_entity_pos(3, 0, float("nan"), float("nan"))
    b.set_reward_mode("sparse")
    b.set_reward_mode("pbrs")
    with pytest.raises(nat.NppError):
        b.level_waypoints(0)
    b.close()
    # a level whose paths carry more than 512 waypoints: refused by name, the option stays off, the mode stays on
    long_level = _serpentine(levels[0])
    b = _batch([levels[0], long_level], 2, [0, 1], waypoints=False)
    with pytest.raises(nat.NppError) as e:
        b.set_reward_waypoints(True)
    assert e.value.code == nat.NPP_ERR_UNSUPPORTED and "level 1" in str(e.value) and "512" in str(e.value)
    bonus = torch.full((2,), SENTINEL_F, dtype=torch.float32, device="cuda")
    b.step(_cuda(np.zeros(2, dtype=np.uint8)))
    b.step_reward(wp_bonus_out=bonus)
    assert (bonus.cpu().numpy() == np.float32(SENTINEL_F)).all()
    b.set_reward_waypoints(True, {"progress_spacing": 30.0})   # thinner: it fits
    xy, ph = b.level_waypoints(1)
    assert 300 < len(xy) <= 512 and (ph == 1).any()
    b.step(_cuda(np.zeros(2, dtype=np.uint8)))
    b.step_reward(wp_bonus_out=bonus)
    assert (bonus.cpu().numpy() >= 0).all()   # written
    b.close()
    b = NppBatch(2)
    with pytest.raises(nat.NppError):
        b.set_reward_waypoints(True)
    b.close()


# ---- the host classes -----------------------------------------------------------------------------------------------------------
def _np(v):
    return v.cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)


@pytest.mark.parametrize("output", ["torch", "numpy"])
def test_vec_env_returns_the_kernel_reward_and_waypoint_info(lib, fix, output):
    from nclone_amd.vec_env import NppVecEnvironment

    z, ks, steps = fix["z"], fix["ok"], 120
    env = NppVecEnvironment([fix["levels"][k] for k in ks], len(ks), level_ids=np.arange(len(ks)), truncation_limit=100000, fast_reset=False,
                            reward_mode="pbrs", reward_waypoints=True, output=output)
    for e, k in enumerate(ks):
        xy, ph = env.level_waypoints(e)
        assert np.array_equal(xy, z["wp%d" % k][:, :2]) and np.array_equal(ph, z["wp%d" % k][:, 2].astype(np.uint8)), fix["names"][k]
    acts = np.stack([z["aact%d" % k][:steps] for k in ks])
    env.reset()
    rew, bonus, info3 = [], [], []
    for t in range(steps):
        _obs, r, _term, _trunc, info = env.step(acts[:, t])
        w = info["waypoints"]
        rew.append(_np(r).copy())
        bonus.append(_np(w["bonus"]).copy())
        info3.append(np.stack([_np(w["index"]), _np(w["next_expected"]), _np(w["collected"])], axis=1).copy())
    rew, bonus, info3 = np.stack(rew), np.stack(bonus), np.stack(info3)
    for e, k in enumerate(ks):
        assert np.array_equal(rew[:, e].view(np.uint32), z["arew%d" % k][:steps].astype(np.float32).view(np.uint32)), fix["names"][k]
        assert np.array_equal(bonus[:, e].view(np.uint32), z["awpb%d" % k][:steps].astype(np.float32).view(np.uint32)), fix["names"][k]
        assert np.array_equal(info3[:, e], z["awpi%d" % k][:steps][:, [0, 2, 3]]), fix["names"][k]
    env.set_waypoint_params(progress_scale=0.5)
    with pytest.raises(ValueError):
        env.set_waypoint_params(progress_spacing=24.0)
    # a sequence replay runs with the mode off and restarts the waypoint state on the state it ends in
    _obs, info = env.reset(options={"checkpoint": [2, 2, 2]})
    assert info["checkpoint_replay"]
    _obs, _r, _t, _tr, info = env.step(np.zeros(len(ks), dtype=np.uint8))
    assert (_np(info["waypoints"]["collected"]) <= 1).all() and (_np(info["waypoints"]["next_expected"]) >= 0).all()
    env.close()


def test_single_env_and_class_refusals(lib, fix):
    from nclone_amd.async_env import NppAsyncVecEnvironment
    from nclone_amd.vec_env import NppEnvironment, NppVecEnvironment

    z = fix["z"]
    k = fix["names"].index("c0:replay:0")
    env = NppEnvironment(map_data=fix["levels"][k], truncation_limit=100000, fast_reset=False, reward_mode="pbrs", reward_waypoints=True)
    env.reset()
    want, wb, wi = z["arew%d" % k].astype(np.float32), z["awpb%d" % k].astype(np.float32), z["awpi%d" % k]
    t = ends = 0
    while t < 60:
        _obs, rew, term, trunc, info = env.step(int(z["aact%d" % k][t]))
        w = info["waypoints"]
        assert np.float32(rew) == want[t] and np.float32(w["bonus"]) == wb[t], t
        assert [w["index"], w["next_expected"], w["collected"]] == wi[t, [0, 2, 3]].tolist(), t
        t += 1
        if term or trunc:
            ends += 1
            env.reset()
    assert ends >= 2 and (wi[:60, 0] >= 0).sum() >= 2   # without auto-reset the caller's reset() restarts the waypoint state
    assert len(env.level_waypoints(0)[0]) == len(z["wp%d" % k])
    env.close()
    with pytest.raises(ValueError):
        NppVecEnvironment([fix["levels"][k]], 2, reward_waypoints=True)   # needs reward_mode="pbrs"
    with pytest.raises(ValueError):
        NppAsyncVecEnvironment([fix["levels"][k]], 8, n_streams=2, reward_waypoints=True)
    env = NppVecEnvironment([fix["levels"][k]], 2, reward_mode="pbrs")
    with pytest.raises(RuntimeError):
        env.set_waypoint_params(progress_scale=1.0)
    with pytest.raises(RuntimeError):
        env.level_waypoints(0)
    env.close()
