"""GPU tests of reward mode "pbrs" (npp_set_reward_mode / npp_step_reward): the device kernel along the reference's own
rollouts of tests/golden/reward.npz and on levels the fixture never saw, against the host build of the same rule (npp_reward_host,
which tests/test_reward_host.py pins to the fixture bit for bit) -- reward and components as f32 bits, the position-cache branch as
an integer --, the mode off, observation overlap, the refusals, restores, and the host classes.

The fixture's scripted rollout "d" places the ninja by assignment and is checked on the host only."""
import ctypes as C
import os

import numpy as np
import pytest

from tests.test_reward_host import END_BITS, host_reward, level_constants

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = ("reward", "reward_components", "positions", "flags", "frames")
END_ALL = 11   # won, dead, truncated: the flags bits after which the step kernel auto-resets


@pytest.fixture(scope="module")
def lib():
    from nclone_amd import _native

    return _native.lib()


@pytest.fixture(scope="module")
def fix(lib):
    z = np.load(os.path.join(ROOT, "tests", "golden", "reward.npz"))
    names = bytes(z["names"]).decode().split("\n")
    ok = [k for k in range(len(names)) if not np.isinf(z["const%d" % k]).any()]   # (the reference raises on the seventh)
    assert len(ok) == 6
    return {"z": z, "names": names, "ok": ok, "levels": [z["m%d" % k] for k in range(len(names))]}


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _batch(levels, n, assign, pbrs=True, autoreset=True, params=None, outputs=("positions", "reward_components"), **kw):
    from nclone_amd.engine import NppBatch

    b = NppBatch(n, autoreset=autoreset, outputs=outputs, fast_reset=False, **kw)   # the fixture resets with NPlayHeadless.reset()
    b.load_levels(levels)
    b.assign_levels(assign)
    b.set_truncation_limit(100000)
    b.reset()
    b.observe()
    if pbrs:
        b.set_reward_mode("pbrs", params)
    return b


class Trace:
    """what the device produced per step, and the positions the host twin needs (row 0: the state before the first step)"""

    def __init__(self, b):
        self.b = b
        self.status = torch.zeros(b.n, dtype=torch.int32, device="cuda")
        self.pos = [b.to_host(("positions",))["positions"][:, :2].copy()]
        self.rows = {k: [] for k in OUT + ("status",)}

    def step(self, act, skip=4):
        self.b.step(_cuda(act), frame_skip=skip)
        self.b.step_reward(status_out=self.status)
        h = self.b.to_host(OUT)
        for k in OUT:
            self.rows[k].append(h[k].copy())
        self.rows["status"].append(self.status.cpu().numpy().copy())
        self.pos.append(h["positions"][:, :2].copy())

    def arrays(self):
        return {k: np.stack(v) for k, v in self.rows.items()}, np.stack(self.pos)

    def restart(self):
        """a reset / restore happened outside the step kernel: the twin starts again from here"""
        self.b.observe()   # (the block's positions are those of the last launch that wrote them)
        self.pos = [self.b.to_host(("positions",))["positions"][:, :2].copy()]
        self.rows = {k: [] for k in self.rows}


def _check_twin(lib, levels, assign, rows, pos, params=None, end_bits=END_ALL, envs=None):
    """device == npp_reward_host at the device's own positions, flags and frames: f32 bits of reward and components, the branch"""
    kinds = np.zeros(4, int)
    for e in (range(pos.shape[1]) if envs is None else envs):
        rc, rew, comp, kind = host_reward(lib, levels[assign[e]], pos[:, e], rows["flags"][:, e], rows["frames"][:, e].astype(np.uint16), params,
                                          end_bits=end_bits)
        assert rc == 0, e
        got, want = rows["reward"][:, e], rew.astype(np.float32)
        bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
        assert len(bad) == 0, (e, assign[e], bad[:5], got[bad[:5]], want[bad[:5]])
        assert np.array_equal(rows["reward_components"][:, e].view(np.uint32), comp.astype(np.float32).view(np.uint32)), e
        assert np.array_equal(rows["status"][:, e], kind), e
        kinds += np.bincount(kind, minlength=4)
    return kinds


def _follow(lib, fix, ks, n):
    """n envs, env e on level ks[e % len(ks)], along both recorded rollouts; every step of every env is compared"""
    z = fix["z"]
    lv = [ks[e % len(ks)] for e in range(n)]
    assign = np.arange(n) % len(ks)
    levels = [fix["levels"][k] for k in ks]
    b = _batch(levels, n, assign)
    checked = 0
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
        kinds = _check_twin(lib, levels, assign, rows, pos)
        assert kinds[0] > 0 and kinds[1] > 0 and kinds[3] > 0, kinds
        for e, k in enumerate(lv):   # hence the fixture: the device follows the recorded trajectory and returns the recorded reward
            m = len(z["%sact%d" % (phase, k)])
            assert np.array_equal(pos[:m + 1, e], z["%spos%d" % (phase, k)]), (phase, fix["names"][k])
            assert np.array_equal(rows["flags"][:m, e] & 7, z["%sflags%d" % (phase, k)]), (phase, fix["names"][k])
            assert np.array_equal(rows["frames"][:m, e], z["%sframes%d" % (phase, k)]), (phase, fix["names"][k])
            want = z["%srew%d" % (phase, k)].astype(np.float32)
            assert np.array_equal(rows["reward"][:m, e].view(np.uint32), want.view(np.uint32)), (phase, fix["names"][k])
            checked += m
    b.close()
    return checked


def test_rollouts_on_the_device_67_envs(lib, fix):
    """The six levels the mode accepts, mixed inside one wavefront, plus a three-lane tail; with in-kernel auto-reset (the random
    rollouts hold 46 episode ends)."""
    assert _follow(lib, fix, fix["ok"], 67) > 67 * 300


def test_rollouts_on_the_device_single_env(lib, fix):
    k = fix["names"].index("mines:replay:24")
    assert _follow(lib, fix, [k], 1) == 300 + len(fix["z"]["bact%d" % k])


def test_non_default_params(lib, fix):
    z, k = fix["z"], 0
    par = z["params_c"]
    b = _batch([fix["levels"][k]], 3, [0, 0, 0], params=dict(zip(("death_penalty", "level_completion_reward", "switch_activation_reward",
                                                                  "time_penalty_per_step", "pbrs_objective_weight", "pbrs_gamma"), par)))
    tr = Trace(b)
    for a in z["aact%d" % k][:150]:
        tr.step(np.full(3, a, dtype=np.uint8))
    rows, pos = tr.arrays()
    _check_twin(lib, [fix["levels"][k]], [0, 0, 0], rows, pos, params=par)
    assert np.array_equal(rows["reward"][:, 0].view(np.uint32), z["crew%d" % k][:150].astype(np.float32).view(np.uint32))
    b.set_reward_params(None)   # back to the defaults from the next step on
    b.step(_cuda(np.zeros(3, dtype=np.uint8)))
    b.step_reward()
    b.close()


# ---- twin: levels the fixture never saw; one 64-step run shared by the tests below ------------------------------------------------
N_TWIN, STEPS_TWIN = 259, 64


def _twin_levels(lib, fix):
    zz = np.load(os.path.join(ROOT, "tests", "golden", "zoo.npz"))
    r = np.load(os.path.join(ROOT, "tests", "golden", "rollouts.npz"))
    lv = [zz["rm%d" % k] for k in range(int(zz["n_rollouts"][0]))] + [r["m%d" % k] for k in range(len(bytes(r["names"]).decode().split("\n")))]
    seen = [np.asarray(m, dtype=np.float64) for m in fix["levels"]]
    lv = [m for m in lv if level_constants(lib, m)[0] == 0
          and not any(len(s) == len(m) and np.array_equal(s, np.asarray(m, dtype=np.float64)) for s in seen)]
    assert len(lv) >= 12, len(lv)
    return lv


@pytest.fixture(scope="module")
def twin(lib, fix):
    levels = _twin_levels(lib, fix)
    assign = (np.arange(N_TWIN) * 7) % len(levels)   # levels mixed inside every wavefront
    acts = np.random.default_rng(4243).integers(0, 6, size=(STEPS_TWIN, N_TWIN)).astype(np.uint8)
    b = {"on": _batch(levels, N_TWIN, assign), "overlap": _batch(levels, N_TWIN, assign),
         "never": _batch(levels, N_TWIN, assign, pbrs=False, outputs=("positions",)), "off": _batch(levels, N_TWIN, assign)}
    b["overlap"].set_obs_overlap(40)
    b["off"].set_reward_mode("sparse")   # heard of the feature, switched off again before the first step
    tr = {m: Trace(b[m]) for m in ("on", "overlap")}
    plain = {m: [] for m in ("never", "off")}
    for t in range(STEPS_TWIN):
        for m in tr:
            tr[m].step(acts[t])
        for m in plain:
            b[m].step(_cuda(acts[t]))
            plain[m].append({k: v.copy() for k, v in b[m].to_host(("reward", "flags", "frames", "game_state", "positions")).items()})
    out = {"levels": levels, "assign": assign, "plain": plain}
    for m in tr:
        out[m] = tr[m].arrays()
    for m in b:
        b[m].close()
    return out


def test_twin_device_equals_host_rule(lib, twin):
    rows, pos = twin["on"]
    kinds = _check_twin(lib, twin["levels"], twin["assign"], rows, pos)
    print("twin branches miss / hit / hit without next hop / none:", kinds.tolist(), "levels", len(twin["levels"]))
    assert kinds[0] > 1000 and kinds[1] > 1000 and kinds[3] > 0
    assert (rows["reward_components"][:, :, 0] != 0).any() and (rows["reward_components"][:, :, 3] != 0).any()


def test_mode_off_keeps_the_sparse_reward(twin):
    """The only check on old behaviour: with the mode off (never switched on, or switched off again) the reward plane holds the
    step kernel's sparse constants, and the pbrs batch's state planes are the plain batch's."""
    never, off = twin["plain"]["never"], twin["plain"]["off"]
    rows, pos = twin["on"]
    events = 0
    for t in range(STEPS_TWIN):
        for k in never[t]:
            assert np.array_equal(never[t][k].view(np.uint8), off[t][k].view(np.uint8)), (t, k)
        fl = never[t]["flags"]
        prev = never[t - 1]["flags"] if t else np.zeros_like(fl)
        just = ((fl & 4) != 0) & (((prev & 4) == 0) | ((prev & END_ALL) != 0))
        want = 20.0 * ((fl & 1) != 0) - 3.0 * ((fl & 2) != 0) + 10.0 * just
        assert np.array_equal(never[t]["reward"], want.astype(np.float32)), t
        events += int((want != 0).sum())
        assert np.array_equal(rows["flags"][t], fl) and np.array_equal(pos[t + 1], never[t]["positions"][:, :2]), t
    assert events > 0


def test_obs_overlap_same_bits(twin):
    a, b = twin["on"], twin["overlap"]
    for k in a[0]:
        assert np.array_equal(a[0][k].view(np.uint8), b[0][k].view(np.uint8)), k
    assert np.array_equal(a[1], b[1])


# ---- refusals, restores ---------------------------------------------------------------------------------------------------------
def test_refusals(lib, fix):
    from nclone_amd import _native as nat
    from nclone_amd.engine import NppBatch

    k = fix["ok"][0]
    b = _batch([fix["levels"][k]], 4, [0] * 4)
    acts = _cuda(np.zeros((2, 4), dtype=np.uint8))
    with pytest.raises(ValueError):
        b.step_many(acts)
    out = nat.StepOut()
    assert lib.npp_step_many(b.h, C.c_void_p(acts.data_ptr()), 2, 4, C.byref(out)) == 4   # NPP_ERR_STATE
    with pytest.raises(ValueError):
        b.step_reward()   # no step yet
    b.step(acts[0])
    b.step_reward()
    with pytest.raises(ValueError):
        b.step_reward()   # one call per step
    assert lib.npp_step_reward(b.h, C.c_void_p(b.reward.data_ptr()), None, None) == 4
    assert lib.npp_step_reward(b.h, None, None, None) == 1
    assert lib.npp_set_reward_mode(b.h, 2, None) == 1
    with pytest.raises(ValueError):
        b.set_reward_mode("dense")
    with pytest.raises(ValueError):
        b.set_reward_params({"no_such": 1.0})
    b.set_reward_mode("sparse")
    b.step_many(acts)   # fine again
    with pytest.raises(ValueError):
        b.step_reward()
    b.close()
    # a level on which the reference raises: the mode stays off
    bad = [i for i in range(len(fix["names"])) if i not in fix["ok"]][0]
    b = _batch([fix["levels"][k], fix["levels"][bad]], 2, [0, 1], pbrs=False)
    with pytest.raises(nat.NppError):
        b.set_reward_mode("pbrs")
    with pytest.raises(ValueError):
        b.step_reward()
    b.step(_cuda(np.zeros(2, dtype=np.uint8)))
    b.close()
    # before levels are loaded
    b = NppBatch(2)
    with pytest.raises(nat.NppError):
        b.set_reward_mode("pbrs")
    b.close()


def test_repositioned_entity_is_refused(lib, fix):
    """npp_set_entity_pos: while an exit switch / door is moved, the reward launch and switching the mode on are refused like
    npp_reachability (NPP_ERR_UNSUPPORTED, the mode staying off); once the position is cleared the reward is served again and
    equals the host twin."""
    from nclone_amd import _native as nat

    k = fix["names"].index("mines:replay:24")
    levels, n = [fix["levels"][k]], 5
    act = fix["z"]["aact%d" % k]
    b = _batch(levels, n, [0] * n)
    b.step(_cuda(np.full(n, act[0], dtype=np.uint8)))
    b.step_reward()
    b.set_entity_pos(3, 0, 400.0, 300.0)
    b.step(_cuda(np.full(n, act[1], dtype=np.uint8)))
    with pytest.raises(nat.NppError) as e:
        b.step_reward()
    assert e.value.code == nat.NPP_ERR_UNSUPPORTED and "npp_set_entity_pos" in str(e.value)
    b.set_reward_mode("sparse")
    with pytest.raises(nat.NppError) as e:   # switching on while the entity is moved: refused, and the mode stays off
        b.set_reward_mode("pbrs")
    assert e.value.code == nat.NPP_ERR_UNSUPPORTED and "npp_set_entity_pos" in str(e.value)
    b.step(_cuda(np.full(n, act[2], dtype=np.uint8)))
    with pytest.raises(ValueError):
        b.step_reward()
    assert lib.npp_step_reward(b.h, C.c_void_p(b.reward.data_ptr()), None, None) == 4   # NPP_ERR_STATE: the mode is off
    b.set_entity_pos(3, 0, float("nan"), float("nan"))
    b.reset()
    b.observe()
    b.set_reward_mode("pbrs")
    tr = Trace(b)
    for t in range(40):
        tr.step(np.full(n, act[t], dtype=np.uint8))
    rows, pos = tr.arrays()
    _check_twin(lib, levels, [0] * n, rows, pos)
    assert np.array_equal(pos[:, 3], fix["z"]["apos%d" % k][:41])   # the env whose switch had been moved plays the level as recorded
    assert np.array_equal(rows["reward"][:, 3].view(np.uint32), fix["z"]["arew%d" % k][:40].astype(np.float32).view(np.uint32))
    b.close()


def test_truncation_under_auto_reset(lib, fix):
    """The known deviation: a step that ends by truncation and is auto-reset carries time penalty + switch milestone only; the env's
    reward state restarts on the spawn state.  Device == host twin on the device's own flags (bit 3 included)."""
    k = fix["names"].index("mines:replay:24")
    levels, n = [fix["levels"][k]], 3
    par = fix["z"]["params_c"]
    b = _batch(levels, n, [0] * n, params=list(par))
    b.set_truncation_limit(40)
    b.reset()
    b.observe()
    tr = Trace(b)
    rng = np.random.default_rng(9)
    for t in range(36):
        tr.step(rng.integers(0, 6, size=n).astype(np.uint8))
    rows, pos = tr.arrays()
    _check_twin(lib, levels, [0] * n, rows, pos, params=par)
    trunc = (rows["flags"] & 8) != 0
    assert trunc.sum() >= 2 * n
    assert np.array_equal(rows["reward"][trunc], ((par[3] * rows["frames"][trunc].astype(np.float64)) * 0.1).astype(np.float32))
    assert not rows["reward_components"][trunc].any() and (rows["status"][trunc] == 3).all()
    b.close()


def test_restore_and_reset_restart_the_reward_state(lib, fix):
    """An archive restore, a snapshot restore and a reset put an env on another state: its reward state restarts there (first step:
    no shaping term, the path length and the milestones start again), which is what the host twin started at that state gives."""
    z = fix["z"]
    k = fix["names"].index("mines:replay:24")
    levels, n = [fix["levels"][k]], 5
    act = z["aact%d" % k]
    b = _batch(levels, n, [0] * n)
    b.archive_create(4)
    tr = Trace(b)
    for t in range(12):
        tr.step(np.full(n, act[t], dtype=np.uint8))
    envs = np.arange(n, dtype=np.int32)
    assert (b.archive_store(envs[:2], np.array([0, 1], dtype=np.int32), status=True).cpu().numpy() == 0).all()
    b.snapshot()
    for t in range(12, 30):
        tr.step(np.full(n, act[t], dtype=np.uint8))
    rows, pos = tr.arrays()
    _check_twin(lib, levels, [0] * n, rows, pos)
    # envs 0, 1: from the archive (no status asked for; env 2's entry is skipped); env 3: reset; env 4 goes on
    b.archive_restore(envs[:3], np.array([0, 1, -1], dtype=np.int32))
    b.reset(mask=np.array([0, 0, 0, 1, 0], dtype=np.uint8))
    before = pos[-1]
    tr.restart()
    assert np.array_equal(tr.pos[0][:2], pos[12, :2]) and np.array_equal(tr.pos[0][3], pos[0, 3]) and np.array_equal(tr.pos[0][[2, 4]], before[[2, 4]])
    for t in range(30, 60):
        tr.step(np.full(n, act[t], dtype=np.uint8))
    rows2, pos2 = tr.arrays()
    _check_twin(lib, levels, [0] * n, rows2, pos2, envs=[0, 1, 3])
    assert (rows2["reward_components"][0, [0, 1, 3], 0] == 0).all()   # the first step of a restarted env only initialises the potential
    # the untouched envs went on with their state: the twin over the whole run
    whole = {c: np.concatenate([rows[c], rows2[c]]) for c in rows}
    _check_twin(lib, levels, [0] * n, whole, np.concatenate([pos, pos2[1:]]), envs=[2, 4])
    b.restore()   # the snapshot: every env back at step 12
    tr.restart()
    assert np.array_equal(tr.pos[0], pos[12])
    for t in range(12, 24):
        tr.step(np.full(n, act[t], dtype=np.uint8))
    rows3, pos3 = tr.arrays()
    _check_twin(lib, levels, [0] * n, rows3, pos3)
    b.close()


# ---- the host classes -----------------------------------------------------------------------------------------------------------
def _np(v):
    return v.cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)


def _surface(fix, steps, **kw):
    from nclone_amd.vec_env import NppVecEnvironment

    ks = fix["ok"]
    env = NppVecEnvironment([fix["levels"][k] for k in ks], len(ks), level_ids=np.arange(len(ks)), truncation_limit=100000, fast_reset=False,
                            reward_mode="pbrs", **kw)
    acts = np.stack([fix["z"]["aact%d" % k][:steps] for k in ks])
    obs, _info = env.reset()
    pos = [np.stack([_np(obs["player_x"]), _np(obs["player_y"])], axis=1).copy()]
    rows = {c: [] for c in ("reward", "reward_components", "flags", "frames")}
    for t in range(steps):
        obs, rew, term, _trunc, info = env.step(acts[:, t])
        pos.append(np.stack([_np(obs["player_x"]), _np(obs["player_y"])], axis=1).copy())
        fl = _np(info["player_won"]).astype(np.uint8) | _np(info["player_dead"]).astype(np.uint8) << 1 | _np(info["switch_activated"]).astype(np.uint8) << 2
        assert np.array_equal(_np(term), (fl & 3) != 0)
        rows["flags"].append(fl)
        rows["frames"].append(_np(info["frames_executed"]).copy())
        rows["reward"].append(_np(rew).copy())
        assert _np(info["pbrs_components"]).shape == (len(ks), 6)
        rows["reward_components"].append(_np(info["pbrs_components"]).copy())
    return env, {c: np.stack(v) for c, v in rows.items()}, np.stack(pos)


@pytest.mark.parametrize("output", ["torch", "numpy"])
def test_vec_env_returns_the_kernel_reward(lib, fix, output):
    env, rows, pos = _surface(fix, 120, output=output)
    z = fix["z"]
    for e, k in enumerate(fix["ok"]):
        assert np.array_equal(pos[:, e], z["apos%d" % k][:121]), fix["names"][k]
        assert np.array_equal(rows["reward"][:, e].view(np.uint32), z["arew%d" % k][:120].astype(np.float32).view(np.uint32)), fix["names"][k]
    rows["status"] = None
    for e, k in enumerate(fix["ok"]):
        rc, rew, comp, _kind = host_reward(lib, fix["levels"][k], pos[:, e], rows["flags"][:, e], rows["frames"][:, e].astype(np.uint16), end_bits=END_ALL)
        assert rc == 0 and np.array_equal(rows["reward_components"][:, e].view(np.uint32), comp.astype(np.float32).view(np.uint32))
    env.set_reward_params(time_penalty_per_step=-0.01)
    _obs, rew, _t, _tr, info = env.step(np.zeros(len(fix["ok"]), dtype=np.uint8))
    assert _np(rew).shape == (len(fix["ok"]),)
    # a sequence replay runs with the mode off and restarts the reward state on the state it ends in
    _obs, info = env.reset(options={"checkpoint": [2, 2, 2]})
    assert info["checkpoint_replay"]
    _obs, rew, _t, _tr, info = env.step(np.zeros(len(fix["ok"]), dtype=np.uint8))
    assert (_np(info["pbrs_components"])[:, 0] == 0).all()   # first step after the restart: the potential is initialised only
    env.close()


def test_single_env_without_autoreset_and_class_refusals(lib, fix):
    from nclone_amd.async_env import NppAsyncVecEnvironment
    from nclone_amd.vec_env import NppEnvironment, NppVecEnvironment

    z = fix["z"]
    k = fix["names"].index("c0:replay:0")
    env = NppEnvironment(map_data=fix["levels"][k], truncation_limit=100000, fast_reset=False, reward_mode="pbrs")
    obs, _ = env.reset()
    t, rews, ends = 0, [], 0
    want = z["arew%d" % k].astype(np.float32)
    while t < 60:
        obs, rew, term, trunc, info = env.step(int(z["aact%d" % k][t]))
        assert info["pbrs_components"].shape == (6,) and info["pbrs_components"].dtype == np.float32
        assert np.float32(rew) == want[t], t
        t += 1
        if term or trunc:
            ends += 1
            obs, _ = env.reset()
    assert ends >= 2   # without auto-reset the caller's reset() restarts the reward state
    env.close()
    with pytest.raises(ValueError):
        NppAsyncVecEnvironment([fix["levels"][k]], 8, n_streams=2, reward_mode="pbrs")
    with pytest.raises(ValueError):
        NppVecEnvironment([fix["levels"][k]], 2, reward_mode="dense")
