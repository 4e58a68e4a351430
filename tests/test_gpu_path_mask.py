"""GPU tests of path-direction action masking (npp_set_action_masking / npp_path_action_mask): the device kernel along
the reference's own rollouts of tests/golden/pathmask.npz (direction, hard mask and from-graph bit of every observation, the rows
after an auto-reset included), a twin against the host build of the same detector on levels the fixture never saw, the modes, the
host classes' observation paths, the counters and the refusals.  Every comparison is on integers and exact.

There is no hook that writes a ninja position into an env, so the fixture's off-trajectory probes are checked on the host only
(tests/test_path_mask_host.py); the twin below stands in for them on the device."""
import ctypes as C
import os

import numpy as np
import pytest

from tests.path_mask_ref import hard_mask_bits, mask_bits

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CORE = ("game_state", "entity_pos", "reward", "frames", "action_mask", "flags", "terminal_state", "positions")


@pytest.fixture(scope="module")
def fix():
    z = np.load(os.path.join(ROOT, "tests", "golden", "pathmask.npz"))
    names = bytes(z["names"]).decode().split("\n")
    return {"z": z, "names": names, "levels": [z["m%d" % k] for k in range(len(names))]}


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _batch(levels, n, assign, mode, outputs=("positions", "path_direction"), **kw):
    from nclone_amd.engine import NppBatch

    b = NppBatch(n, autoreset=True, outputs=outputs, fast_reset=False, **kw)   # the fixture resets with NPlayHeadless.reset()
    b.load_levels(levels)
    b.assign_levels(assign)
    b.set_truncation_limit(100000)
    if mode != "never":
        b.set_action_masking(mode)
    b.reset()
    b.observe()
    return b


def _expected_counters(graph, term):
    """The counters' definition on the host: observations since the last reset, those classified from the graph, latched when a step
    ended the episode (the returned row is then the first of the next episode)."""
    obs, app, last = 1, int(graph[0]), (0, 0)
    for t in range(len(term)):
        if term[t]:
            last, obs, app = (obs, app), 0, 0
        obs += 1
        app += int(graph[t + 1])
    return obs, app, last[0], last[1]


def _follow(fix, ks, n):
    """n envs, env e on level ks[e % len(ks)], along both recorded rollouts in hard mode; every returned row is compared."""
    z = fix["z"]
    lv = [ks[e % len(ks)] for e in range(n)]
    b = _batch([fix["levels"][k] for k in ks], n, np.arange(n) % len(ks), "hard")
    status = torch.zeros(n, dtype=torch.int32, device="cuda")
    checked = 0
    for phase, skip in (("a", 4), ("b", 1)):
        steps = max(len(z["%sact%d" % (phase, k)]) for k in ks)
        act = np.zeros((n, steps), dtype=np.uint8)
        valid = np.zeros((n, steps + 1), dtype=bool)
        want = {c: np.zeros((n, steps + 1) + ((2,) if c == "pos" else ()), dtype=np.float64 if c == "pos" else np.int64)
                for c in ("pos", "dir", "hard", "graph", "inert")}
        for e, k in enumerate(lv):
            a = z["%sact%d" % (phase, k)]
            act[e, :len(a)] = a
            valid[e, :len(a) + 1] = True
            for c in want:
                want[c][e, :len(a) + 1] = z["%s%s%d" % (phase, c, k)]
        if phase == "b":
            b.reset(mode="full")
            b.observe()

        def check(t):
            b.path_action_mask(status_out=status)
            h = b.to_host(("action_mask", "path_direction", "positions"))
            v = valid[:, t]
            assert np.array_equal(h["positions"][v, :2], want["pos"][v, t]), (phase, t)   # the device follows the recorded trajectory
            got = {"dir": h["path_direction"], "hard": mask_bits(h["action_mask"]), "graph": status.cpu().numpy()}
            for c, g in got.items():
                bad = np.flatnonzero((g != want[c][:, t]) & v)
                assert len(bad) == 0, (phase, t, c, bad[:6], g[bad[:6]], want[c][bad[:6], t], [fix["names"][lv[i]] for i in bad[:6]])
            return int(v.sum())

        checked += check(0)
        for t in range(steps):
            b.step(_cuda(act[:, t]), frame_skip=skip)
            checked += check(t + 1)
        if phase == "a":   # counters: against a host count over the same rollout, the latch at every auto-reset
            st = {k: v.cpu().numpy().astype(np.int64) for k, v in b.path_mask_stats().items()}
            for e, k in enumerate(lv):
                exp = _expected_counters(z["agraph%d" % k], z["aterm%d" % k])
                got = (st["observed"][e], st["applied"][e], st["last_observed"][e], st["last_applied"][e])
                assert got == exp, (fix["names"][k], got, exp)
    b.close()
    return checked


def test_rollouts_on_the_device_67_envs(fix):
    """One env per fixture level plus padding envs: a full 64-lane wavefront and a three-lane tail, the levels mixed inside one
    wavefront.  The fixture has 37 auto-resets in the random rollouts and one won episode per replay."""
    ks = list(range(len(fix["names"])))
    assert sum(int(fix["z"]["aterm%d" % k].sum()) for k in ks) >= 30
    assert _follow(fix, ks, 67) > 67 * 300


def test_rollouts_on_the_device_single_env(fix):
    k = fix["names"].index("doors:replay:127")
    assert _follow(fix, [k], 1) == 301 + len(fix["z"]["bact%d" % k]) + 1


# ---- twin: levels the fixture never saw; one 64-step run shared by the tests below ------------------------------------------------
N_TWIN, STEPS_TWIN = 259, 64


def _twin_levels(fix):
    from nclone_amd.engine import reach_level_info

    z = np.load(os.path.join(ROOT, "tests", "golden", "zoo.npz"))
    r = np.load(os.path.join(ROOT, "tests", "golden", "rollouts.npz"))
    lv = [z["rm%d" % k] for k in range(int(z["n_rollouts"][0]))] + [r["m%d" % k] for k in range(len(bytes(r["names"]).decode().split("\n")))]
    seen = [np.asarray(m, dtype=np.float64) for m in fix["levels"]]
    lv = [m for m in lv if reach_level_info(m)["supported"]
          and not any(len(s) == len(m) and np.array_equal(s, np.asarray(m, dtype=np.float64)) for s in seen)]
    assert len(lv) >= 20
    return lv


def _mode_at(t):
    """the switching batch: hard, soft, off, hard, ... eight observations each (observation t follows step t - 1)"""
    return ("hard", "soft", None, "hard")[(t // 8) % 4]


@pytest.fixture(scope="module")
def twin(fix):
    levels = _twin_levels(fix)
    assign = (np.arange(N_TWIN) * 7) % len(levels)   # levels mixed inside every wavefront
    acts = np.random.default_rng(4242).integers(0, 6, size=(STEPS_TWIN, N_TWIN)).astype(np.uint8)
    b = {m: _batch(levels, N_TWIN, assign, m) for m in ("hard", "soft")}
    b["never"] = _batch(levels, N_TWIN, assign, "never", outputs=("positions",))
    b["off"] = _batch(levels, N_TWIN, assign, "hard")
    b["off"].set_action_masking(None)   # heard of the feature, switched off again before the first observation
    b["switch"] = _batch(levels, N_TWIN, assign, _mode_at(0))
    status = torch.zeros(N_TWIN, dtype=torch.int32, device="cuda")
    rec = {m: [] for m in b}
    rec["state"], rec["status"] = [], []
    for t in range(STEPS_TWIN + 1):
        if t:
            a = _cuda(acts[t - 1])
            for m in b:
                b[m].step(a)
        b["switch"].set_action_masking(_mode_at(t))
        b["hard"].path_action_mask(status_out=status)
        b["soft"].path_action_mask()
        if _mode_at(t):
            b["switch"].path_action_mask()
        rec["status"].append(status.cpu().numpy().copy())
        rec["state"].append(b["never"].dump_state())
        for m in b:
            names = CORE if m in ("never", "off") else ("action_mask", "path_direction", "positions")
            rec[m].append({k: v.copy() for k, v in b[m].to_host(names).items()})
    for m in b:
        b[m].close()
    return {"levels": levels, "assign": assign, "rec": rec}


def test_twin_device_equals_host_detector(twin):
    """Direction, from-graph bit and hard mask of 259 envs x 65 observations equal npp_path_direction_host at the dumped positions
    plus the Python keep-masks applied to the mask of a batch that never heard of the feature."""
    from nclone_amd import _native as nat

    lib = nat.lib()
    rec, assign = twin["rec"], twin["assign"]
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    seen = np.zeros(4, int)
    for t in range(STEPS_TWIN + 1):
        f, di = rec["state"][t]
        pos = np.ascontiguousarray(f[:, :2])
        sw = np.ascontiguousarray((di[:, 13] != 1).astype(np.uint8))   # exit switch not active: activated (2 = the level has none)
        assert np.array_equal(pos, rec["hard"][t]["positions"][:, :2])
        want_d, want_g = np.zeros(N_TWIN, np.int8), np.zeros(N_TWIN, np.uint8)
        for l in np.unique(assign):
            e = np.flatnonzero(assign == l)
            m = np.ascontiguousarray(twin["levels"][l], dtype=np.float64)
            pe, se = np.ascontiguousarray(pos[e]), np.ascontiguousarray(sw[e])
            d, g = np.zeros(len(e), np.int8), np.zeros(len(e), np.uint8)
            assert lib.npp_path_direction_host(m.ctypes.data_as(C.POINTER(C.c_double)), m.size, p(pe), p(se), len(e), p(d), p(g), None) == 0
            want_d[e], want_g[e] = d, g
        assert np.array_equal(rec["hard"][t]["path_direction"], want_d), t
        assert np.array_equal(rec["status"][t], want_g), t
        inert = mask_bits(rec["never"][t]["action_mask"])
        assert np.array_equal(mask_bits(rec["hard"][t]["action_mask"]), hard_mask_bits(inert, want_d)), t
        seen += np.bincount(want_d, minlength=4)
    print("twin directions none / left / right / down:", seen.tolist())
    assert (seen > 0).all()


def test_modes_off_soft_and_switching(twin):
    rec = twin["rec"]
    for t in range(STEPS_TWIN + 1):
        for k in CORE:   # off: every output bit-identical to a batch that never heard of the feature
            assert np.array_equal(rec["off"][t][k].view(np.uint8), rec["never"][t][k].view(np.uint8)), (t, k)
        inert = rec["never"][t]["action_mask"]
        assert np.array_equal(rec["soft"][t]["action_mask"], inert), t                                  # soft: mask as off ...
        assert np.array_equal(rec["soft"][t]["path_direction"], rec["hard"][t]["path_direction"]), t   # ... direction as hard
        mode = _mode_at(t)   # a mode set between two steps holds at the next observation
        assert np.array_equal(rec["switch"][t]["action_mask"], rec["hard"][t]["action_mask"] if mode == "hard" else inert), (t, mode)
        if mode:
            assert np.array_equal(rec["switch"][t]["path_direction"], rec["hard"][t]["path_direction"]), (t, mode)
    assert any((rec["hard"][t]["action_mask"] != rec["never"][t]["action_mask"]).any() for t in range(STEPS_TWIN + 1))


# ---- the host classes ----------------------------------------------------------------------------------------------------------
SURF_STEPS = 60


def _np(v):
    return v.cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v)


def _surface_run(fix, steps=SURF_STEPS, store_at=None, **kw):
    """NppVecEnvironment on the fixture's levels along the recorded random rollout; returns per observation the mask bits, the
    direction and the info of the step."""
    from nclone_amd.vec_env import NppVecEnvironment

    n = len(fix["names"])
    env = NppVecEnvironment(fix["levels"], n, level_ids=np.arange(n), truncation_limit=100000, fast_reset=False,
                            action_masking_mode="hard", **kw)
    acts = np.stack([fix["z"]["aact%d" % k][:steps] for k in range(n)])
    obs, info = env.reset()
    rows = [(mask_bits(_np(obs["action_mask"])), _np(info["path_direction"]).copy(), None)]
    held = []
    for t in range(steps):
        prev = obs
        obs, _rew, term, trunc, info = env.step(acts[:, t])
        if kw.get("output") == "numpy":   # the previous observation's block stays valid while this one is staged
            held.append((mask_bits(prev["action_mask"]) == rows[-1][0]).all())
        rows.append((mask_bits(_np(obs["action_mask"])), _np(info["path_direction"]).copy(),
                     {k: _np(info[k]).copy() for k in ("deterministic_mask_applied_count", "deterministic_mask_rate")}
                     | {"done": _np(term | trunc).copy()}))
        if store_at is not None and t + 1 == store_at:
            assert (_np(env.archive_store(np.arange(n, dtype=np.int32))) == 0).all()
    return env, obs, rows, held


def _check_surface(fix, rows, where):
    z, n = fix["z"], len(fix["names"])
    for t, (bits, d, _info) in enumerate(rows):
        assert np.array_equal(bits, [z["ahard%d" % k][t] for k in range(n)]), (where, t)
        assert np.array_equal(d, [z["adir%d" % k][t] for k in range(n)]), (where, t)


@pytest.mark.parametrize("surface", ["plain", "minimal", "numpy", "stacked"])
def test_surfaces_agree_with_the_reference(fix, surface):
    kw = {"plain": {}, "minimal": {"observation_mode": "minimal"}, "numpy": {"output": "numpy"},
          "stacked": {"enable_state_stacking": True, "state_stack_size": 3}}[surface]
    env, obs, rows, held = _surface_run(fix, **kw)
    _check_surface(fix, rows, surface)
    z, n = fix["z"], len(fix["names"])
    assert tuple(obs["action_mask"].shape) == (n, 6)   # (with frame stacking the mask is not stacked)
    if surface == "numpy":
        assert len(held) == SURF_STEPS and all(held)
    # the info keys at episode end: the episode's from-graph count and its share of the episode's observations, from the fixture
    ends = 0
    for k in range(n):
        cnt = tot = 0
        for t in range(SURF_STEPS + 1):
            info = rows[t][2]
            if info is not None and z["aterm%d" % k][t - 1]:
                assert info["done"][k] and info["deterministic_mask_applied_count"][k] == cnt, (surface, k, t)
                assert info["deterministic_mask_rate"][k] == cnt / tot, (surface, k, t)
                cnt = tot = 0
                ends += 1
            elif info is not None:
                assert not info["done"][k] and info["deterministic_mask_applied_count"][k] == 0
            cnt += int(z["agraph%d" % k][t])
            tot += 1
    assert ends >= 3
    env.close()


def test_restart_from_an_archive_slot_shows_the_restored_direction(fix):
    n = len(fix["names"])
    env, _obs, rows, _held = _surface_run(fix, steps=40, store_at=20, checkpoint_slots=n)
    _check_surface(fix, rows, "archive")
    obs = env.restart(np.arange(n, dtype=np.int32))
    assert np.array_equal(mask_bits(_np(obs["action_mask"])), rows[20][0])
    assert np.array_equal(_np(env.batch.out.t["path_direction"]), rows[20][1])
    assert any(rows[20][1][k] != rows[40][1][k] or rows[20][0][k] != rows[40][0][k] for k in range(n))   # (the restart moved something)
    env.close()


def test_checkpoint_options_of_reset_return_the_filtered_mask(fix):
    """reset(options={"checkpoint": seq}) replays the sequence in one launch (no observation inside it) and
    reset(options={"checkpoint": {"slots": ...}}) restores archive slots: both return the mask and the direction the plain path
    returned at the same state, and the counters restart with that observation."""
    n, K = len(fix["names"]), 24
    env, _obs, rows, _held = _surface_run(fix, steps=40, store_at=K, checkpoint_slots=n)
    _check_surface(fix, rows, "plain path")
    seq = np.stack([fix["z"]["aact%d" % k][:K] for k in range(n)])
    for options in ({"checkpoint": seq}, {"checkpoint": {"action_sequence": seq}}, {"checkpoint": {"slots": np.arange(n, dtype=np.int32)}}):
        obs, info = env.reset(options=options)
        assert np.array_equal(mask_bits(_np(obs["action_mask"])), rows[K][0]), list(options["checkpoint"])[:1]
        assert np.array_equal(_np(info["path_direction"]), rows[K][1])
        st = {k: _np(v) for k, v in env.batch.path_mask_stats().items()}
        assert (st["observed"] == 1).all() and np.array_equal(st["applied"], [fix["z"]["agraph%d" % k][K] for k in range(n)])
        obs, _rew, _term, _trunc, info = env.step(np.array([fix["z"]["aact%d" % k][K] for k in range(n)], dtype=np.uint8))   # the mode is on again
        assert np.array_equal(mask_bits(_np(obs["action_mask"])), rows[K + 1][0])
        assert np.array_equal(_np(info["path_direction"]), rows[K + 1][1])
    assert (rows[K][0] != 63).any() and (rows[K][1] != 0).any()   # (the filter removed something at that state)
    env.close()


def test_single_environment_and_annealing(fix):
    from nclone_amd.vec_env import NppEnvironment

    z, k = fix["z"], fix["names"].index("doors:replay:127")
    one = NppEnvironment(map_data=fix["levels"][k], truncation_limit=100000, fast_reset=False, action_masking_mode="hard")
    obs, info = one.reset()
    assert isinstance(info["path_direction"], int) and info["path_direction"] == z["adir%d" % k][0]
    for t in range(12):
        assert mask_bits(obs["action_mask"]) == z["ahard%d" % k][t]
        obs, _rew, term, trunc, info = one.step(int(z["aact%d" % k][t]))
        if term or trunc:   # no auto-reset here: the terminal observation is the episode's last counted one
            assert info["deterministic_mask_applied_count"] >= 0 and 0.0 <= info["deterministic_mask_rate"] <= 1.0
            break
        assert info["path_direction"] == z["adir%d" % k][t + 1]
    one.set_action_masking_mode("soft")
    obs, _info = one.reset()
    assert mask_bits(obs["action_mask"]) == z["ainert%d" % k][0]
    one.close()


def _two_exit_level(base):
    """A map with two exit door / switch pairs (map_loader.py:108-123: exit doors first, their switches 5 * exit_count later)."""
    m = np.asarray(base, dtype=np.float64)
    assert int(m[1156]) == 1 and int(m[1235]) == 3 and int(m[1240]) == 4   # [1230:1235] is the ninja's record
    door, switch, rest = m[1235:1240], m[1240:1245], m[1245:]
    door2, switch2 = door.copy(), switch.copy()
    door2[1] += 8
    switch2[1] += 8
    out = np.concatenate([m[:1235], door, door2, switch, switch2, rest])
    out[1156] = 2
    return out


def test_refusals(fix):
    from nclone_amd import _native as nat
    from nclone_amd.async_env import NppAsyncVecEnvironment
    from nclone_amd.levels import curriculum0_levels
    from nclone_amd.vec_env import NppVecEnvironment

    base = next(m for m in curriculum0_levels()[0] if int(m[1156]) == 1 and int(m[1235]) == 3 and int(m[1240]) == 4)
    two = _two_exit_level(base)
    b = _batch([fix["levels"][0], two], 64, np.zeros(64, dtype=np.int32), "hard")   # even when no env plays the level
    before = b.to_host(("action_mask",))["action_mask"].copy()
    with pytest.raises(nat.NppError) as e:
        b.path_action_mask()
    assert e.value.code == nat.NPP_ERR_UNSUPPORTED and "level 1" in str(e.value)
    assert np.array_equal(b.to_host(("action_mask",))["action_mask"], before)   # the mask is left unfiltered
    with pytest.raises(ValueError, match="action masking"):
        b.step_many(torch.zeros((2, 64), dtype=torch.uint8, device="cuda"))
    b.set_action_masking(None)
    with pytest.raises(nat.NppError) as e:
        b.path_action_mask()
    assert e.value.code == nat.NPP_ERR_STATE
    b.step_many(torch.zeros((2, 64), dtype=torch.uint8, device="cuda"))
    b.close()
    env = NppVecEnvironment([fix["levels"][0], two], 8, level_ids=np.arange(8) % 2, truncation_limit=100000, action_masking_mode="hard")
    with pytest.raises(nat.NppError) as e:
        env.reset()
    assert e.value.code == nat.NPP_ERR_UNSUPPORTED and "npp_reachability: level 1" in str(e.value)
    env.close()
    with pytest.raises(ValueError, match="action masking"):
        NppAsyncVecEnvironment([fix["levels"][0]], 64, action_masking_mode="soft")
