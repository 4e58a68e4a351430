"""GPU tests of the minimal observation mode (npp_minimal_observation; the reference's observation_mode = MINIMAL,
gym_environment/npp_environment.py:2232-2270, compute_minimal_observation observation_processor.py:505-567).

1. against the reference (tests/golden/minimal.npz, make_golden_minimal.py): all levels in one batch, auto-reset on, four launch
   geometries.  Columns 0-19 and 36-39 bit-identical (copies of reachability values pinned bit for bit, or one correctly rounded
   f64 quotient of bit-exact state); columns 20-35 are copies of spatial_context entries, whose pinned tolerance in this project
   is 1.2e-7 (test_gpu_parity.py::test_spatial_context_matches_reference): the same bound, the worst difference printed.
2. device twin without a fixture: a full-mode batch (spatial_context + reachability) and a minimal-mode batch step the same
   actions; the minimal row is, bit for bit, the gather of the twin's own outputs and the numpy-f64 encodings of npp_dump_state.
3. the same bits with the observation overlap, after snapshot / restore, across level-pool draws, around npp_set_entity_pos, and
   with npp_reachability_ex before or after in the same observation.
4. the host classes: key set, shapes, dtypes, values, what is absent, the refusals.

Column 39 (launch_pad_buffer): the fixture holds -1 only (its generator's docstring says why), and no rollout here is known to
reach another value; tests 1 and 2 compare whatever occurs.  Its non-negative values are pinned on the CPU, on the function the
kernel runs (tests/test_minimal_obs_host.py::test_state_encodings_match_numpy_on_every_field_value)."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXACT = list(range(20)) + [36, 37, 38, 39]
MINES = list(range(20, 36))
MINE_TOL = 1.2e-7          # test_spatial_context_matches_reference's bound
MAX_HOR_SPEED = 3.333      # nclone/constants
REACH_COLS = [13, 14, 15, 16, 8, 9, 12, 24]
MINE_COLS = [64 + 6 * m + f for m in range(4) for f in (0, 1, 2, 5)]


@pytest.fixture(scope="module")
def minimal():
    z = np.load(os.path.join(ROOT, "tests", "golden", "minimal.npz"))
    names = bytes(z["names"]).decode().split("\n")
    n = len(names)
    return {"levels": [z["m%d" % k] for k in range(n)], "names": names, "acts": np.stack([z["a%d" % k] for k in range(n)]),
            "rows": np.stack([z["o%d" % k] for k in range(n)])}


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _compare_with_reference(got, ref, names, where, worst):
    bad = np.flatnonzero((got[:, EXACT] != ref[:, EXACT]).any(axis=1))
    assert len(bad) == 0, (where, [(names[i], [EXACT[c] for c in np.flatnonzero(got[i, EXACT] != ref[i, EXACT])]) for i in bad])
    d = float(np.abs(got[:, MINES] - ref[:, MINES]).max())
    worst[0] = max(worst[0], d)
    assert d <= MINE_TOL, (where, d)


@pytest.mark.parametrize("geometry", [(16, 4), (1, 1), (4, 4), (64, 4)])
def test_minimal_observation_matches_reference(minimal, geometry):
    from nclone_amd.engine import NppBatch

    names, acts, rows = minimal["names"], minimal["acts"], minimal["rows"]
    n = len(names)
    b = NppBatch(n, autoreset=True, outputs=("minimal_observation", "reach_status"), fast_reset=False)   # the fixture resets with NPlayHeadless.reset()
    assert "spatial_context" not in b.out.t and "reachability_features" not in b.out.t
    b.load_levels(minimal["levels"])
    b.set_launch_geometry(*geometry)
    b.assign_levels(np.arange(n))
    b.set_truncation_limit(100000)
    b.reset()
    b.observe()
    b.minimal_observation()
    worst = [0.0]

    def check(t):
        h = b.to_host(("minimal_observation", "reach_status"))
        assert not h["reach_status"].any(), (t, [names[i] for i in np.flatnonzero(h["reach_status"])])   # status OK on every level
        _compare_with_reference(h["minimal_observation"], rows[:, t], names, (geometry, t), worst)

    check(0)
    for t in range(acts.shape[1]):
        b.step(_cuda(acts[:, t]))
        b.minimal_observation()
        check(t + 1)
    b.close()
    print("minimal_observation %r: worst mine-column difference %.3g (bound %.3g), the other 24 columns exact" % (geometry, worst[0], MINE_TOL))


def _encode(f, di):
    """Columns 0-11 and 36-39 from npp_dump_state (f64 [N, 12], i32 [N, 32]) as the reference computes them: f64, one rounding."""
    n = len(f)
    o = np.zeros((n, 40), dtype=np.float32)
    o[:, 0] = f[:, 2] / MAX_HOR_SPEED
    o[:, 1] = f[:, 3] / MAX_HOR_SPEED
    o[np.arange(n), 2 + np.minimum(di[:, 0], 4)] = 1.0
    o[:, 7] = np.where(di[:, 1] != 0, 1.0, -1.0)
    o[:, 8] = np.where(di[:, 2] != 0, 1.0, -1.0)
    o[:, 9] = np.where(di[:, 2] != 0, di[:, 3] - 1.0, 0.0)
    o[:, 10] = f[:, 4]
    o[:, 11] = f[:, 5]
    for c, k, span in ((36, 4, 5.0), (37, 5, 5.0), (38, 6, 5.0), (39, 7, 4.0)):
        buf = di[:, k].astype(np.float64) - 1.0
        o[:, c] = np.where(buf >= 0, buf / span, -1.0)
    return o


def _gather(full_batch):
    """The minimal rows a full-mode batch implies: its own reachability_features / spatial_context + the state encodings."""
    f, di = full_batch.dump_state()
    h = full_batch.to_host(("spatial_context", "reachability_features"))
    o = _encode(f, di)
    o[:, 12:20] = h["reachability_features"][:, REACH_COLS]
    o[:, 20:36] = h["spatial_context"][:, MINE_COLS]
    return o, di


def _twin_levels():
    from nclone_amd.engine import reach_level_info

    z = np.load(os.path.join(ROOT, "tests", "golden", "zoo.npz"))
    r = np.load(os.path.join(ROOT, "tests", "golden", "rollouts.npz"))
    nz, nr = int(z["n_rollouts"][0]), len(bytes(r["names"]).decode().split("\n"))
    lv = [(z["rm%d" % k], z["ra%d" % k]) for k in range(nz)] + [(r["m%d" % k], r["a%d" % k]) for k in range(nr)]
    keep = [reach_level_info(m)["supported"] for m, _a in lv]   # (npp_reachability's domain: one exit switch)
    assert sum(keep[:nz]) >= 1 and sum(keep[nz:]) >= 20   # entity-zoo levels and plain ones both take part
    lv = [x for x, k in zip(lv, keep) if k]
    steps = min(len(a) for _m, a in lv)
    return [m for m, _a in lv], np.stack([a[:steps] for _m, a in lv])


def _pair(levels, n, autoreset=True, fast_reset=False, assign=None):
    from nclone_amd.engine import NppBatch

    out = []
    for outputs in (("spatial_context", "reachability_features", "mine_sdf_features", "reach_status"), ("minimal_observation", "reach_status")):
        b = NppBatch(n, autoreset=autoreset, outputs=outputs, fast_reset=fast_reset)
        b.load_levels(levels)
        b.assign_levels(np.arange(n) % len(levels) if assign is None else assign)
        b.set_truncation_limit(100000)
        b.reset()
        b.observe()
        out.append(b)
    return out


def _observe_pair(full, mini, where):
    full.reachability()
    mini.minimal_observation()
    want, di = _gather(full)
    got = mini.to_host(("minimal_observation",))["minimal_observation"]
    bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    assert len(bad) == 0, (where, bad[:8].tolist(), got[bad[0][0]], want[bad[0][0]])
    return di


@pytest.mark.parametrize("autoreset", [True, False])
def test_minimal_observation_equals_full_mode_twin(autoreset):
    """No fixture: every level of zoo.npz / rollouts.npz that npp_reachability serves.  Without auto-reset the dead and the
    celebrating ninja stay in the batch, so every state code (6, 7, 8 capped at one-hot index 4) is covered."""
    levels, acts = _twin_levels()
    n = len(levels)
    full, mini = _pair(levels, n, autoreset=autoreset)
    states = set(_observe_pair(full, mini, "reset")[:, 0].tolist())
    bufs = set()
    for t in range(acts.shape[1]):
        a = _cuda(acts[:, t])
        full.step(a)
        mini.step(a)
        di = _observe_pair(full, mini, t)
        states |= set(di[:, 0].tolist())
        bufs |= set((di[:, 7] - 1).tolist())
    print("twin (autoreset %s): %d levels, %d steps, state codes %s, launch pad buffer values %s" % (autoreset, n, acts.shape[1], sorted(states), sorted(bufs)))
    assert {0, 1, 3, 4} <= states
    if not autoreset:
        assert states & {6, 7, 8}
    full.close()
    mini.close()


def test_minimal_observation_overlap_snapshot_pool_and_call_order():
    """The same bits as the full-mode twin's gather with npp_set_obs_overlap at 50 %, after npp_snapshot / npp_restore, across
    level-pool draws, around npp_set_entity_pos (refused while an entity is moved, as npp_reachability is; served again once the
    override is cleared), and with npp_reachability_ex called before or after in the same observation."""
    from nclone_amd import _native as nat
    from nclone_amd.engine import NppBatch
    from nclone_amd.levels import door_levels, mine_levels

    levels = mine_levels()[0][:4] + door_levels()[0][:4]
    n = 512   # 32 reachability groups: a 50 % cut has whole groups on both sides
    rng = np.random.default_rng(11)
    assign = (np.arange(n) // 64) % len(levels)
    full, mini = _pair(levels, n, fast_reset=True, assign=assign)
    for b in (full, mini):
        b.set_step_variant(1)   # pinned: the overlap never splits a launch the autotuner is timing
    mini.set_obs_overlap(50)
    # the host's conditions for cutting the step launch in two parts (npp_capi.cpp step_impl): workgroups of whole 16-env
    # reachability groups and a decided step variant -- without them this leg would test the unsplit path
    g, wpb = mini.launch_geometry()
    assert (64 // g) * wpb % 16 == 0 and mini.step_variant() == (1, True)
    _observe_pair(full, mini, "reset")

    def step(where):
        a = _cuda(rng.integers(0, 6, size=n).astype(np.uint8))
        full.step(a)
        mini.step(a)
        _observe_pair(full, mini, where)

    for t in range(40):
        step(("overlap", t))
    mini.set_obs_overlap(0)
    # snapshot / restore: the rows after the restore are those at the snapshot, and the run goes on in step with the twin
    full.snapshot()
    mini.snapshot()
    at_snap = mini.to_host(("minimal_observation",))["minimal_observation"].copy()
    for t in range(10):
        step(("before restore", t))
    full.restore()
    mini.restore()
    full.observe()
    mini.observe()
    _observe_pair(full, mini, "restored")
    assert np.array_equal(mini.to_host(("minimal_observation",))["minimal_observation"].view(np.uint32), at_snap.view(np.uint32))
    for t in range(10):
        step(("after restore", t))
    # npp_reachability_ex in the same observation, after and before: both calls give the bits either gives alone
    both = NppBatch(n, autoreset=True, outputs=("minimal_observation", "reachability_features", "mine_sdf_features", "reach_status", "switch_states"),
                    fast_reset=True)
    both.load_levels(levels)
    both.assign_levels(assign)
    both.set_truncation_limit(100000)
    both.reset()
    both.observe()
    f2, m2 = _pair(levels, n, fast_reset=True, assign=assign)
    rng2 = np.random.default_rng(12)
    for t in range(30):
        if t % 2:
            both.reachability(with_switch_states=True)
            both.minimal_observation()
        else:
            both.minimal_observation()
            both.reachability(with_switch_states=True)
        f2.reachability()
        m2.minimal_observation()
        hb = both.to_host(("minimal_observation", "reachability_features", "mine_sdf_features"))
        hf = f2.to_host(("reachability_features", "mine_sdf_features"))
        hm = m2.to_host(("minimal_observation",))
        assert np.array_equal(hb["minimal_observation"].view(np.uint32), hm["minimal_observation"].view(np.uint32)), t
        assert np.array_equal(hb["reachability_features"].view(np.uint32), hf["reachability_features"].view(np.uint32)), t
        assert np.array_equal(hb["mine_sdf_features"].view(np.uint32), hf["mine_sdf_features"].view(np.uint32)), t
        a = _cuda(rng2.integers(0, 6, size=n).astype(np.uint8))
        for b in (both, f2, m2):
            b.step(a)
    # a re-allocated output block: the handle forgets where the rows were written (they may have lived in the old block), so the
    # call is refused until the next step / observe instead of reading through a stale pointer
    both.enable_outputs("work")
    with pytest.raises(nat.NppError) as e:
        both.minimal_observation()
    assert e.value.code == nat.NPP_ERR_STATE
    both.observe()
    both.minimal_observation()
    m2.minimal_observation()
    assert np.array_equal(both.to_host(("minimal_observation",))["minimal_observation"].view(np.uint32),
                          m2.to_host(("minimal_observation",))["minimal_observation"].view(np.uint32))
    for b in (both, f2, m2):
        b.close()
    # npp_set_entity_pos: refused like npp_reachability while the switch is moved, served again (same bits) once it is cleared
    for b in (full, mini):
        b.set_entity_pos(3, 0, 400.0, 300.0)
    with pytest.raises(nat.NppError) as e:
        mini.minimal_observation()
    assert e.value.code == nat.NPP_ERR_UNSUPPORTED and "npp_set_entity_pos" in str(e.value)
    for b in (full, mini):
        b.set_entity_pos(3, 0, float("nan"), float("nan"))
        b.reset()
        b.observe()
    _observe_pair(full, mini, "override cleared")
    step("after override")
    # level pool: both draw the same levels (same seed); short episodes so that many envs change level
    w = np.linspace(1.0, 2.0, len(levels))
    for b in (full, mini):
        b.set_truncation_limit(40)
        b.set_level_pool(w, seed=99)
    before = mini.env_levels().copy()
    changed = 0
    for t in range(40):
        step(("pool", t))
        now = mini.env_levels()
        assert np.array_equal(now, full.env_levels())
        changed += int((now != before).sum())
        before = now
    assert changed > n // 4
    full.close()
    mini.close()


def test_minimal_mode_of_the_host_classes(minimal):
    from nclone_amd import _native as nat
    from nclone_amd import spaces
    from nclone_amd.vec_env import NppEnvironment, NppVecEnvironment

    names, acts, rows = minimal["names"], minimal["acts"], minimal["rows"]
    n = len(names)
    space = spaces.observation_space(minimal=True)
    scalars = {"player_x", "player_y", "player_won", "player_dead", "death_cause", "switch_activated", "switch_x", "switch_y",
               "exit_door_x", "exit_door_y"}
    for output in ("torch", "numpy"):
        env = NppVecEnvironment(minimal["levels"], n, level_ids=np.arange(n), truncation_limit=100000, output=output, fast_reset=False,
                                observation_mode="minimal")
        assert set(env.observation_space.spaces.keys()) == set(space.spaces.keys()) == {"minimal_observation", "action_mask"}
        t = env.batch.out.t
        assert "minimal_observation" in t
        assert not {"reachability_features", "mine_sdf_features", "switch_states", "spatial_context"} & set(t)
        worst = [0.0]

        def check(obs, step):
            assert set(obs.keys()) == {"minimal_observation", "action_mask"} | scalars and "game_state" not in obs
            for k, box in space.spaces.items():
                v = obs[k].cpu().numpy() if output == "torch" else obs[k]
                assert v.shape == (n,) + tuple(box.shape) and v.dtype == box.dtype, k
            for k in scalars:
                assert tuple(obs[k].shape) == (n,), k
            got = obs["minimal_observation"].cpu().numpy() if output == "torch" else obs["minimal_observation"]
            _compare_with_reference(got, rows[:, step], names, (output, step), worst)

        obs, _info = env.reset()
        check(obs, 0)
        for s in range(120):
            obs, rew, term, trunc, info = env.step(acts[:, s])
            check(obs, s + 1)
            ended = (term | trunc).cpu().numpy() if output == "torch" else (term | trunc)
            won = obs["player_won"].cpu().numpy() if output == "torch" else obs["player_won"]
            dead = obs["player_dead"].cpu().numpy() if output == "torch" else obs["player_dead"]
            assert not (won | dead)[ended].any()   # an auto-reset env shows its spawn state
            assert info["terminal_observation"].shape == (n, 41)
        env.close()
    # the single environment
    one = NppEnvironment(map_data=minimal["levels"][3], truncation_limit=100000, fast_reset=False, observation_mode="minimal")
    assert set(one.observation_space.spaces.keys()) == {"minimal_observation", "action_mask"}
    obs, _info = one.reset()
    for s in range(40):
        assert set(obs.keys()) == {"minimal_observation", "action_mask"} | scalars
        assert obs["minimal_observation"].shape == (40,) and obs["minimal_observation"].dtype == np.float32
        assert obs["action_mask"].shape == (6,) and obs["action_mask"].dtype == np.int8
        assert isinstance(obs["player_won"], bool) and isinstance(obs["player_x"], float)
        _compare_with_reference(obs["minimal_observation"][None], rows[3:4, s], names[3:4], ("single", s), [0.0])
        obs, rew, term, trunc, info = one.step(int(acts[3, s]))
        if term or trunc:
            break
    one.close()
    # conflicting options and unknown modes
    lv = minimal["levels"][:1]
    for kw in ({"enable_visual_observations": True}, {"enable_visual_frame_stacking": True}, {"enable_state_stacking": True},
               {"enable_graph_observations": True}, {"enable_spatial_context": True}, {"enable_reachability": True},
               {"enable_switch_states": True}):
        with pytest.raises(ValueError, match=list(kw)[0]):
            NppVecEnvironment(lv, 4, observation_mode="minimal", **kw)
        with pytest.raises(ValueError, match=list(kw)[0]):
            NppEnvironment(map_data=lv[0], observation_mode="minimal", **kw)
    with pytest.raises(ValueError, match="observation_mode"):
        NppVecEnvironment(lv, 4, observation_mode="MINIMAL")
    # a level with several exit switches is refused with the reachability error
    from tests.test_gpu_reach import _two_exit_level

    from nclone_amd.levels import curriculum0_levels

    two = _two_exit_level(next(m for m in curriculum0_levels()[0] if int(m[1156]) == 1 and int(m[1235]) == 3 and int(m[1240]) == 4))
    env = NppVecEnvironment([lv[0], two], 8, level_ids=np.arange(8) % 2, truncation_limit=100000, observation_mode="minimal")
    with pytest.raises(nat.NppError) as e:
        env.reset()
    assert e.value.code == nat.NPP_ERR_UNSUPPORTED and "npp_reachability: level 1" in str(e.value)
    env.close()
