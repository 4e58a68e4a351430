"""GPU checks of the goal curriculum (include/npp_amd.h npp_set_goal_curriculum).

1. Physics on variant levels: every tick of tests/golden/goal.npz -- the reference simulator after its own apply_to_simulator, three
   episodes (map load, Simulator.reset, fast_reset) on four (level, stage) pairs -- in discrete state and fp64 positions, 67 envs with
   the variants mixed inside a wavefront.
2. The bookkeeping kernels against the Python restatement tests/goal_ref.py after EVERY step, twice with identical bits.
3. The level pool, npp_reset and npp_assign_levels land on the variant of the level's stage; the refusals; a level without stages.
"""
import numpy as np
import pytest

from tests import goal_ref as gr

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


def _batch(n, **kw):
    from nclone_amd.engine import NppBatch

    return NppBatch(n, **kw)


def _disc(i):
    return i[:, :20].clip(0, 255).astype(np.uint8)


def _levels(z):
    return [z["m%d" % k] for k in range(7)]


def _state(b):
    g = b.goal_views()
    torch.cuda.synchronize()
    return (g["level_words"].cpu().numpy().copy(), g["ring"].cpu().numpy().view(np.uint32).copy(), g["env_words"].cpu().numpy().copy())


def test_variant_physics_matches_the_reference(golden):
    z = golden.z("goal")
    rl, rs = [int(v) for v in z["roll_level"]], [int(v) for v in z["roll_stage"]]
    n, R = 67, len(rl)
    b = _batch(n, autoreset=False)
    b.load_levels(_levels(z))
    b.set_goal_curriculum(True, stage_distance_interval=100.0, auto_advance=False)
    g = b.goal_views()
    assert g["n_base"] == 7 and b.n_levels == 7 + sum(int(z["astages%d" % k][0]) for k in range(7))
    for k in range(7):   # the handle's stage table is the fixture's
        ns, dist, orig, pos = b.goal_stage_positions(k)
        assert ns == int(z["astages%d" % k][0]) and np.array_equal(pos.view(np.uint64), z["apos%d" % k].view(np.uint64)), k
        assert np.array_equal(dist.view(np.uint64), z["adist%d" % k].view(np.uint64)) and np.array_equal(orig.reshape(2, 2), z["orig%d" % k])
    for k, s in zip(rl, rs):
        b.goal_set_stage(s, level=k)
    b.reset()                                   # the pending stages take effect at an episode start
    base = np.array([rl[e % R] for e in range(n)], dtype=np.int32)   # the four variants mixed inside the wavefront; env 64.. beyond it
    b.assign_levels(base)                       # first creation on the variant: the state a map load leaves (episode 1 of the fixture)
    want_level = np.array([np.flatnonzero((g["base_of"] == rl[e % R]) & (g["stage_of"] == rs[e % R]))[0] for e in range(n)], dtype=np.int32)
    assert np.array_equal(b.env_levels(), want_level)
    start = [0] * R
    for ep in range(3):
        T = [int(z["rep%d" % r][ep]) for r in range(R)]
        tmax = max(T)
        inputs = np.zeros((tmax, n), dtype=np.uint8)
        for e in range(n):
            r = e % R
            inputs[: T[r], e] = z["rin%d" % r][start[r]: start[r] + T[r]]
        d_in = torch.from_numpy(inputs).cuda()
        for tick in range(tmax):
            b.tick(d_in[tick: tick + 1])
            f, di = b.dump_state()
            for r in range(R):
                if tick >= T[r]:
                    continue
                ref, dref = z["rt%d" % r][start[r] + tick], z["rd%d" % r][start[r] + tick]
                for e in range(r, n, R):
                    assert np.array_equal(f[e, :4], ref), (ep, r, tick, e, f[e, :4], ref)
                    assert np.array_equal(_disc(di[e: e + 1])[0], dref), (ep, r, tick, e)
        for r in range(R):
            start[r] += T[r]
        if ep < 2:
            b.reset(mode="full" if ep == 0 else "fast")
            assert np.array_equal(b.env_levels(), want_level)   # the same stage: nobody changes level
    # entity_positions reports the moved switch and door
    b.observe()
    ep_ = b.entity_pos.cpu().numpy()
    for e in range(n):
        sw_door = z["apos%d" % rl[e % R]][rs[e % R]]
        want = np.array([sw_door[0] / 1056.0, sw_door[1] / 600.0, sw_door[2] / 1056.0, sw_door[3] / 600.0], dtype=np.float32)
        assert np.allclose(ep_[e, 2:6], want, atol=1e-7), (e, ep_[e], want)


def test_variant_physics_one_env_alone(golden):
    """each of the four fixture variants in a batch of ONE env (a wavefront with one live group): the first episode, tick for tick"""
    z = golden.z("goal")
    for r, (k, s) in enumerate(zip(z["roll_level"], z["roll_stage"])):
        b = _batch(1, autoreset=False)
        b.load_levels(_levels(z))
        b.set_goal_curriculum(True, auto_advance=False)
        b.goal_set_stage(int(s), level=int(k))
        b.reset()
        b.assign_levels(np.array([k], dtype=np.int32))
        T = int(z["rep%d" % r][0])
        d_in = torch.from_numpy(np.ascontiguousarray(z["rin%d" % r][:T, None])).cuda()
        for tick in range(T):
            b.tick(d_in[tick: tick + 1])
            f, di = b.dump_state()
            assert np.array_equal(f[0, :4], z["rt%d" % r][tick]), (r, tick)
            assert np.array_equal(_disc(di)[0], z["rd%d" % r][tick]), (r, tick)


def test_archive_round_trip_on_a_variant(golden):
    """store on a variant level, play on, restore: the state comes back bit for bit; a slot of another stage's variant is refused by the
    archive's same-level rule (status 2), unchanged"""
    z = golden.z("goal")
    n = 8
    b = _batch(n, autoreset=False)
    b.load_levels(_levels(z))
    b.set_goal_curriculum(True, auto_advance=False)
    g = b.goal_views()
    b.assign_levels(np.full(n, 3, dtype=np.int32))          # mines:replay:24, stage 0
    b.archive_create(4)
    rng = np.random.default_rng(1)
    acts = torch.from_numpy(rng.integers(0, 8, size=(60, n)).astype(np.uint8)).cuda()
    b.tick(acts[:20])
    f0, i0 = b.dump_state()
    c0 = b.entity_checksum()
    assert (g["stage_of"][b.env_levels()] == 0).all()
    st = b.archive_store(np.array([0, 1], dtype=np.int32), np.array([0, 1], dtype=np.int32), status=True)
    assert st.cpu().numpy().tolist() == [0, 0]
    b.tick(acts[20:60])
    assert not np.array_equal(b.dump_state()[0][:2], f0[:2])
    st = b.archive_restore(np.array([0, 1, 2], dtype=np.int32), np.array([0, 1, 1], dtype=np.int32), status=True)
    assert st.cpu().numpy().tolist() == [0, 0, 0]
    f1, i1 = b.dump_state()
    c1 = b.entity_checksum()
    assert np.array_equal(f1[:2], f0[:2]) and np.array_equal(i1[:2], i0[:2]) and np.array_equal(c1[:2], c0[:2])
    assert np.array_equal(f1[2], f0[1]) and np.array_equal(c1[2], c0[1])          # one slot into another env of the same variant
    b.goal_set_stage(2, level=3)
    b.reset(np.array([0, 0, 0, 0, 0, 0, 0, 1], dtype=np.uint8))                   # env 7 moves to the stage-2 variant
    assert g["stage_of"][b.env_levels()].tolist() == [0] * 7 + [2]
    st = b.archive_restore(np.array([7], dtype=np.int32), np.array([0], dtype=np.int32), status=True)
    assert st.cpu().numpy().tolist() == [2]                                       # the record's level is another variant


def _on_variants(z, n, rollouts, outputs, load=tuple(range(7))):
    """a batch whose env e plays the fixture variant rollouts[e % len(rollouts)], reset as the fixture's rollouts start"""
    from nclone_amd.engine import NppBatch

    b = NppBatch(n, autoreset=True, outputs=outputs, fast_reset=False)   # the fixture resets with NPlayHeadless.reset()
    b.load_levels([z["m%d" % k] for k in load])   # (`load`: which fixture levels; reward mode "pbrs" refuses mines:replay:91 as ever)
    base = {r: list(load).index(int(z["roll_level"][r])) for r in rollouts}
    b.set_goal_curriculum(True, auto_advance=False)
    for r in rollouts:
        b.goal_set_stage(int(z["roll_stage"][r]), level=base[r])
    b.reset()
    b.assign_levels(np.array([base[rollouts[e % len(rollouts)]] for e in range(n)], dtype=np.int32))
    b.set_truncation_limit(100000)
    b.reset()
    b.observe()
    g = b.goal_views()
    assert np.array_equal(g["stage_of"][b.env_levels()], [z["roll_stage"][rollouts[e % len(rollouts)]] for e in range(n)])
    return b


def test_observations_on_variants_match_the_reference(golden):
    """reachability features, path-mask direction, entity_positions and switch_states along the fixture's rollouts on four variants,
    67 envs mixed inside a wavefront, through in-kernel auto-resets: equal to what the reference computed on the moved LevelData"""
    z = golden.z("goal")
    out = ("positions", "reachability_features", "reach_status", "path_direction", "switch_states")
    n, R = 67, 4
    b = _on_variants(z, n, list(range(R)), out)
    b.set_action_masking("soft")
    env_r = np.arange(n) % R

    def check(t):
        b.reachability()
        b.switch_states()
        b.path_action_mask()
        h = b.to_host(out + ("entity_pos",))
        for r in range(R):
            rows = np.flatnonzero(env_r == r)
            assert (h["positions"][rows, :2] == z["op%d" % r][t]).all(), (r, t)
            assert not h["reach_status"][rows].any(), (r, t)
            assert (h["reachability_features"][rows].view(np.uint32) == z["of%d" % r][t].view(np.uint32)).all(), (r, t)
            assert (h["path_direction"][rows] == z["odir%d" % r][t]).all(), (r, t)
            p = z["apos%d" % int(z["roll_level"][r])][int(z["roll_stage"][r])]
            want = np.array([p[0] / 1056.0, p[1] / 600.0, p[2] / 1056.0, p[3] / 600.0], dtype=np.float32)
            assert np.allclose(h["entity_pos"][rows, 2:6], want, atol=1e-7), (r, t)
            assert (h["switch_states"][rows] == h["switch_states"][rows[0]]).all()

    check(0)
    for t in range(200):
        acts = np.array([z["oa%d" % r][t] for r in env_r], dtype=np.uint8)
        b.step(torch.from_numpy(acts).cuda())
        check(t + 1)
    assert sum(int(z["ot%d" % r].sum()) for r in range(R)) >= 4   # episodes ended and restarted on the variant along the way


def test_reward_pbrs_on_variants_matches_the_reference(golden):
    """reward "pbrs" with its components on two variants: the f32 bits of the reference's rewards (RewardCalculator with the manager),
    along random actions at frame skip 4 and along the level's replay at one input per step (a switch and a win on a variant)"""
    z, corpus = golden.z("goal"), golden.z("corpus")
    names = golden.names("goal")
    to_action = {(0, 0): 0, (-1, 0): 1, (1, 0): 2, (0, 1): 3, (-1, 1): 4, (1, 1): 5}
    rollouts = [int(r) for r in z["reward_rollouts"]]
    for pre, fs in (("w", 4), ("v", 1)):
        n = 6
        b = _on_variants(z, n, rollouts, ("positions", "reward_components"), load=(0, 1, 3, 4, 5, 6))
        b.set_reward_mode("pbrs")
        acts = []
        for r in rollouts:
            if pre == "w":
                acts.append(z["wact%d" % r])
            else:
                idx = int(names[int(z["roll_level"][r])].rsplit(":", 1)[1])
                by = corpus["in%d" % idx]
                acts.append(np.array([to_action[((0 if (v & 6) == 6 else (-1 if v & 4 else (1 if v & 2 else 0))), int(v & 1))] for v in by], dtype=np.uint8))
        steps = [len(z["%srew%d" % (pre, r)]) for r in rollouts]
        assert all(len(a) >= s_ for a, s_ in zip(acts, steps))
        env_r = [rollouts[e % len(rollouts)] for e in range(n)]
        wins = 0
        for t in range(max(steps)):
            a = np.array([acts[rollouts.index(r)][min(t, len(acts[rollouts.index(r)]) - 1)] for r in env_r], dtype=np.uint8)
            b.step(torch.from_numpy(a).cuda(), frame_skip=fs)
            b.step_reward()
            h = b.to_host(("positions", "reward", "reward_components", "flags", "frames"))
            for e, r in enumerate(env_r):
                if t >= steps[rollouts.index(r)]:
                    continue
                assert np.array_equal(h["positions"][e, :2], z["%spos%d" % (pre, r)][t + 1]), (pre, r, t)
                assert h["flags"][e] & 3 == z["%sflags%d" % (pre, r)][t] & 3 and h["frames"][e] == z["%sframes%d" % (pre, r)][t], (pre, r, t)
                want = np.float32(z["%srew%d" % (pre, r)][t])
                assert h["reward"][e].view(np.uint32) == want.view(np.uint32), (pre, r, t, h["reward"][e], want)
                ref = z["%scomp%d" % (pre, r)][t].astype(np.float32)
                c = h["reward_components"][e]
                live = (h["flags"][e] & 3) == 0
                assert c[0] == ref[0] and c[3] == ref[2] and c[4] == ref[3] and (c[1] if live else c[2]) == ref[1], (pre, r, t, c, ref)
                wins += int(h["flags"][e] & 1)
        if pre == "v":
            assert wins >= 1
        b.close()


def _stages_run(z, seed):
    """67 envs on four levels, W = 4, threshold 0.5, 64 steps of random actions; wins forced by placing ninjas on switch and door"""
    n, window, steps = 67, 4, 64
    picks = [4, 0, 3, 2]   # c0:replay:0 (2 stages), doors:replay:127 (2), mines:replay:24 (7), mines:replay:91 (none)
    b = _batch(n, autoreset=True)
    b.load_levels([z["m%d" % k] for k in picks])
    b.set_goal_curriculum(True, stage_distance_interval=100.0, advancement_threshold=0.5, rolling_window=window)
    g = b.goal_views()
    num_stages = [int(z["astages%d" % k][0]) for k in picks]
    ref = gr.GoalRef(num_stages, n, window, gr.need_for(window, 0.5))
    assert g["need"] == ref.need == 2 and np.array_equal(g["base_of"], ref.base_of) and np.array_equal(g["stage_of"], ref.stage_of)
    base = (np.arange(n) % 4).astype(np.int32)
    b.assign_levels(base)
    level = b.env_levels().copy()
    assert np.array_equal(level, [ref.level_for(int(v)) for v in base])
    pos = [b.goal_stage_positions(k)[3] for k in range(4)]
    rng = np.random.default_rng(seed)
    history, trace = [], []
    episode_level = level.copy()
    for step in range(steps):
        if step == 40:
            b.goal_set_stage(1, level=2)   # mines:replay:24 has advanced beyond stage 1 by then or not: either way the stage is replaced
            ref.set_stage(1, 2)
        # forced wins: every third env (rotating) is put on its switch, or on its door once the switch is hit
        f, di = b.dump_state()
        rows = f[:, :4].copy()
        for e in range(step % 3, n, 3):
            bl, st = int(ref.base_of[level[e]]), int(ref.stage_of[level[e]])
            if st < 0:
                continue
            sw_active = di[e, 13] == 1
            p = pos[bl][st]
            rows[e] = [p[0], p[1], 0.0, 0.0] if sw_active else [p[2], p[3], 0.0, 0.0]
        b.set_ninja_state(rows)
        actions = torch.from_numpy(rng.integers(0, 6, size=n).astype(np.uint8)).cuda()
        b.step(actions)
        torch.cuda.synchronize()
        flags = b.flags.cpu().numpy().copy()
        ended = (flags & gr.END_BITS) != 0
        before = level.copy()
        ref.apply(flags, level)
        got = b.env_levels()
        lv, ring, env = _state(b)
        assert np.array_equal(got, level), (step, np.flatnonzero(got != level))
        assert np.array_equal(lv, ref.lv) and np.array_equal(ring, ref.ring) and np.array_equal(env, ref.env), step
        # an env changes level only where its episode ended, and then plays the variant of its level's stage
        assert np.array_equal(level[~ended], before[~ended])
        for e in np.flatnonzero(ended):
            assert level[e] == ref.level_for(int(before[e]))
        history.append(int(ended.sum()))
        trace.append((flags, got.copy(), lv, ring, env))
    return ref.events, history, trace


def test_stage_bookkeeping_equals_the_restatement_and_is_reproducible(golden):
    z = golden.z("goal")
    ev, history, trace = _stages_run(z, 7)
    assert ev["advance"] >= 1 and ev["wrap"] >= 1 and ev["stale"] >= 1 and ev["pending"] >= 1 and ev["pinned"] >= 1, ev
    assert max(history) >= 2   # several ends in one step
    ev2, _h, trace2 = _stages_run(z, 7)
    assert ev2 == ev
    for a, c in zip(trace, trace2):
        assert all(np.array_equal(x, y) for x, y in zip(a, c))


def test_pool_reset_and_assignment_land_on_the_current_variant(golden):
    from tests import level_pool_ref as pr

    z = golden.z("goal")
    n = 67
    b = _batch(n, autoreset=True)
    b.load_levels(_levels(z))
    b.set_goal_curriculum(True, auto_advance=False)
    g = b.goal_views()
    ref = gr.GoalRef([int(z["astages%d" % k][0]) for k in range(7)], n, 500, gr.need_for(500, 0.8), auto_advance=False)
    with pytest.raises(ValueError):
        b.set_level_pool(np.ones(b.n_levels))      # the weights are per base level
    w = np.array([1.0, 2.0, 1.0, 3.0, 0.0, 1.0, 2.0])
    b.set_level_pool(w, seed=11)
    b.goal_set_stage(2)                            # every level to stage 2, clamped to its last
    ref.set_stage(2)
    b.draw_levels()
    counts = np.zeros(n, dtype=np.uint32)
    drawn = pr.draw(w, 11, np.arange(n), counts)
    level = b.env_levels()
    lvw = g["level_words"].cpu().numpy()
    assert lvw[gr.STAGE].tolist() == [1, 1, 0, 2, 1, 1, 2] and (lvw[gr.PENDING] == -1).all()
    bases = g["base_of"][level]
    assert (bases != 4).all()                      # weight 0 is never drawn
    assert np.array_equal(bases, drawn)
    for e in range(n):   # base levels are mapped to the variant of the stage; the level without stages stays on its base level
        bl = int(bases[e])
        assert level[e] == (bl if lvw[gr.NUM_STAGES, bl] == 0 else lvw[gr.VARIANT0, bl] + lvw[gr.STAGE, bl])
    assert (level[bases == 2] == 2).all() and (bases == 2).any()
    # steps under the pool: an env that ends draws a base level and lands on its variant
    # the drawn base level is the pool model's, with the draw standing between the two goal launches: counts replayed through pr.draw
    rng = np.random.default_rng(3)
    model = pr.PoolModel(n, w, 11)
    model.draw(np.ones(n, dtype=bool))            # the draw_levels() above
    ends = 0
    for _ in range(60):
        b.step(torch.from_numpy(rng.integers(0, 6, size=n).astype(np.uint8)).cuda())
        torch.cuda.synchronize()
        ended = (b.flags.cpu().numpy() & gr.END_BITS) != 0
        idx, lv = model.draw(ended)
        bases[idx] = lv
        ends += len(idx)
        level = b.env_levels()
        assert np.array_equal(g["base_of"][level], bases)
    assert ends >= 5
    assert np.array_equal(g["stage_of"][level] >= 0, lvw[gr.NUM_STAGES][g["base_of"][level]] > 0)
    assert all(level[e] == lvw[gr.VARIANT0, g["base_of"][level[e]]] + lvw[gr.STAGE, g["base_of"][level[e]]] for e in range(n) if g["stage_of"][level[e]] >= 0)
    b.set_level_pool(None)
    # without auto-reset semantics: an explicit reset maps to the current variant
    b.goal_set_stage(0)
    before = b.env_levels()
    b.reset()
    after = b.env_levels()
    assert np.array_equal(g["base_of"][after], g["base_of"][before]) and (g["stage_of"][after] <= 0).all()
    # assign_levels takes base ids
    b.assign_levels(np.full(n, 3, dtype=np.int32))
    assert (b.env_levels() == lvw[gr.VARIANT0, 3]).all()
    from nclone_amd import _native as nat

    with pytest.raises(nat.NppError):
        b.assign_levels(np.full(n, 8, dtype=np.int32))   # a variant id is not a base id


def test_refusals_and_switching_off(golden):
    from nclone_amd import _native as nat

    z = golden.z("goal")
    n = 8
    b = _batch(n, autoreset=True)
    b.load_levels(_levels(z)[:2])
    b.set_goal_curriculum(True)
    acts = torch.zeros((2, n), dtype=torch.uint8).cuda()
    with pytest.raises(nat.NppError) as e:
        b.step_many(acts)
    assert e.value.code == nat.NPP_ERR_STATE and "goal curriculum" in str(e.value) and "npp_step_many" in str(e.value)
    with pytest.raises(nat.NppError) as e:
        nat.check(b.h, b.lib.npp_set_reward_waypoints(b.h, 1, None))
    assert e.value.code == nat.NPP_ERR_STATE and "goal curriculum" in str(e.value) and "npp_set_reward_waypoints" in str(e.value)
    inputs, offsets, levels = np.zeros(10, dtype=np.uint8), np.array([0, 10], dtype=np.int64), np.zeros(1, dtype=np.int32)
    with pytest.raises(nat.NppError) as e:
        nat.check(b.h, b.lib.npp_demo_create(b.h, inputs.ctypes.data, offsets.ctypes.data, levels.ctypes.data, 1, 1, 0, 1))
    assert e.value.code == nat.NPP_ERR_STATE and "goal curriculum" in str(e.value) and "npp_demo_create" in str(e.value)
    # graph observations: no fixture pins the graph rows of a variant level
    rows = torch.zeros((n, 38), dtype=torch.float32).cuda()
    with pytest.raises(nat.NppError) as e:
        nat.check(b.h, b.lib.npp_graph_observation(b.h, rows.data_ptr(), rows.data_ptr(), rows.data_ptr(), rows.data_ptr(), 0))
    assert e.value.code == nat.NPP_ERR_UNSUPPORTED and "goal curriculum" in str(e.value) and "npp_graph_observation" in str(e.value)
    # npp_archive_seed: the replays belong to the base levels
    b.archive_create(4)
    b.archive_cells_create(seed=1)
    with pytest.raises(nat.NppError) as e:
        nat.check(b.h, b.lib.npp_archive_seed(b.h, inputs.ctypes.data, offsets.ctypes.data, levels.ctypes.data, 1, 0, None, None))
    assert e.value.code == nat.NPP_ERR_STATE and "goal curriculum" in str(e.value) and "npp_archive_seed" in str(e.value)
    b.archive_create(0)
    with pytest.raises(ValueError):
        b.set_goal_curriculum(True, stage_distance_interval=0.0)
    with pytest.raises(ValueError):
        b.set_goal_curriculum(True, rolling_window=0)
    assert b.n_levels == 2 + 2 + 2
    b.set_goal_curriculum(False)                  # back to the base levels
    assert b.n_levels == 2 and (b.env_levels() < 2).all()
    with pytest.raises(ValueError):
        b.goal_views()
    b.step_many(acts)                             # served again


def test_host_classes(golden):
    """NppVecEnvironment(goal_curriculum=True): info["goal_curriculum"], set_curriculum_stage, the episode records, and the README's
    curriculum example extended by the goal curriculum; NppEnvironment passes the options through; the async class refuses."""
    from nclone_amd.async_env import NppAsyncVecEnvironment
    from nclone_amd.vec_env import NppEnvironment, NppVecEnvironment

    z = golden.z("goal")
    levels, n = _levels(z), 16
    env = NppVecEnvironment(levels, n, level_ids=np.arange(n) % 7, output="numpy", episode_stats=True, level_weights=np.ones(7), level_seed=5,
                            goal_curriculum=True, goal_curriculum_params=dict(rolling_window=4, advancement_threshold=0.5))
    env.reset(seed=1)
    st = env.goal_curriculum_state()
    assert st["num_stages"].tolist() == [2, 2, 0, 7, 2, 2, 5] and (st["stage"] == 0).all()
    assert np.array_equal(st["positions"][3], z["apos3"][0]) and np.array_equal(st["positions"][2], z["orig2"].ravel())
    rng = np.random.default_rng(0)
    for _ in range(30):
        _obs, _r, _term, _trunc, info = env.step(rng.integers(0, 6, size=n))
    gc = info["goal_curriculum"]
    assert set(gc) >= {"unified_stage", "num_stages", "stage_distance_interval", "curriculum_switch_pos", "curriculum_exit_pos",
                       "original_switch_pos", "original_exit_pos", "episode_count", "switch_activation_count", "completion_count", "at_final_stage"}
    assert gc["stage_distance_interval"] == 100.0 and (info["level_id"] < 7).all() and (info["level_id"] >= 0).all()
    for e in range(n):
        k = int(info["level_id"][e])
        assert gc["num_stages"][e] == st["num_stages"][k]
        want = z["apos%d" % k][gc["unified_stage"][e]] if st["num_stages"][k] else z["orig%d" % k].ravel()
        assert np.array_equal(np.concatenate([gc["curriculum_switch_pos"][e], gc["curriculum_exit_pos"][e]]), want)
        assert np.array_equal(np.concatenate([gc["original_switch_pos"][e], gc["original_exit_pos"][e]]), z["orig%d" % k].ravel())
    assert (gc["episode_count"] >= gc["switch_activation_count"]).all() and (gc["switch_activation_count"] >= gc["completion_count"]).all()
    ep = info["episode"]
    assert ((ep["level_id"] < 7) & (ep["stage"] >= -1)).all()
    # the README's example, extended: more of what is not yet won, and the long levels one stage further
    rate = env.episode_level_stats()["success_rate"]
    rate = rate.cpu().numpy() if hasattr(rate, "cpu") else np.asarray(rate)
    assert len(rate) == env._b.n_levels   # one row per (level, stage): per-stage outcomes for free
    env.set_curriculum_stage(3)                     # every level, clamped to its last stage
    env.reset()
    st = env.goal_curriculum_state()
    assert st["stage"].tolist() == [1, 1, 0, 3, 1, 1, 3]
    _obs, _r, _t, _tr, info = env.step(rng.integers(0, 6, size=n))
    assert all(info["goal_curriculum"]["unified_stage"][e] == st["stage"][int(info["level_id"][e])] for e in range(n))
    assert info["goal_curriculum"]["at_final_stage"].tolist() == [bool(st["num_stages"][k] and st["stage"][k] == st["num_stages"][k] - 1)
                                                                 for k in info["level_id"]]
    with pytest.raises(ValueError):
        NppVecEnvironment(levels, n, reward_mode="pbrs", reward_waypoints=True, goal_curriculum=True)
    with pytest.raises(ValueError, match="goal_curriculum"):
        NppVecEnvironment(levels, n, goal_curriculum=True, enable_graph_observations=True)
    full = NppVecEnvironment(levels[3:4], 4, output="numpy", goal_curriculum=True, enable_reachability=True, reward_mode="pbrs",
                             action_masking_mode="hard", enable_switch_states=True)   # served on the variants (pinned above)
    full.reset()
    obs4, rew4, _t4, _tr4, info4 = full.step(np.zeros(4, dtype=np.int64))
    assert obs4["reachability_features"].shape == (4, 38) and np.isfinite(rew4).all() and "path_direction" in info4
    mini = NppVecEnvironment(levels[3:4], 4, output="numpy", goal_curriculum=True, observation_mode="minimal")
    mini.reset()
    mini.step(np.zeros(4, dtype=np.int64))
    with pytest.raises(ValueError):
        NppAsyncVecEnvironment(levels, 8, n_streams=2, goal_curriculum=True)
    one = NppEnvironment(map_data=levels[3], goal_curriculum=True, goal_curriculum_params=dict(stage_distance_interval=48.0))
    one.reset()
    assert one.goal_curriculum_state()["num_stages"].tolist() == [14]
    one.set_curriculum_stage(5)
    one.reset()
    s1 = one.goal_curriculum_state()
    assert s1["stage"].tolist() == [5] and np.array_equal(s1["positions"][0], z["bpos3"][5])
    _o, _r, _te, _tr, info1 = one.step(0)
    # the single-env class never auto-resets, and the rule counts behind auto-resetting steps only: its counters stay 0 (documented)
    gc1 = info1["goal_curriculum"]
    assert gc1["unified_stage"] == 5 and gc1["num_stages"] == 14 and gc1["episode_count"] == 0 and gc1["at_final_stage"] is False
    assert gc1["curriculum_switch_pos"] == tuple(z["bpos3"][5][:2]) and gc1["original_exit_pos"] == tuple(z["orig3"][1])
