#!/usr/bin/env python3
"""Golden fixture for the goal curriculum: `IntermediateGoalManager`
(gym_environment/reward_calculation/intermediate_goal_manager.py) produced by RUNNING the reference.

Companion of make_golden_reward.py (same rules: build container only, never imported by the package, the tests, bench.py or
smoke(); the output is pure data; nothing is restated).

    HOME=/tmp/orahome python3 tests/golden/make_golden_goal.py      # -> goal.npz

How the reference is run: the env's call sequence (npp_environment.py:874-975) re-enacted call by call on the seven levels of
reward.npz: `store_original_positions(exit_switch_position(), exit_door_position())`, a LevelData from the freshly loaded map, a
graph from `GraphBuilder.build_graph(level_data, ninja_pos=int(spawn))`, `build_paths_for_level(graph, level_data, spawn)`.  The
stage is then set through `state.unified_stage` (what `set_curriculum_stage` ends in) and the two getters are read for every
stage.  For the rollouts the real `apply_to_simulator` moves the entities of a live `NPlayHeadless`.

Per level k and interval tag q ("a" = 100.0, the default; "b" = 48.0):
  m<k>                 map_data
  orig<k>              f64[2, 2] original exit switch / exit door position
  path0_<k>, path1_<k> i32[n, 2] the manager's node paths spawn -> switch, switch -> exit (interval independent)
  {q}dist<k>           f64[3] spawn -> switch, switch -> exit, combined
  {q}stages<k>         i32[1] num_stages (0: the level has no paths, both getters return the original positions)
  {q}pos<k>            f64[max(num_stages, 1), 4] switch x, y, door x, y per stage (row 0 of a level without stages: the getters'
                       answer at stage 0)
Rollouts at interval 100.0, r = 0.. over ROLLOUTS (level tag, stage):
  roll_level, roll_stage   i32[n]
  rt<r> f64[T, 4], rd<r> u8[T, 20]   per tick over three episodes: ninja x, y, xspeed, yspeed and make_golden.disc_row
  rin<r> u8[T]             the input byte of every tick (jump | right << 1 | left << 2): the level's replay, then random bytes
  rep<r> i32[3]            ticks of each episode.  Episode 1 follows the map load, episode 2 `Simulator.reset()`, episode 3
                           `fast_reset()`; apply_to_simulator is applied in front of each
  rcell<r> i32[2, 2]       old and new 24-px cell index (x * 25 + y) of switch and door
Observations on the same four variants, 200 random actions at frame skip 4 (see main()):
  oa<r> u8[200] actions; op<r> f64[201, 2] ninja position at each observation; os<r> u8 exit_switch_activated; oc<r> u8 1 where the
  features were recomputed; ot<r> u8[200] 1 where the step ended the episode; of<r> f32[201, 38] reachability_features;
  od<r> i32[201, 2] toggle mines, deadly ones; odir<r> i8 path-mask direction (0 none 1 left 2 right 3 down); ograph<r> u8 from-graph bit
Reward "pbrs" on ROLLOUTS[0] and [1] (see main()): wconst<r> f64[3]; wact<r> u8[200]; wframes<r>, wflags<r>, wpos<r> f64[201, 2],
  wrew<r>, wcomp<r> f64[200, 4], wkind<r> as reward.npz's columns; v...<r> the same for the level's replay at one input per step; reward_params f64[6] as reward.npz's params
same_tick_wins             i32[1] wins in the tick that hit the switch (0: see main())
interval                   f64[2]; names: newline-separated level tags
"""
import logging
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LEVELS = [("reach.npz", "doors:replay:127"), ("reach.npz", "doors:replay:128"), ("reach.npz", "mines:replay:91"),
          ("reach.npz", "mines:replay:24"), ("reach.npz", "c0:replay:0"), ("reach2.npz", "c0:replay:20"),
          ("reach2.npz", "zoo:replay:16")]   # the seven levels of make_golden_reward.py
INTERVALS = (("a", 100.0), ("b", 48.0))
ROLLOUTS = [("mines:replay:24", 0), ("zoo:replay:16", 1), ("doors:replay:128", 0), ("c0:replay:0", 1)]
EXTRA_TICKS = 400   # random inputs behind the replay
EPISODE_CAP = 1500


def main():
    sys.path.insert(0, HERE)
    import make_golden_reach as mgr

    mgr.prepare()
    import nclone  # noqa: F401  (the prepared copy: make_golden puts the unprepared tree in front of the path)
    import make_golden as mg
    from nclone.nplay_headless import NPlayHeadless
    from nclone.graph.level_data import LevelData, extract_start_position_from_map_data
    from nclone.gym_environment.entity_extractor import EntityExtractor
    from nclone.graph.reachability.graph_builder import GraphBuilder
    from nclone.gym_environment.reward_calculation.intermediate_goal_manager import IntermediateGoalManager
    from nclone.gym_environment.reward_calculation.reward_config import GoalCurriculumConfig

    logging.disable(logging.CRITICAL)
    corpus = np.load(os.path.join(HERE, "corpus.npz"))
    golden = np.load(os.path.join(HERE, "reward.npz"))
    fixtures, out, tags = {}, {}, []
    COVER = {"switch_cell_changed": 0, "switch_cell_same": 0, "door_cell_changed": 0, "win": 0, "win_tick_after_switch": 0}
    SAME_TICK = [0]
    out["interval"] = np.array([v for _q, v in INTERVALS], dtype=np.float64)

    def load(k):
        fname, tag = LEVELS[k]
        if fname not in fixtures:
            z = np.load(os.path.join(HERE, fname))
            fixtures[fname] = (z, bytes(z["names"]).decode().split("\n"))
        z, names = fixtures[fname]
        m = z["m%d" % names.index(tag)]
        assert np.array_equal(np.asarray(m, dtype=np.float64), golden["m%d" % k])
        hp = NPlayHeadless(enable_rendering=False)
        hp.load_map_from_map_data(mgr.to_list(m))
        return m, hp

    def manager(hp, interval):
        mgm = IntermediateGoalManager(GoalCurriculumConfig(enabled=True, stage_distance_interval=interval))
        mgm.store_original_positions(hp.exit_switch_position(), hp.exit_door_position())
        tiles = np.zeros((23, 42), dtype=np.int32)
        for (x, y), t in hp.get_tile_data().items():
            if 0 <= x - 1 < 42 and 0 <= y - 1 < 23:
                tiles[y - 1, x - 1] = int(t)
        spawn = extract_start_position_from_map_data(hp.sim.map_data)
        ld = LevelData(start_position=spawn, tiles=tiles, entities=EntityExtractor(hp).extract_graph_entities(), switch_states={})
        gd = GraphBuilder().build_graph(ld, ninja_pos=(int(spawn[0]), int(spawn[1])))
        mgm.build_paths_for_level(gd, ld, spawn)
        return mgm

    for k, (_fname, tag) in enumerate(LEVELS):
        m, hp = load(k)
        out["m%d" % k] = np.asarray(m, dtype=np.float64)
        tags.append(tag)
        out["orig%d" % k] = np.array([hp.exit_switch_position(), hp.exit_door_position()], dtype=np.float64)
        for q, interval in INTERVALS:
            mgm = manager(hp, interval)
            p0 = np.array(mgm._spawn_to_switch_path, dtype=np.int32).reshape(-1, 2)
            p1 = np.array(mgm._switch_to_exit_path, dtype=np.int32).reshape(-1, 2)
            if q == "a":
                out["path0_%d" % k], out["path1_%d" % k] = p0, p1
            else:
                assert np.array_equal(p0, out["path0_%d" % k]) and np.array_equal(p1, out["path1_%d" % k])
            out["%sdist%d" % (q, k)] = np.array([mgm._spawn_to_switch_distance, mgm._switch_to_exit_distance, mgm._combined_distance],
                                                 dtype=np.float64)
            out["%sstages%d" % (q, k)] = np.array([mgm._num_stages], dtype=np.int32)
            rows = []
            for s in range(max(mgm._num_stages, 1)):
                mgm.state.unified_stage = s
                rows.append(list(mgm.get_curriculum_switch_position()) + list(mgm.get_curriculum_exit_position()))
            out["%spos%d" % (q, k)] = np.array(rows, dtype=np.float64).reshape(-1, 4)
            assert mgm._num_stages == 0 or (mgm.state.unified_stage == mgm._num_stages - 1 and mgm.is_at_final_stage())
            print(k, tag, "interval", interval, "stages", mgm._num_stages, "dist", out["%sdist%d" % (q, k)], "paths", len(p0), len(p1),
                  "last", rows[-1], "orig", out["orig%d" % k].ravel(), flush=True)

    # ---- per-tick physics on moved entities: the real apply_to_simulator on a live simulator
    out["roll_level"] = np.array([[t for _f, t in LEVELS].index(t) for t, _s in ROLLOUTS], dtype=np.int32)
    out["roll_stage"] = np.array([s for _t, s in ROLLOUTS], dtype=np.int32)
    for r, (tag, stage) in enumerate(ROLLOUTS):
        k = int(out["roll_level"][r])
        _m, hp = load(k)
        mgm = manager(hp, 100.0)
        assert stage < mgm._num_stages
        mgm.state.unified_stage = stage
        sw = mg.exit_switch(hp.sim)
        door = sw.parent
        cells = [[sw.cell[0] * 25 + sw.cell[1], 0], [door.cell[0] * 25 + door.cell[1], 0]]
        idx = int(tag.rsplit(":", 1)[1])
        rng = np.random.default_rng(61000 + r)
        rows, drows, ins, eps = [], [], [], []
        for ep in range(3):
            if ep == 1:
                hp.reset()
            elif ep == 2:
                hp.sim.fast_reset()
            mgm.apply_to_simulator(hp.sim)
            sw = mg.exit_switch(hp.sim)   # Simulator.reset() rebuilds the entities
            door = sw.parent
            assert (sw.xpos, sw.ypos) == tuple(out["apos%d" % k][stage, :2]) and (door.xpos, door.ypos) == tuple(out["apos%d" % k][stage, 2:])
            assert sw.active and door not in hp.sim.grid_entity[door.cell] and hp.sim.grid_entity[sw.cell][-1] is sw
            if ep == 0:
                cells[0][1] = sw.cell[0] * 25 + sw.cell[1]
                cells[1][1] = door.cell[0] * 25 + door.cell[1]
            stream = list(corpus["in%d" % idx]) if ep == 0 else []
            stream += list(rng.integers(0, 8, size=EXTRA_TICKS + EPISODE_CAP))
            n0 = len(rows)
            active = [True, True]   # the switch at the end of the two previous ticks
            for b in stream[:EPISODE_CAP]:
                h, j = mg.controls(int(b))
                hp.tick(h, j)
                nj = hp.sim.ninja
                ins.append(int(b))
                rows.append([nj.xpos, nj.ypos, nj.xspeed, nj.yspeed])
                drows.append(mg.disc_row(hp.sim))
                if nj.state == 8:
                    COVER["win"] += 1
                    # the ninja's entity list is gathered before its collision loop (physics.py:79-101) and the door joins its
                    # cell when the switch is hit: on these rollouts the earliest win comes one tick behind the switch and none
                    # falls into its tick (counted and stored, so a change of that shows)
                    SAME_TICK[0] += int(active[1])
                    COVER["win_tick_after_switch"] += int(active[0] and not active[1])
                active = [active[1], bool(sw.active)]
                if nj.state in (6, 7, 8):
                    break
            eps.append(len(rows) - n0)
        COVER["switch_cell_changed"] += cells[0][0] != cells[0][1]
        COVER["switch_cell_same"] += cells[0][0] == cells[0][1]
        COVER["door_cell_changed"] += cells[1][0] != cells[1][1]
        out["rt%d" % r] = np.array(rows, dtype=np.float64).reshape(-1, 4)
        out["rd%d" % r] = np.array(drows, dtype=np.uint8).reshape(-1, mg.N_DISC)
        out["rin%d" % r] = np.array(ins, dtype=np.uint8)
        out["rep%d" % r] = np.array(eps, dtype=np.int32)
        out["rcell%d" % r] = np.array(cells, dtype=np.int32)
        print("rollout", r, tag, "stage", stage, "episode ticks", eps, "final states", [int(drows[sum(eps[:i + 1]) - 1][0]) for i in range(3)],
              "cells", cells, flush=True)

    # ---- observations on the variants: reachability features and the path-mask direction along a rollout, the manager handed to the
    #      feature calculator as reachability_mixin.py:52-60 does, the env's call sequences as make_golden_reach.py and
    #      make_golden_pathmask.py re-enact them; the graph and the LevelData come from the simulator AFTER apply_to_simulator
    import types
    import make_golden_pathmask as mgp
    from nclone.graph.reachability.path_distance_calculator import CachedPathDistanceCalculator
    from nclone.graph.reachability.feature_computation import compute_reachability_features_from_graph

    detect = mgp.reference_detector()
    OBS = {"recomputed": 0, "episodes": 0, "switch_rows": 0, "directions": set()}
    for r, (tag, stage) in enumerate(ROLLOUTS):
        k = int(out["roll_level"][r])
        _m, hp = load(k)
        mgm = manager(hp, 100.0)
        mgm.state.unified_stage = stage
        mgm.apply_to_simulator(hp.sim)
        tiles = np.zeros((23, 42), dtype=np.int32)
        for (x, y), t in hp.get_tile_data().items():
            if 0 <= x - 1 < 42 and 0 <= y - 1 < 23:
                tiles[y - 1, x - 1] = int(t)
        ld = LevelData(start_position=extract_start_position_from_map_data(hp.sim.map_data), tiles=tiles,
                       entities=EntityExtractor(hp).extract_graph_entities(), switch_states={})
        assert tuple(hp.exit_switch_position()) == tuple(out["apos%d" % k][stage, :2])
        p0 = hp.ninja_position()
        gd = GraphBuilder().build_graph(ld, ninja_pos=(int(p0[0]), int(p0[1])))
        pc = CachedPathDistanceCalculator(max_cache_size=200, use_astar=True, goal_curriculum_manager=mgm)
        pc.build_level_cache(ld, gd["adjacency"], gd.get("base_adjacency"), gd)
        pcd = CachedPathDistanceCalculator(max_cache_size=200, use_astar=True, goal_curriculum_manager=mgm)   # the reward side's, read by the detector
        pcd.build_level_cache(ld, gd["adjacency"], gd.get("base_adjacency"), gd)
        env = types.SimpleNamespace(
            reward_calculator=types.SimpleNamespace(pbrs_calculator=types.SimpleNamespace(path_calculator=pcd)),
            nplay_headless=hp, current_graph_data=gd, _spatial_hash=None, _subcell_lookup=None, _deterministic_mask_applied_count=0)
        state = {"key": None, "f": None}
        P, S, C, T, F, D, DIR, GR = [], [], [], [], [], [], [], []

        def observe():
            pos = hp.ninja_position()
            key = ((int(pos[0] // 24), int(pos[1] // 24)), hp.exit_switch_activated())
            rec = 0
            if key != state["key"] or state["f"] is None:
                pc.build_level_cache(ld, gd["adjacency"], gd.get("base_adjacency", gd["adjacency"]), gd)
                f, _sd, _ed = compute_reachability_features_from_graph(gd["adjacency"], gd, ld, pos, pc,
                                                                       goal_positions=hp.get_goal_positions_for_features())
                state["key"], state["f"] = key, f.copy()
                rec = 1
            c0 = env._deterministic_mask_applied_count
            d = detect(env)
            P.append([pos[0], pos[1]])
            S.append(int(hp.exit_switch_activated()))
            C.append(rec)
            F.append(state["f"].copy())
            m1, m21 = hp.get_mine_entities()
            D.append([len(m1) + len(m21), sum(int(e.state == 0) for e in m1) + sum(int(e.state == 0) for e in m21)])
            DIR.append(mgp.DIRS[d])
            GR.append(env._deterministic_mask_applied_count - c0)
            OBS["directions"].add(mgp.DIRS[d])

        observe()
        acts = np.random.default_rng(62000 + r).integers(0, 6, size=200).astype(np.uint8)
        for a in acts:
            pc.clear_step_cache()
            h, j = mgr.ACTIONS[a]
            term = 0
            for _ in range(4):
                hp.tick(h, j)
                if hp.sim.ninja.state in (6, 7, 8):
                    term = 1
                    break
            T.append(term)
            if term:
                hp.reset()
                mgm.apply_to_simulator(hp.sim)
                pc.clear_cache()   # _reset_reachability_state
            observe()
        out["oa%d" % r], out["op%d" % r], out["os%d" % r] = acts, np.array(P, dtype=np.float64), np.array(S, dtype=np.uint8)
        out["oc%d" % r], out["ot%d" % r], out["of%d" % r] = np.array(C, dtype=np.uint8), np.array(T, dtype=np.uint8), np.array(F, dtype=np.float32)
        out["od%d" % r], out["odir%d" % r], out["ograph%d" % r] = np.array(D, dtype=np.int32), np.array(DIR, dtype=np.int8), np.array(GR, dtype=np.uint8)
        OBS["recomputed"] += int(np.sum(C)); OBS["episodes"] += int(np.sum(T)); OBS["switch_rows"] += int(np.sum(S))
        print("observations", r, tag, "stage", stage, "recomputed", int(np.sum(C)), "episodes", int(np.sum(T)), "switch rows", int(np.sum(S)),
              "misses", pc.misses, "directions", np.bincount(np.array(DIR), minlength=4).tolist(), flush=True)
    print("observation coverage:", OBS)
    assert OBS["recomputed"] > 100 and OBS["episodes"] >= 4 and OBS["switch_rows"] >= 10 and len(OBS["directions"]) >= 3

    # ---- reward "pbrs" on two variants: RewardCalculator(RewardConfig(enable_path_waypoints=False), goal_curriculum_manager=mgr), the
    #      life cycle make_golden_reward.py re-enacts (a one-tick warm-up episode, then the recorded rollout), the manager handed to
    #      calculate_reward as base_environment.py:644 does, apply_to_simulator after every reset
    from nclone.gym_environment.reward_calculation.main_reward_calculator import RewardCalculator
    from nclone.gym_environment.reward_calculation.reward_config import RewardConfig

    REW = {"death": 0, "win": 0, "switch_live": 0, "pbrs_nonzero": 0}
    out["reward_rollouts"] = np.array([0, 1], dtype=np.int32)   # indices into ROLLOUTS
    for r in (0, 1):
        tag, stage = ROLLOUTS[r]
        k = int(out["roll_level"][r])
        _m, hp = load(k)
        mgm = manager(hp, 100.0)
        mgm.state.unified_stage = stage
        mgm.apply_to_simulator(hp.sim)
        tiles = np.zeros((23, 42), dtype=np.int32)
        for (x, y), t in hp.get_tile_data().items():
            if 0 <= x - 1 < 42 and 0 <= y - 1 < 23:
                tiles[y - 1, x - 1] = int(t)
        ld = LevelData(start_position=extract_start_position_from_map_data(hp.sim.map_data), tiles=tiles,
                       entities=EntityExtractor(hp).extract_graph_entities(), switch_states={})
        p0 = hp.ninja_position()
        gd = GraphBuilder().build_graph(ld, ninja_pos=(int(p0[0]), int(p0[1])))
        adj, badj = gd["adjacency"], gd.get("base_adjacency", gd["adjacency"])
        rc = RewardCalculator(RewardConfig(enable_path_waypoints=False), goal_curriculum_manager=mgm)
        pcr = rc.pbrs_calculator.path_calculator
        pcr.build_level_cache(ld, adj, badj, gd)
        pbrs = rc.pbrs_calculator
        state = {"key": None, "sw": None, "ex": None}

        def observe():
            p = hp.ninja_position()
            sw = bool(hp.exit_switch_activated())
            key = (int(p[0] // 24), int(p[1] // 24), sw)
            if key != state["key"]:
                pcr.build_level_cache(ld, adj, badj, gd)
                _f, a_, b_ = compute_reachability_features_from_graph(adj, gd, ld, p, pcr, goal_positions=hp.get_goal_positions_for_features())
                state["key"], state["sw"], state["ex"] = key, a_, b_
            s_, e_ = hp.exit_switch_position(), hp.exit_door_position()
            n = hp.sim.ninja
            return dict(player_x=p[0], player_y=p[1], player_xspeed=n.xspeed, player_yspeed=n.yspeed, switch_activated=sw,
                        switch_x=s_[0], switch_y=s_[1], exit_door_x=e_[0], exit_door_y=e_[1], player_dead=n.has_died(),
                        player_won=n.has_won(), level_data=ld, _adjacency_graph=adj, _graph_data=gd,
                        _cached_switch_distance=state["sw"], _cached_exit_distance=state["ex"])

        def restart():
            hp.reset()
            mgm.apply_to_simulator(hp.sim)
            pcr.clear_cache()
            rc.reset()
            state["key"] = None
            return observe()

        def rollout(ctrl, ticks, record):
            prev = restart()
            pos, flags, frames, rew, comp, kind = [[prev["player_x"], prev["player_y"]]], [], [], [], [], []
            for h, j in ctrl:
                n_ticks = 0
                for _ in range(ticks):
                    hp.tick(h, j)
                    n_ticks += 1
                    if hp.sim.ninja.state in (6, 7, 8):
                        break
                o = observe()
                m0 = pbrs._cache_misses
                rv = rc.calculate_reward(o, prev, frames_executed=n_ticks, curriculum_manager=mgm)
                c = rc.last_pbrs_components
                term = bool(c["is_terminal"])
                kd = 3 if term else (0 if pbrs._cache_misses > m0 else (2 if o.get("_pbrs_cache_hit") else 1))
                flags.append(int(o["player_won"]) | int(o["player_dead"]) << 1 | int(o["switch_activated"]) << 2)
                frames.append(n_ticks)
                rew.append(rv)
                comp.append([c["pbrs_reward"], c["milestone_reward"], c.get("completion_approach_bonus", 0.0), c["terminal_reward"] if term else 0.0])
                kind.append(kd)
                if record:
                    REW["death"] += int(o["player_dead"]); REW["win"] += int(o["player_won"])
                    REW["switch_live"] += int(o["switch_activated"] and not prev["switch_activated"] and not term)
                    REW["pbrs_nonzero"] += int(c["pbrs_reward"] != 0.0)
                prev = restart() if term else o
                pos.append([prev["player_x"], prev["player_y"]])
            return dict(frames=np.array(frames, dtype=np.uint16), flags=np.array(flags, dtype=np.uint8), pos=np.array(pos, dtype=np.float64),
                        rew=np.array(rew, dtype=np.float64), comp=np.array(comp, dtype=np.float64), kind=np.array(kind, dtype=np.uint8))

        rollout([(0, 0)], 1, False)   # warm-up episode: the level constants
        out["wconst%d" % r] = np.array([pbrs._cached_spawn_to_switch_distance, pbrs._cached_switch_to_exit_distance,
                                        pbrs._cached_combined_path_distance], dtype=np.float64)
        acts = np.random.default_rng(63000 + r).integers(0, 6, size=200)
        out["wact%d" % r] = acts.astype(np.uint8)
        for name, v in rollout([mgr.ACTIONS[a] for a in acts], 4, True).items():
            out["w%s%d" % (name, r)] = v
        idx = int(tag.rsplit(":", 1)[1])   # second rollout: the level's own replay, one input per step (it reaches the moved goals)
        for name, v in rollout([mg.controls(int(b)) for b in corpus["in%d" % idx]], 1, True).items():
            out["v%s%d" % (name, r)] = v
        print("reward", r, tag, "stage", stage, "const", out["wconst%d" % r], "episodes", int(((out["wflags%d" % r] & 3) != 0).sum()), flush=True)
    fresh = RewardConfig()
    out["reward_params"] = np.array([fresh.death_penalty, fresh.level_completion_reward, fresh.switch_activation_reward,
                                     fresh.time_penalty_per_step, fresh.pbrs_objective_weight, rc.pbrs_gamma], dtype=np.float64)
    print("reward coverage:", REW)
    assert REW["death"] >= 1 and REW["pbrs_nonzero"] >= 50 and REW["win"] >= 1 and REW["switch_live"] >= 1

    print("coverage:", COVER, "same-tick wins", SAME_TICK[0])
    assert SAME_TICK[0] == 0
    out["same_tick_wins"] = np.array(SAME_TICK, dtype=np.int32)
    for name, v in COVER.items():
        assert v >= 1, name
    out["names"] = np.frombuffer("\n".join(tags).encode(), dtype=np.uint8)
    p = os.path.join(HERE, "goal.npz")
    np.savez_compressed(p, **out)
    print("goal.npz", os.path.getsize(p))
    assert os.path.getsize(p) < 1_000_000


if __name__ == "__main__":
    main()
