#!/usr/bin/env python3
"""Golden fixture for reward mode "pbrs": the step reward `RewardCalculator.calculate_reward`
(gym_environment/reward_calculation/main_reward_calculator.py:225-904) returns, produced by RUNNING the reference.

Companion of make_golden_reach.py / make_golden_pathmask.py (same rules: build container only, never imported by the package, the
tests, bench.py or smoke(); the output is pure data).

    HOME=/tmp/orahome python3 tests/golden/make_golden_reward.py      # -> reward.npz

How the reference is run.  Nothing is restated:
  * the package, the level, the graph and the level cache as make_golden_pathmask.py builds them, the cache on the calculator's own
    `pbrs_calculator.path_calculator`, which is the calculator the feature code is handed too;
  * `RewardCalculator(RewardConfig(enable_path_waypoints=False))`, no curriculum manager, no momentum waypoints;
  * the env's life cycle around it, re-enacted call by call (base_environment.py:483-757, reachability_mixin.py:67-70, 150-222):
    per step the ticks (early stop on win / death), then the observation -- `compute_reachability_features_from_graph` ONLY when
    (x // 24, y // 24, switch) changed, its two raw distances kept as `_cached_switch_distance` / `_cached_exit_distance` -- then
    `calculate_reward(final_obs, initial_obs, frames_executed=ticks run)`; at an episode end Simulator.reset, the path calculator's
    `clear_cache()` (+ `build_level_cache` at the next feature computation, as the mixin does), `RewardCalculator.reset()`, the cache
    key dropped, and the observation of the reset state, which becomes the next step's `prev_obs`;
  * the per-level constants (`_compute_combined_path_distance`, pbrs_potentials.py:897-1178) are computed by the reference at the
    first potential of a level.  That call also leaves entries in the path calculator's per-episode dictionary, so the calculator's
    very first episode on a level differs from all later ones.  The fixture pins the later ones: a one-tick warm-up episode runs
    before the recorded rollouts;
  * non-default parameters: a subclass of RewardConfig that overrides the five properties, and `pbrs_gamma` on the calculator.

Rows.  Per level k rollouts "a" (300 random actions at frame skip 4), "b" (the level's own replay from corpus.npz, one action per
tick), for level 0 "c" (rollout "a"'s actions under the non-default parameters: act / frames / flags / pos are rollout "a"'s), and for level 3 "d" (scripted, see main()):
  m<k>              map_data f64;  const<k> f64[3] spawn -> switch, switch -> exit, combined; all +inf where the reference raises
                    ("Combined geometric path distance is infinite"): such a level has no rollouts
  {p}act<k>         u8[steps] action 0..5;  {p}frames<k> u16[steps] ticks executed
  {p}flags<k>       u8[steps] of the state the step ended in, before the reset: bit 0 won, bit 1 dead, bit 2 exit_switch_activated
  {p}pos<k>         f64[steps + 1, 2] position at the observation a vector env returns: row 0 after the first reset, after a terminal
                    step the row of the reset state
  {p}rew<k>         f64[steps] the reward
  {p}comp<k>        f64[steps, 4] last_pbrs_components: pbrs_reward, milestone_reward (the distance milestone on a live step, the
                    switch milestone on a terminal one), completion_approach_bonus, terminal_reward (0 on a live step)
  {p}kind<k>        u8[steps] 0 position-cache miss, 1 hit, 2 hit without next hop, 3 terminal step
params              f64[6] death_penalty, level_completion_reward, switch_activation_reward, time_penalty_per_step,
                    pbrs_objective_weight, pbrs_gamma of a fresh RewardConfig() / RewardCalculator;  params_c: those of rollout "c"
pot_*, app_*        PBRSPotentials.objective_distance_potential and _calculate_completion_approach_bonus called directly on grids
names               newline-separated level tags
With NPP_REWARD_DEBUG=<path> the generator also writes the calculators' internal state per step to <path> (not committed).
"""
import logging
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
STEPS = 300
LEVELS = [("reach.npz", "doors:replay:127"), ("reach.npz", "doors:replay:128"), ("reach.npz", "mines:replay:91"),
          ("reach.npz", "mines:replay:24"), ("reach.npz", "c0:replay:0"), ("reach2.npz", "c0:replay:20"),
          ("reach2.npz", "zoo:replay:16")]   # the seven levels of make_golden_pathmask.py
INPUT_TO_ACTION = {(0, 0): 0, (-1, 0): 1, (1, 0): 2, (0, 1): 3, (-1, 1): 4, (1, 1): 5}
PARAMS_C = (-35.0, 150.0, 60.0, -0.01, 25.0, 0.995)


def controls(b):
    j, r, l = b & 1, (b >> 1) & 1, (b >> 2) & 1
    return (0 if (l and r) else (-1 if l else (1 if r else 0))), j


def main():
    sys.path.insert(0, HERE)
    import make_golden_reach as mgr

    mgr.prepare()
    from nclone.nplay_headless import NPlayHeadless
    from nclone.graph.level_data import LevelData, extract_start_position_from_map_data
    from nclone.gym_environment.entity_extractor import EntityExtractor
    from nclone.graph.reachability.graph_builder import GraphBuilder
    from nclone.graph.reachability.feature_computation import compute_reachability_features_from_graph
    from nclone.gym_environment.reward_calculation.main_reward_calculator import RewardCalculator
    from nclone.gym_environment.reward_calculation.reward_config import RewardConfig
    from nclone.gym_environment.reward_calculation.pbrs_potentials import PBRSPotentials

    logging.disable(logging.CRITICAL)

    class ConfigC(RewardConfig):
        death_penalty = property(lambda self: PARAMS_C[0])
        level_completion_reward = property(lambda self: PARAMS_C[1])
        switch_activation_reward = property(lambda self: PARAMS_C[2])
        time_penalty_per_step = property(lambda self: PARAMS_C[3])
        pbrs_objective_weight = property(lambda self: PARAMS_C[4])

    corpus = np.load(os.path.join(HERE, "corpus.npz"))
    fixtures, out, dbg, tags = {}, {}, {}, []
    COVER = {k: 0 for k in ("miss", "hit", "hit_no_hop", "dist_milestone_switch", "dist_milestone_exit", "switch_live", "switch_death",
                            "death", "win", "win_efficiency", "episode_start", "approach", "first_step")}
    fresh = RewardCalculator(RewardConfig(enable_path_waypoints=False))
    out["params"] = np.array([fresh.config.death_penalty, fresh.config.level_completion_reward, fresh.config.switch_activation_reward,
                              fresh.config.time_penalty_per_step, fresh.config.pbrs_objective_weight, fresh.pbrs_gamma], dtype=np.float64)
    out["params_c"] = np.array(PARAMS_C, dtype=np.float64)
    out["cache_threshold_sq"] = np.array([fresh.pbrs_calculator._position_cache_threshold_sq], dtype=np.float64)

    for k, (fname, tag) in enumerate(LEVELS):
        if fname not in fixtures:
            z = np.load(os.path.join(HERE, fname))
            fixtures[fname] = (z, bytes(z["names"]).decode().split("\n"))
        z, names = fixtures[fname]
        m = z["m%d" % names.index(tag)]
        hp = NPlayHeadless(enable_rendering=False)
        hp.load_map_from_map_data(mgr.to_list(m))
        tiles = np.zeros((23, 42), dtype=np.int32)
        for (x, y), t in hp.get_tile_data().items():
            if 0 <= x - 1 < 42 and 0 <= y - 1 < 23:
                tiles[y - 1, x - 1] = int(t)
        ents = EntityExtractor(hp).extract_graph_entities()
        ld = LevelData(start_position=extract_start_position_from_map_data(hp.sim.map_data), tiles=tiles, entities=ents,
                       switch_states={}, curriculum_stage=None)
        p0 = hp.ninja_position()
        gd = GraphBuilder().build_graph(ld, ninja_pos=(int(p0[0]), int(p0[1])))
        adj, badj = gd["adjacency"], gd.get("base_adjacency", gd["adjacency"])

        def rollout(prefix, rc, ctrl, ticks, record=True, after_switch=None):
            cover = COVER if record else dict.fromkeys(COVER, 0)
            pc = rc.pbrs_calculator.path_calculator
            pbrs = rc.pbrs_calculator
            state = {"key": None, "sw": None, "ex": None}

            def observe():
                p = hp.ninja_position()
                sw = bool(hp.exit_switch_activated())
                key = (int(p[0] // 24), int(p[1] // 24), sw)
                if key != state["key"]:
                    pc.build_level_cache(ld, adj, badj, gd)
                    _f, a, b = compute_reachability_features_from_graph(adj, gd, ld, p, pc, goal_positions=hp.get_goal_positions_for_features())
                    state["key"], state["sw"], state["ex"] = key, a, b
                s, e = hp.exit_switch_position(), hp.exit_door_position()
                n = hp.sim.ninja
                return dict(player_x=p[0], player_y=p[1], player_xspeed=n.xspeed, player_yspeed=n.yspeed, switch_activated=sw,
                            switch_x=s[0], switch_y=s[1], exit_door_x=e[0], exit_door_y=e[1], player_dead=n.has_died(),
                            player_won=n.has_won(), level_data=ld, _adjacency_graph=adj, _graph_data=gd,
                            _cached_switch_distance=state["sw"], _cached_exit_distance=state["ex"])

            def restart():
                hp.reset()
                pc.clear_cache()   # _reset_reachability_state
                rc.reset()
                state["key"] = None
                return observe()

            prev = restart()
            pos, flags, frames, rew, comp, kind, D = [[prev["player_x"], prev["player_y"]]], [], [], [], [], [], []
            first = True
            queue, done = list(ctrl), []
            while queue:
                h, j = queue.pop(0)
                done.append((h, j))
                n_ticks = 0
                if h == "place":   # scripted: the ninja is put at j = (x, y) by assignment, no tick runs
                    hp.sim.ninja.xpos, hp.sim.ninja.ypos = j
                else:
                    for _ in range(ticks):
                        hp.tick(h, j)
                        n_ticks += 1
                        if hp.sim.ninja.state in (6, 7, 8):
                            break
                o = observe()
                if after_switch is not None and o["switch_activated"]:
                    queue, after_switch = [("place", q) for q in after_switch], None
                h0, m0 = pbrs._cache_hits, pbrs._cache_misses
                ms0 = (rc._last_milestone_distance_to_switch, rc._last_milestone_distance_to_exit)
                r = rc.calculate_reward(o, prev, frames_executed=n_ticks)
                c = rc.last_pbrs_components
                term = bool(c["is_terminal"])
                just = o["switch_activated"] and not prev["switch_activated"]
                if term:
                    kd = 3
                    cover["death" if o["player_dead"] else "win"] += 1
                    cover["win_efficiency"] += c.get("efficiency_bonus", 0.0) > 0.0
                    cover["switch_death"] += bool(just and o["player_dead"])
                else:
                    kd = 0 if pbrs._cache_misses > m0 else (2 if o.get("_pbrs_cache_hit") else 1)
                    assert (pbrs._cache_hits - h0) + (pbrs._cache_misses - m0) == 1
                    cover[("miss", "hit", "hit_no_hop")[kd]] += 1
                    cover["switch_live"] += bool(just)
                    cover["approach"] += c["completion_approach_bonus"] > 0.0
                    cover["first_step"] += first
                    if c["milestone_reward"] > 0.0:
                        cover["dist_milestone_exit" if o["switch_activated"] else "dist_milestone_switch"] += 1
                flags.append(int(o["player_won"]) | int(o["player_dead"]) << 1 | int(o["switch_activated"]) << 2)
                frames.append(n_ticks)
                rew.append(r)
                comp.append([c["pbrs_reward"], c["milestone_reward"], c.get("completion_approach_bonus", 0.0),
                             c["terminal_reward"] if term else 0.0])
                kind.append(kd)
                none = lambda v, d: d if v is None else v
                D.append([o["_cached_switch_distance"], o["_cached_exit_distance"], none(c.get("current_potential"), np.nan),
                          none(pbrs._cached_distance, np.nan), *none(pbrs._cached_start_node, (-1, -1)), *none(pbrs._cached_next_hop, (-1, -1)),
                          none(pc._last_geometric_distance, np.nan), *none(pc._last_start_node, (-1, -1)), *none(pc._last_next_hop, (-1, -1)),
                          none(c.get("distance_to_goal"), np.nan), rc.episode_path_length, none(rc.optimal_path_length, np.nan),
                          o["player_x"], o["player_y"]])
                first = False
                prev = o
                if term:
                    prev = restart()
                    first = True
                    cover["episode_start"] += 1
                pos.append([prev["player_x"], prev["player_y"]])
            if not record:
                return None
            traj = {"act": np.array([INPUT_TO_ACTION.get(c, 255) for c in done], dtype=np.uint8), "frames": np.array(frames, dtype=np.uint16),
                    "flags": np.array(flags, dtype=np.uint8), "pos": np.array(pos, dtype=np.float64)}
            for name, v in traj.items():
                if prefix == "c":   # the trajectory does not depend on the reward: rollout "a"'s arrays serve
                    assert np.array_equal(v, out["a%s%d" % (name, k)])
                else:
                    out["%s%s%d" % (prefix, name, k)] = v
            out["%srew%d" % (prefix, k)] = np.array(rew, dtype=np.float64)
            out["%scomp%d" % (prefix, k)] = np.array(comp, dtype=np.float64)
            out["%skind%d" % (prefix, k)] = np.array(kind, dtype=np.uint8)
            dbg["%sdbg%d" % (prefix, k)] = np.array(D, dtype=np.float64)
            return np.bincount(kind, minlength=4).tolist()

        rc = RewardCalculator(RewardConfig(enable_path_waypoints=False))
        rc.pbrs_calculator.path_calculator.build_level_cache(ld, adj, badj, gd)
        out["m%d" % k] = np.asarray(m, dtype=np.float64)
        tags.append(tag)
        try:
            rollout("w", rc, [(0, 0)], 1, record=False)   # warm-up episode: the level constants (see the module docstring)
        except RuntimeError as e:   # _compute_combined_path_distance raises: the reference cannot train on this level
            assert "Combined geometric path distance is infinite" in str(e), e
            out["const%d" % k] = np.full(3, np.inf)
            print(k, tag, "the reference raises:", str(e)[:110], flush=True)
            continue
        pb = rc.pbrs_calculator
        out["const%d" % k] = np.array([pb._cached_spawn_to_switch_distance, pb._cached_switch_to_exit_distance,
                                       pb._cached_combined_path_distance], dtype=np.float64)
        acts = np.random.default_rng(52000 + k).integers(0, 6, size=STEPS)   # make_golden_pathmask.py's actions: trajectories the device is known to follow
        ka = rollout("a", rc, [mgr.ACTIONS[a] for a in acts], 4)
        idx = int(tag.rsplit(":", 1)[1])
        assert np.array_equal(np.asarray(m, dtype=np.float64), corpus["m%d" % idx].astype(np.float64)), tag
        kb = rollout("b", rc, [controls(int(b)) for b in corpus["in%d" % idx]], 1)
        kc = None
        if k == 0:
            rc2 = RewardCalculator(ConfigC(enable_path_waypoints=False), pbrs_gamma=PARAMS_C[5])
            rc2.pbrs_calculator.path_calculator.build_level_cache(ld, adj, badj, gd)
            rollout("w", rc2, [(0, 0)], 1, record=False)
            kc = rollout("c", rc2, [mgr.ACTIONS[a] for a in acts], 4)
        kd = None
        if k == 3:
            # rollout "d": a hit of the position cache WITHOUT a next hop.  The only node without one is the exit door's goal node, at
            # most 8.5 px from the door, and a ninja whose closest node it is stands within 18.5 px of the door: it has won (22 px).
            # No play reaches the branch, so the replay runs up to the switch and the ninja is then PLACED on that node, beside it
            # and away from it, without a tick (frames 0, action 255)
            lc = rc.pbrs_calculator.path_calculator
            lc.build_level_cache(ld, adj, badj, gd)
            gp = lc.level_cache._goal_id_to_goal_pos["exit"]
            node = [n for n in adj if lc.level_cache.get_next_hop(n, "exit") is None
                    and lc.level_cache.get_geometric_distance(n, gp, "exit") == 0.0]
            assert len(node) == 1
            nx, ny = node[0][0] + 24.0, node[0][1] + 24.0
            kd = rollout("d", rc, [controls(int(b)) for b in corpus["in%d" % idx]], 1,
                         after_switch=[(nx, ny), (nx + 1.5, ny + 1.0), (nx - 2.0, ny + 0.5), (nx - 40.0, ny), (nx - 41.0, ny + 0.25)])
        print(k, tag, "const", out["const%d" % k].tolist(), "kinds [miss, hit, hit-no-hop, terminal] a", ka, "b", kb, "c", kc, "d", kd, flush=True)

    # ---- RewardConfig-independent pieces, called directly
    ks = [30.0, 50.0, 180.0, 1234.5]
    pot_in, pot_out = [], []
    for s2s in ks:
        for s2e in (10.0, 400.0):
            for sw in (False, True):
                kk = max(50.0, (s2s + s2e) * 2.0 if sw else s2s)
                for d in [0.0, 1e-9, 0.5 * kk, kk - 1e-9, kk, kk + 1e-9, 1.7 * kk, 3.0 * kk, 25.0 * kk, float("inf")]:
                    st = dict(switch_activated=sw, switch_x=500.0, switch_y=300.0, exit_door_x=700.0, exit_door_y=120.0, player_x=123.7,
                              player_y=456.2, _cached_switch_distance=d, _cached_exit_distance=d, _pbrs_spawn_to_switch_distance=s2s,
                              _pbrs_switch_to_exit_distance=s2e)
                    pot_in.append([s2s, s2e, float(sw), d, st["player_x"], st["player_y"], 500.0, 300.0, 700.0, 120.0])
                    pot_out.append(PBRSPotentials.objective_distance_potential(st, adjacency={}, level_data=None, path_calculator=None, graph_data=None))
    out["pot_in"], out["pot_out"] = np.array(pot_in, dtype=np.float64), np.array(pot_out, dtype=np.float64)
    app = [0.0, 1e-12, 0.3, 9.99, 50.0, 77.7, 99.0, 99.999999, 100.0 - 1e-13, 100.0, 100.0 + 1e-13, 101.0, 1e6, float("inf")]
    app += np.random.default_rng(5).uniform(0.0, 100.0, size=300).tolist()
    out["app_in"] = np.array(app, dtype=np.float64)
    out["app_out"] = np.array([fresh._calculate_completion_approach_bonus(d) for d in app], dtype=np.float64)
    out["app_none"] = np.array([fresh._calculate_completion_approach_bonus(None)], dtype=np.float64)

    print("coverage:", COVER)
    for name in ("miss", "hit", "hit_no_hop", "dist_milestone_switch", "dist_milestone_exit", "switch_live", "death", "win_efficiency",
                 "episode_start", "approach"):
        assert COVER[name] >= 1, name
    out["names"] = np.frombuffer("\n".join(tags).encode(), dtype=np.uint8)
    p = os.path.join(HERE, "reward.npz")
    np.savez_compressed(p, **out)
    print("reward.npz", os.path.getsize(p), "(pathmask.npz:", os.path.getsize(os.path.join(HERE, "pathmask.npz")), ")")
    if os.environ.get("NPP_REWARD_DEBUG"):
        np.savez_compressed(os.environ["NPP_REWARD_DEBUG"], **dbg)
    assert os.path.getsize(p) <= os.path.getsize(os.path.join(HERE, "pathmask.npz"))


if __name__ == "__main__":
    main()
