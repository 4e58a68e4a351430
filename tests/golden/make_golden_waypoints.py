#!/usr/bin/env python3
"""Golden fixture for the sequential path waypoints of reward mode "pbrs": `RewardCalculator.calculate_reward` under a fresh
`RewardConfig()` (enable_path_waypoints=True, the reference's default), produced by RUNNING the reference.

Companion of make_golden_reward.py (same rules: build container only, never imported by the package, the tests, bench.py or
smoke(); the output is pure data).

    HOME=/tmp/orahome python3 tests/golden/make_golden_waypoints.py      # -> waypoints.npz

How the reference is run: exactly as make_golden_reward.py runs it (the env's life cycle re-enacted call by call, a one-tick warm-up
episode), on the same seven levels and action streams, with two additions: the calculator is `RewardCalculator(RewardConfig())`, and
after `build_level_cache` `extract_path_waypoints_for_level(level_data, graph_data, map_name)` is called as the graph mixin does
(mixins/graph_mixin.py:462).  `_calculate_sequential_waypoint_bonus` and `_calculate_waypoint_farming_penalty` are wrapped to record
what they are handed and what they return; nothing is restated.

Rows.  Per level k:
  m<k>, const<k>    as reward.npz
  path0_<k>, path1_<k>   i32[n, 2] the node paths spawn -> switch, switch -> exit of `_compute_original_paths`
  nodes<k>          i32[3, 2] spawn, switch and exit node
  wp<k>             f64[n, 4] the waypoint table in sequence order: x, y, phase (0 pre_switch, 1 post_switch), node_index
                    (absent on the level the reference refuses: const<k> is +inf)
rollouts "a" (300 random actions at frame skip 4), "b" (the level's own replay), for level 0 "c" (rollout "a"'s actions under the
non-default waypoint numbers params_wp_c), and on the first level with 8 pre-switch waypoints "e" (scripted placements, see main()); per rollout what reward.npz has ({p}act,
{p}frames, {p}flags, {p}pos, {p}rew, {p}comp, {p}kind) plus
  {p}wpb<k>         f64[steps] the unscaled waypoint bonus (0 on a terminal step: the bonus is not evaluated there)
  {p}wpi<k>         i32[steps, 4] collected seq index or -1, collection_type (0 none, 1 in_sequence, 2 out_of_sequence), next expected
                    index after the step, collected count after the step (both BEFORE the reset on a terminal step)
  {p}farm<k>        f64[steps] the farming penalty on death rows (0 elsewhere)
params_wp           f64[4] collection radius, out-of-order scale, progress scale, progress spacing of a fresh RewardConfig()
params_wp_c         those of rollout "c"
grid_in, grid_out   get_waypoint_bonus called directly: rows idx, total, in-sequence, progress scale, out-of-order scale
farm_distance_none  u8[1]: 1 = `obs.get("_pbrs_last_distance_to_goal")` was None at every death, so the penalty is always 0
names               newline-separated level tags
"""
import logging
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
STEPS = 300
LEVELS = [("reach.npz", "doors:replay:127"), ("reach.npz", "doors:replay:128"), ("reach.npz", "mines:replay:91"),
          ("reach.npz", "mines:replay:24"), ("reach.npz", "c0:replay:0"), ("reach2.npz", "c0:replay:20"),
          ("reach2.npz", "zoo:replay:16")]   # the seven levels of make_golden_reward.py
INPUT_TO_ACTION = {(0, 0): 0, (-1, 0): 1, (1, 0): 2, (0, 1): 3, (-1, 1): 4, (1, 1): 5}
PARAMS_WP_C = (22.0, 0.5, 0.5, 12.0)   # radius, out-of-order scale, progress scale, spacing


def controls(b):
    j, r, l = b & 1, (b >> 1) & 1, (b >> 2) & 1
    return (0 if (l and r) else (-1 if l else (1 if r else 0))), j


def main():
    sys.path.insert(0, HERE)
    import make_golden_reach as mgr

    mgr.prepare()
    import math
    from nclone.nplay_headless import NPlayHeadless
    from nclone.graph.level_data import LevelData, extract_start_position_from_map_data
    from nclone.gym_environment.entity_extractor import EntityExtractor
    from nclone.graph.reachability.graph_builder import GraphBuilder
    from nclone.graph.reachability.feature_computation import compute_reachability_features_from_graph
    from nclone.gym_environment.reward_calculation.main_reward_calculator import RewardCalculator
    from nclone.gym_environment.reward_calculation.reward_config import RewardConfig

    logging.disable(logging.CRITICAL)

    class ConfigC(RewardConfig):
        waypoint_progress_scale = property(lambda self: PARAMS_WP_C[2])

    class ConfigG(RewardConfig):   # the grid: the progress scale as a plain attribute
        scale = 2.0
        waypoint_progress_scale = property(lambda self: self.scale)

    corpus = np.load(os.path.join(HERE, "corpus.npz"))
    golden = np.load(os.path.join(HERE, "reward.npz"))
    fixtures, out, tags = {}, {}, []
    COVER = {k: 0 for k in ("in_sequence", "out_skip", "out_backwards", "post_blocked", "two_in_radius", "death_collected",
                            "episode_start_after_collection", "death", "win")}
    SCRIPTED = []   # the scripted rollout runs on the first level with enough waypoints of both phases
    FARM_NONE = [0, 0]   # deaths, deaths whose distance argument was None
    fresh = RewardConfig()
    out["params_wp"] = np.array([fresh.waypoint_collection_radius, fresh.waypoint_out_of_order_scale, fresh.waypoint_progress_scale,
                                 fresh.path_waypoint_progress_spacing], dtype=np.float64)
    out["params_wp_c"] = np.array(PARAMS_WP_C, dtype=np.float64)
    assert fresh.enable_path_waypoints is True

    for k, (fname, tag) in enumerate(LEVELS):
        if fname not in fixtures:
            z = np.load(os.path.join(HERE, fname))
            fixtures[fname] = (z, bytes(z["names"]).decode().split("\n"))
        z, names = fixtures[fname]
        m = z["m%d" % names.index(tag)]
        assert np.array_equal(np.asarray(m, dtype=np.float64), golden["m%d" % k])
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

        def instrument(rc):
            """record what the two waypoint functions are handed and return"""
            log = {"bonus": None, "farm": None}
            f_bonus, f_farm = rc._calculate_sequential_waypoint_bonus, rc._calculate_waypoint_farming_penalty

            def bonus(current_pos, previous_pos, switch_activated):
                # prev_player_pos was overwritten with the current position before the bonus runs (:534 before :662)
                assert previous_pos is not None and tuple(previous_pos) == tuple(current_pos), (previous_pos, current_pos)
                radius = rc.config.waypoint_collection_radius
                seq = rc._waypoint_sequence
                if not seq and rc.current_path_waypoints_by_phase:   # built inside the call: the same order
                    seq = [(w, w.phase, w.node_index) for ph in ("pre_switch", "post_switch") for w in rc.current_path_waypoints_by_phase.get(ph, [])]
                near = blocked = 0
                for w, ph, _i in seq:
                    if (w.position, ph) in rc._collected_path_waypoints:
                        continue
                    d = math.sqrt((current_pos[0] - w.position[0]) ** 2 + (current_pos[1] - w.position[1]) ** 2)
                    if d <= radius:
                        if ph == "post_switch" and not switch_activated:
                            blocked += 1
                        else:
                            near += 1
                nxt0 = rc._next_expected_waypoint_index
                b, mt = f_bonus(current_pos, previous_pos, switch_activated)
                log["bonus"] = (b, mt["collection_type"], near, blocked, nxt0)
                return b, mt

            def farm(distance_to_goal, optimal_distance, waypoints_collected, total_waypoints):
                v = f_farm(distance_to_goal, optimal_distance, waypoints_collected, total_waypoints)
                log["farm"] = (v, distance_to_goal is None, waypoints_collected)
                return v

            rc._calculate_sequential_waypoint_bonus = bonus
            rc._calculate_waypoint_farming_penalty = farm
            return log

        def rollout(prefix, rc, log, ctrl, ticks, record=True, compare=None):
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
            pos, flags, frames, rew, comp, kind, wpb, wpi, farm = [[prev["player_x"], prev["player_y"]]], [], [], [], [], [], [], [], []
            done = []
            for h, j in ctrl:
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
                m0 = pbrs._cache_misses
                log["bonus"] = log["farm"] = None
                r = rc.calculate_reward(o, prev, frames_executed=n_ticks)
                c = rc.last_pbrs_components
                term = bool(c["is_terminal"])
                if term:
                    kd = 3
                    cover["death" if o["player_dead"] else "win"] += 1
                    assert log["bonus"] is None
                else:
                    kd = 0 if pbrs._cache_misses > m0 else (2 if o.get("_pbrs_cache_hit") else 1)
                n_col, nxt = len(rc._collected_path_waypoints), rc._next_expected_waypoint_index
                if log["bonus"] is not None:
                    b, ctype, near, blocked, nxt0 = log["bonus"]
                    ct = {"none": 0, "in_sequence": 1, "out_of_sequence": 2}[ctype]
                    idx = nxt - 1 if ct else -1
                    wpb.append(b)
                    wpi.append([idx, ct, nxt, n_col])
                    cover["in_sequence"] += ct == 1
                    cover["out_skip"] += ct == 2 and idx > nxt0
                    cover["out_backwards"] += ct == 2 and idx + 1 < nxt0
                    cover["post_blocked"] += blocked > 0
                    cover["two_in_radius"] += near >= 2
                    assert (ct != 0) == (near > 0), (ct, near)
                else:   # a terminal step, or a calculator with waypoints off
                    wpb.append(0.0)
                    wpi.append([-1, 0, nxt, n_col])
                if log["farm"] is not None:
                    v, none, n_wp = log["farm"]
                    assert o["player_dead"] and n_wp == n_col
                    FARM_NONE[0] += 1
                    FARM_NONE[1] += bool(none)
                    farm.append(v)
                    cover["death_collected"] += n_col > 0
                else:
                    assert not o["player_dead"]
                    farm.append(0.0)
                flags.append(int(o["player_won"]) | int(o["player_dead"]) << 1 | int(o["switch_activated"]) << 2)
                frames.append(n_ticks)
                rew.append(r)
                comp.append([c["pbrs_reward"], c["milestone_reward"], c.get("completion_approach_bonus", 0.0),
                             c["terminal_reward"] if term else 0.0])
                kind.append(kd)
                prev = o
                if term:
                    cover["episode_start_after_collection"] += n_col > 0
                    prev = restart()
                    assert len(rc._collected_path_waypoints) == 0 and rc._next_expected_waypoint_index == 0
                pos.append([prev["player_x"], prev["player_y"]])
            traj = {"act": np.array([INPUT_TO_ACTION.get(c, 255) for c in done], dtype=np.uint8), "frames": np.array(frames, dtype=np.uint16),
                    "flags": np.array(flags, dtype=np.uint8), "pos": np.array(pos, dtype=np.float64), "rew": np.array(rew, dtype=np.float64),
                    "comp": np.array(comp, dtype=np.float64), "kind": np.array(kind, dtype=np.uint8)}
            if compare is not None:   # waypoints off: every row equals reward.npz
                for name, v in traj.items():
                    assert np.array_equal(v, golden["%s%s%d" % (compare, name, k)]), (tag, compare, name)
                assert not np.any(wpb) and not np.any(farm)
                return None
            if not record:
                return None
            for name, v in traj.items():
                if prefix == "c" and name in ("act", "frames", "flags", "pos"):   # the trajectory does not depend on the reward
                    assert np.array_equal(v, out["a%s%d" % (name, k)])
                else:
                    out["%s%s%d" % (prefix, name, k)] = v
            if prefix in "ab":   # the trajectories of reward.npz, which the device is known to follow
                for name in ("act", "frames", "flags", "pos"):
                    assert np.array_equal(traj[name], golden["%s%s%d" % (prefix, name, k)]), (tag, prefix, name)
            out["%swpb%d" % (prefix, k)] = np.array(wpb, dtype=np.float64)
            out["%swpi%d" % (prefix, k)] = np.array(wpi, dtype=np.int32)
            out["%sfarm%d" % (prefix, k)] = np.array(farm, dtype=np.float64)
            w = np.array(wpi, dtype=np.int32)
            return [int((w[:, 1] == 1).sum()), int((w[:, 1] == 2).sum())]

        def calculator(cfg):
            rc = RewardCalculator(cfg)
            rc.pbrs_calculator.path_calculator.build_level_cache(ld, adj, badj, gd)
            n = rc.extract_path_waypoints_for_level(ld, gd, tag)   # graph_mixin.py:462
            return rc, instrument(rc), n

        rc, log, n_wp = calculator(RewardConfig())
        out["m%d" % k] = np.asarray(m, dtype=np.float64)
        tags.append(tag)
        out["path0_%d" % k] = np.array(getattr(rc, "_cached_switch_path", None) or [], dtype=np.int32).reshape(-1, 2)
        out["path1_%d" % k] = np.array(getattr(rc, "_cached_exit_path", None) or [], dtype=np.int32).reshape(-1, 2)
        out["nodes%d" % k] = np.array([rc._cached_spawn_node, rc._cached_switch_node, rc._cached_exit_node], dtype=np.int32)
        try:
            rollout("w", rc, log, [(0, 0)], 1, record=False)   # warm-up episode: the level constants
        except RuntimeError as e:   # _compute_combined_path_distance raises: the reference cannot train on this level
            assert "Combined geometric path distance is infinite" in str(e), e
            assert np.all(np.isinf(golden["const%d" % k]))
            out["const%d" % k] = np.full(3, np.inf)
            print(k, tag, "the reference raises:", str(e)[:110], "(waypoints extracted: %d)" % n_wp, flush=True)
            continue
        pb = rc.pbrs_calculator
        out["const%d" % k] = np.array([pb._cached_spawn_to_switch_distance, pb._cached_switch_to_exit_distance,
                                       pb._cached_combined_path_distance], dtype=np.float64)
        assert np.array_equal(out["const%d" % k], golden["const%d" % k])
        seq = [w for ph in ("pre_switch", "post_switch") for w in sorted(rc.current_path_waypoints_by_phase[ph], key=lambda w: w.node_index)]
        assert len(seq) == n_wp
        out["wp%d" % k] = np.array([[w.position[0], w.position[1], float(w.phase == "post_switch"), float(w.node_index)] for w in seq],
                                   dtype=np.float64).reshape(-1, 4)
        acts = np.random.default_rng(52000 + k).integers(0, 6, size=STEPS)   # make_golden_reward.py's actions
        ctrl_a = [mgr.ACTIONS[a] for a in acts]
        idx = int(tag.rsplit(":", 1)[1])
        ctrl_b = [controls(int(b)) for b in corpus["in%d" % idx]]
        ka = rollout("a", rc, log, ctrl_a, 4)
        assert [(w.position, w.phase) for w, _p, _i in rc._waypoint_sequence] == [(w.position, w.phase) for w in seq] or not rc._waypoint_sequence
        kb = rollout("b", rc, log, ctrl_b, 1)
        kc = ke = None
        if k == 0:
            rc2, log2, n2 = calculator(ConfigC(waypoint_collection_radius=PARAMS_WP_C[0], waypoint_out_of_order_scale=PARAMS_WP_C[1]))
            assert n2 == n_wp
            rollout("w", rc2, log2, [(0, 0)], 1, record=False)
            kc = rollout("c", rc2, log2, ctrl_a, 4)
        W = out["wp%d" % k]
        n_pre = int((W[:, 2] == 0).sum())
        print(k, tag, "waypoints", n_wp, "pre", n_pre, flush=True)
        if "e" not in SCRIPTED and n_pre >= 8 and n_wp > n_pre + 1:
            SCRIPTED.append("e")
            # rollout "e": placements, without a tick (frames 0, action 255), on and beside waypoints in an order play does not
            # produce: a skip ahead, a step back to an uncollected earlier waypoint (next-expected moves backwards), in-sequence
            # collections from there, a spot within the radius of a post-switch waypoint while the switch is off
            spots = [(W[5, 0], W[5, 1]), (W[2, 0] + 1.5, W[2, 1] - 1.0), (W[3, 0], W[3, 1]), (W[4, 0] + 0.25, W[4, 1]), (W[4, 0] + 0.25, W[4, 1]),
                     (W[n_pre + 1, 0], W[n_pre + 1, 1] + 2.0), (W[7, 0] + 17.9, W[7, 1]), (W[7, 0] + 18.0, W[7, 1]), (W[0, 0], W[0, 1] + 0.5)]
            ke = rollout("e", rc, log, [("place", q) for q in spots], 1)
        # waypoints off: every row of reward.npz
        rc3 = RewardCalculator(RewardConfig(enable_path_waypoints=False))
        rc3.pbrs_calculator.path_calculator.build_level_cache(ld, adj, badj, gd)
        assert rc3.extract_path_waypoints_for_level(ld, gd, tag) == 0
        log3 = instrument(rc3)
        rollout("w", rc3, log3, [(0, 0)], 1, record=False)
        rollout("a", rc3, log3, ctrl_a, 4, compare="a")
        rollout("b", rc3, log3, ctrl_b, 1, compare="b")
        print(k, tag, "waypoints", n_wp, "pre", int((out["wp%d" % k][:, 2] == 0).sum()), "paths", len(out["path0_%d" % k]), len(out["path1_%d" % k]),
              "collections [in, out] a", ka, "b", kb, "c", kc, "e", ke, flush=True)

    # ---- get_waypoint_bonus, called directly
    cfg = ConfigG()
    gin, gout = [], []
    for total in (1, 2, 3, 7, 19, 20, 21, 40, 62, 300, 512):
        for i in sorted({0, 1, total // 2, total - 2, total - 1} & set(range(total))):
            for scale in (2.0, 1.5, 0.5, 0.0):
                for oscale in (0.3, 0.5):
                    for inseq in (True, False):
                        cfg.scale = scale
                        cfg.waypoint_out_of_order_scale = oscale
                        gin.append([i, total, float(inseq), scale, oscale])
                        gout.append(cfg.get_waypoint_bonus(collected_idx=i, total_waypoints=total, is_in_sequence=inseq))
    out["grid_in"], out["grid_out"] = np.array(gin, dtype=np.float64), np.array(gout, dtype=np.float64)

    print("coverage:", COVER, "deaths", FARM_NONE)
    for name in ("in_sequence", "out_skip", "out_backwards", "post_blocked", "two_in_radius", "death_collected", "episode_start_after_collection"):
        assert COVER[name] >= 1, name
    # DESIGN.md 20, quirk six: the distance is never in the observation calculate_reward gets, so the farming penalty is always 0
    assert FARM_NONE[0] > 0 and FARM_NONE[0] == FARM_NONE[1]
    out["farm_distance_none"] = np.array([1], dtype=np.uint8)
    out["names"] = np.frombuffer("\n".join(tags).encode(), dtype=np.uint8)
    p = os.path.join(HERE, "waypoints.npz")
    np.savez_compressed(p, **out)
    print("waypoints.npz", os.path.getsize(p), "(reward.npz:", os.path.getsize(os.path.join(HERE, "reward.npz")), ")")
    assert os.path.getsize(p) <= 3 * os.path.getsize(os.path.join(HERE, "reward.npz"))


if __name__ == "__main__":
    main()
