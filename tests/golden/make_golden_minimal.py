#!/usr/bin/env python3
"""Golden fixture for the reference's MINIMAL observation mode (gym_environment/config.py:17-20 `observation_mode`;
npp_environment.py:2232-2270): the 40 floats of `compute_minimal_observation`
(gym_environment/observation_processor.py:505-567), produced by RUNNING the reference.

Companion of make_golden.py / make_golden_reach.py / make_golden_obs.py (same rules: build container only, never imported by
the package, the tests, bench.py or smoke(); the output is pure data).

    HOME=/tmp/orahome python3 tests/golden/make_golden_minimal.py      # -> minimal.npz

How the reference is run.  Nothing is restated; the three pieces are obtained by the means the sibling generators use:
  * the reference package with its generated tables, and the bare package objects for `nclone.gym_environment`:
    make_golden_reach.prepare().  The environment class cannot be instantiated, so its call sequence is re-enacted exactly as
    make_golden_reach.main() does (graph once per level at the spawn, the 38 features recomputed only when
    (ninja cell, exit_switch_activated) changes, `clear_step_cache()` at every step, `clear_cache()` at every episode reset);
  * `spatial_context[64:]`: make_golden.spatial_context_row() on the module make_golden.load_spatial_context() loads, with
    `reset_mine_overlay_cache()` at every reset (npp_environment.py:569-571), called at the terminal observation too, as the env does;
  * `compute_minimal_observation`: its FunctionDef is taken out of observation_processor.py with `ast` and compiled as it
    stands, as make_golden_obs.py does for its two methods (the module imports cv2, which is not installed).
Every line that computes a stored number is the reference's.

Levels (all from reach.npz / reach2.npz, so that npp_reachability serves every one of them): three locked-door levels, four
toggle-mine levels, one exit-only level, and the entity-zoo levels with launch pads (Entity.type 10).  A launch-pad level is
rolled out with the first of SEEDS_LP random plans during which an observation shows the ninja inside its launch-pad buffer
(column 39 >= 0); the generator prints which, or that none did.
RESULT of the run that wrote the committed file: none did -- on none of the three launch-pad levels, in none of the 12 plans.
Checked beyond that while writing this generator: on all 23 entity-zoo levels with launch pads, neither six 300-step random
plans, nor the level's own replay from corpus.npz down-sampled to one action per four ticks (all four offsets), nor that replay
played tick by tick ever leaves `launch_pad_buffer` >= 0 at the end of a tick.  Column 39 is therefore pinned at -1 ONLY by this
fixture; the device twin test of tests/test_gpu_minimal_obs.py checks the column's encoding against npp_dump_state's buffer
field on whatever values its rollouts reach.

Output minimal.npz, per level k (steps = 300):
  m<k>   map_data f64
  a<k>   u8[steps] actions; t<k> u8[steps] 1 where the step ended the episode (Simulator.reset follows)
  o<k>   f32[steps + 1, 40] the rows the env returns: row 0 after reset; after a terminal step the row of the reset state, as
         a vector env returns it
  ot<k>  f32[n_terminal, 40] the row of the terminal state itself for the steps with t = 1, in step order (a dead or
         celebrating ninja: `state` capped at one-hot index 4); st<k> u8[steps + 1] / stt<k> u8[n_terminal] ninja.state there
  rf<k>  f32[steps + 1, 38] reachability_features and sc<k> f32[steps + 1, 48] mine overlay behind each row of o<k> (diagnosis)
names: newline-separated level tags.
"""
import ast
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
SRC = "/root/reference"
STEPS = 300
SEEDS_LP = 12
ZERO_COLUMNS = (14, 15, 18)   # identically 0 in what the reference produces when run this way (see the issue / DESIGN.md 14)


def reference_minimal():
    path = os.path.join(SRC, "nclone", "gym_environment", "observation_processor.py")
    tree = ast.parse(open(path).read(), filename=path)
    fns = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "compute_minimal_observation"]
    assert len(fns) == 1
    ns = {"np": np}
    exec(compile(ast.Module(body=fns, type_ignores=[]), path, "exec"), ns)
    return ns["compute_minimal_observation"]


def coverage(rows, term_states):
    """(columns with fewer than two distinct values, rows whose `state` is capped) over all rows of the fixture."""
    allrows = np.concatenate(rows)
    flat = [c for c in range(40) if len(np.unique(allrows[:, c])) < 2]
    return flat, int(sum(int((s > 4).sum()) for s in term_states))


def main():
    sys.path.insert(0, HERE)
    import make_golden_reach as mgr

    mgr.prepare()
    import nclone  # noqa: F401  (binds the package to the prepared copy before make_golden adds its own path entry)

    import make_golden as mg
    from nclone.nplay_headless import NPlayHeadless
    from nclone.graph.level_data import LevelData, extract_start_position_from_map_data
    from nclone.gym_environment.entity_extractor import EntityExtractor
    from nclone.graph.reachability.graph_builder import GraphBuilder
    from nclone.graph.reachability.path_distance_calculator import CachedPathDistanceCalculator
    from nclone.graph.reachability.feature_computation import compute_reachability_features_from_graph

    minimal = reference_minimal()
    sc = mg.load_spatial_context()
    sys.path.insert(0, ROOT)
    from nclone_amd.levels import curriculum0_levels, door_levels, mine_levels, zoo_levels

    levels, tags, wants_lp = [], [], []

    def pick(fn, prefix, names):
        lv, tg = fn()
        for name in names:
            levels.append(lv[tg.index(name)])
            tags.append(prefix + name)
            wants_lp.append(False)

    pick(door_levels, "doors:", ["replay:127", "hcorr:door:100003", "test_maps:switch-puzzle-1"])
    pick(mine_levels, "mines:", ["replay:12", "replay:71", "hcorr:mines:100001", "hcorr:mines:100017"])
    pick(curriculum0_levels, "c0:", ["replay:0"])
    lv, tg = zoo_levels()
    for m, t in zip(lv, tg):
        hp = NPlayHeadless(enable_rendering=False)
        hp.load_map_from_map_data(mgr.to_list(m))
        if len(hp.sim.entity_dic.get(10, [])) > 0 and sum(wants_lp) < 3:
            levels.append(m)
            tags.append("zoo:" + t)
            wants_lp.append(True)
    assert sum(wants_lp) >= 1, "no entity-zoo level with launch pads"

    out = {}
    all_rows, all_term_states = [], []
    for k, m in enumerate(levels):
        best = None
        for attempt in range(SEEDS_LP if wants_lp[k] else 1):
            hp = NPlayHeadless(enable_rendering=False)
            hp.load_map_from_map_data(mgr.to_list(m))
            tiles = np.zeros((23, 42), dtype=np.int32)
            for (x, y), t in hp.get_tile_data().items():
                if 0 <= x - 1 < 42 and 0 <= y - 1 < 23:
                    tiles[y - 1, x - 1] = int(t)
            ents = EntityExtractor(hp).extract_graph_entities()
            ld = LevelData(start_position=extract_start_position_from_map_data(hp.sim.map_data), tiles=tiles, entities=ents,
                           switch_states={}, curriculum_stage=None)
            gb = GraphBuilder()
            pos = hp.ninja_position()
            gd = gb.build_graph(ld, ninja_pos=(int(pos[0]), int(pos[1])))
            pc = CachedPathDistanceCalculator(max_cache_size=200, use_astar=True)
            pc.build_level_cache(ld, gd["adjacency"], gd.get("base_adjacency"), gd)
            acts = np.random.default_rng(77000 + 100 * attempt + k).integers(0, 6, size=STEPS).astype(np.uint8)
            state = {"key": None, "cached": None}

            def reach():
                pos = hp.ninja_position()
                key = ((int(pos[0] // 24), int(pos[1] // 24)), hp.exit_switch_activated())
                if key != state["key"] or state["cached"] is None:
                    pc.build_level_cache(ld, gd["adjacency"], gd.get("base_adjacency", gd["adjacency"]), gd)
                    f, _sd, _ed = compute_reachability_features_from_graph(gd["adjacency"], gd, ld, pos, pc,
                                                                           goal_positions=hp.get_goal_positions_for_features())
                    state["key"], state["cached"] = key, f.copy()
                return state["cached"].copy()

            def observe():
                rf = reach()
                row = mg.spatial_context_row(sc, hp, tiles)
                return minimal(hp.sim.ninja, rf, row[64:]), rf, row[64:], int(hp.sim.ninja.state)

            sc.reset_mine_overlay_cache()
            O, RF, SC, ST, T, OT, STT = [], [], [], [], [], [], []
            o, rf, ov, st = observe()
            O.append(o); RF.append(rf); SC.append(ov); ST.append(st)
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
                o, rf, ov, st = observe()   # the observation of this step (the terminal one if term)
                if term:
                    OT.append(o); STT.append(st)
                    hp.reset()
                    pc.clear_cache()   # _reset_reachability_state
                    sc.reset_mine_overlay_cache()
                    o, rf, ov, st = observe()   # what a vector env returns after auto-reset
                O.append(o); RF.append(rf); SC.append(ov); ST.append(st)
            run = {"a": acts, "t": np.array(T, dtype=np.uint8), "o": np.array(O, dtype=np.float32),
                   "ot": np.array(OT, dtype=np.float32).reshape(-1, 40), "st": np.array(ST, dtype=np.uint8),
                   "stt": np.array(STT, dtype=np.uint8), "rf": np.array(RF, dtype=np.float32), "sc": np.array(SC, dtype=np.float32)}
            touched = bool((run["o"][:, 39] >= 0).any())
            if best is None or touched:
                best = (attempt, run, touched)
            if touched or not wants_lp[k]:
                break
        attempt, run, touched = best
        out["m%d" % k] = np.asarray(m, dtype=np.float64)
        for key, v in run.items():
            out["%s%d" % (key, k)] = v
        all_rows += [run["o"], run["ot"]]
        all_term_states.append(run["stt"])
        near = int((np.abs(run["sc"].reshape(-1, 8, 6)[:, 3, :2]).sum(axis=1) > 0).sum())
        print(k, tags[k], "episodes", int(run["t"].sum()), "rows with a 4th mine", near, "plan", attempt,
              "launch pad buffer seen" if touched else ("NO launch pad buffer in %d plans" % SEEDS_LP if wants_lp[k] else ""), flush=True)
    out["names"] = np.frombuffer("\n".join(tags).encode(), dtype=np.uint8)
    flat, capped = coverage(all_rows, all_term_states)
    print("columns with a single value:", flat, "(expected:", list(ZERO_COLUMNS), "); rows with a capped state:", capped)
    allrows = np.concatenate(all_rows)
    assert all((allrows[:, c] == 0).all() for c in ZERO_COLUMNS)
    p = os.path.join(HERE, "minimal.npz")
    np.savez_compressed(p, **out)
    print("minimal.npz", os.path.getsize(p))


if __name__ == "__main__":
    main()
