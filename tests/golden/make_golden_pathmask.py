#!/usr/bin/env python3
"""Golden fixture for path-direction action masking: the direction `_detect_straight_path_direction`
(gym_environment/base_environment.py:3109-3253) returns at every observation and the mask `Ninja.get_valid_action_mask()`
(ninja.py:743-800) makes of it in masking mode "hard", produced by RUNNING the reference.

Companion of make_golden.py / make_golden_reach.py / make_golden_minimal.py (same rules: build container only, never imported by
the package, the tests, bench.py or smoke(); the output is pure data).

    HOME=/tmp/orahome python3 tests/golden/make_golden_pathmask.py      # -> pathmask.npz

How the reference is run.  Nothing is restated:
  * the reference package with its generated tables and the bare package objects for `nclone.gym_environment`:
    make_golden_reach.prepare(); the graph and the level cache are built by the call sequence of make_golden_reach.main() -- one
    graph per level at the spawn, CachedPathDistanceCalculator.build_level_cache on it -- which is what the env keeps for an episode;
  * `_detect_straight_path_direction`: its FunctionDef is taken out of base_environment.py with `ast` and compiled as it stands
    (as make_golden_minimal.py does for compute_minimal_observation), and called on a stand-in `self` that carries only what the
    function touches: reward_calculator.pbrs_calculator.path_calculator, nplay_headless, current_graph_data, _spatial_hash /
    _subcell_lookup (None) and _deterministic_mask_applied_count.  The function swallows every exception and returns None; the
    generator counts the tracebacks it prints and asserts there were none;
  * the env's real spatial hash changes nothing: SpatialHash (graph/reachability/spatial_hash.py) has find_closest and
    find_all_within_radius but no `query`, so the `spatial_hash.query(...)` of find_ninja_node (pathfinding_utils.py:1385-1397)
    raises, is swallowed, and the linear scan runs -- asserted below, documented in npp_reach_features.hpp;
  * the masks: NPlayHeadless.get_action_mask() with sim._action_masking_mode = "hard" and sim._path_straightness_direction set as
    _get_action_mask_with_path_update (:3075-3107) sets them -- to None for the inert mask (what the step kernel's action_mask is
    pinned against), to the detector's result for the hard mask.

Rows.  Per level k two rollouts -- prefix "a": 300 random actions at frame skip 4 (the episode ends at the tick the ninja wins or
dies, Simulator.reset follows); prefix "b": the level's own recorded replay from corpus.npz, one action per tick (frame skip 1),
which reaches the switch, the exit phase and the door -- and probes, where the detector (it reads a position and the switch bit
only) is called off-trajectory through a stand-in nplay_headless.
  m<k>            map_data f64
  {a,b}act<k>     u8[steps] action (0..5); {a,b}term<k> u8[steps] 1 where the step ended the episode
  {a,b}pos<k>     f64[steps + 1, 2] position at the observation a vector env returns: row 0 after the reset, after a terminal step
                  the row of the reset state; {a,b}sw<k> u8 exit_switch_activated; {a,b}inert<k> u8 the six bits of the inert mask
                  (bit a = action a valid); {a,b}dir<k> i8 direction 0 none 1 left 2 right 3 down; {a,b}hard<k> u8 bits of the hard
                  mask; {a,b}graph<k> u8 1 where `_deterministic_mask_applied_count` went up
  {a,b}t*<k>      the same six columns for the terminal observations themselves (steps with term = 1, in step order)
  lat             f64[5] x0, y0, step, nx, ny: the probe lattice x0 + step * i, y0 + step * j over the whole level, solid tiles and
                  cells outside the flood fill included; latdir<k> i8[2, nx, ny], latgraph<k> u8[2, nx, ny] by switch bit
  ppos<k>         f64[n, 2] further probe positions: every node, +-9.9 / +-10.1 px around a few nodes, rings of radius 11.9 / 12.0 /
                  12.1 around both goals with the axis points and the points |dx| == 2 |dy|; pdir<k> i8[2, n], pgraph<k> u8[2, n]
names: newline-separated level tags (all from reach.npz / reach2.npz).

RESULT of the run that wrote the committed file (the generator prints and asserts the coverage): every direction in at least 763
probe rows under either goal; rollout rows by (switch bit; none, left, right, down): (0; 1935, 322, 68, 280), (1; 261, 0, 9, 54);
the no-node branch in 198 648 probes, the box fallback in 9 111; the near-goal branch returned none, left and right -- in probes only.
No trajectory row lies within 12 px of its goal, not even on doors:replay:127: the ninja collects a switch at 16 px (radii 10 + 6)
and enters a door at 22 px (10 + 12), so a rollout cannot reach that branch while the goals sit where the map puts them.
"""
import ast
import logging
import os
import sys
import traceback
import types
from typing import Optional

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
SRC = "/root/reference"
STEPS = 300
LATTICE = (1.3, 2.7, 4.0)   # x0, y0, step: 264 x 150 points
LEVELS = [("reach.npz", "doors:replay:127"), ("reach.npz", "doors:replay:128"),       # locked doors (127: switch 6 px from its door)
          ("reach.npz", "mines:replay:91"), ("reach.npz", "mines:replay:24"),         # toggle mines
          ("reach.npz", "c0:replay:0"),                                               # exit only
          ("reach2.npz", "c0:replay:20"),                                             # ReachHdr::miss_exit
          ("reach2.npz", "zoo:replay:16")]                                            # entity zoo
DIRS = {None: 0, "left": 1, "right": 2, "down": 3}
INPUT_TO_ACTION = {(0, 0): 0, (-1, 0): 1, (1, 0): 2, (0, 1): 3, (-1, 1): 4, (1, 1): 5}


def reference_detector():
    path = os.path.join(SRC, "nclone", "gym_environment", "base_environment.py")
    tree = ast.parse(open(path).read(), filename=path)
    cls = [n for n in tree.body if isinstance(n, ast.ClassDef)]
    fns = [f for c in cls for f in c.body if isinstance(f, ast.FunctionDef) and f.name == "_detect_straight_path_direction"]
    assert len(fns) == 1
    ns = {"Optional": Optional, "logger": logging.getLogger("pathmask")}
    exec(compile(ast.Module(body=fns, type_ignores=[]), path, "exec"), ns)
    return ns["_detect_straight_path_direction"]


def controls(b):
    """replay input byte -> (hor, jump) as make_golden.controls (replay/replay_executor.py:61-84; its package needs cv2)"""
    j, r, l = b & 1, (b >> 1) & 1, (b >> 2) & 1
    return (0 if (l and r) else (-1 if l else (1 if r else 0))), j


def bits(mask):
    return sum(1 << a for a in range(6) if mask[a])


def main():
    sys.path.insert(0, HERE)
    import make_golden_reach as mgr

    mgr.prepare()
    from nclone.nplay_headless import NPlayHeadless
    from nclone.graph.level_data import LevelData, extract_start_position_from_map_data
    from nclone.gym_environment.entity_extractor import EntityExtractor
    from nclone.graph.reachability.graph_builder import GraphBuilder
    from nclone.graph.reachability.path_distance_calculator import CachedPathDistanceCalculator
    from nclone.graph.reachability.spatial_hash import SpatialHash

    assert not hasattr(SpatialHash, "query")   # find_ninja_node always ends in its linear scan
    detect = reference_detector()
    failures = []
    traceback.print_exc = lambda *a, **k: failures.append(traceback.format_exc())   # the detector's `except Exception`
    logging.getLogger("pathmask").setLevel(logging.CRITICAL)

    corpus = np.load(os.path.join(HERE, "corpus.npz"))
    fixtures = {}
    out = {}
    tags = []
    cover = {"probe": np.zeros((2, 4), int), "roll": np.zeros((2, 4), int), "near": set(), "no_node": 0, "box": 0}
    x0, y0, step = LATTICE
    nx, ny = int((1056 - x0) // step) + 1, int((600 - y0) // step) + 1
    out["lat"] = np.array([x0, y0, step, nx, ny], dtype=np.float64)
    lx, ly = x0 + step * np.arange(nx), y0 + step * np.arange(ny)
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
        gb = GraphBuilder()
        pos = hp.ninja_position()
        gd = gb.build_graph(ld, ninja_pos=(int(pos[0]), int(pos[1])))
        pc = CachedPathDistanceCalculator(max_cache_size=200, use_astar=True)
        pc.build_level_cache(ld, gd["adjacency"], gd.get("base_adjacency"), gd)

        env = types.SimpleNamespace(
            reward_calculator=types.SimpleNamespace(pbrs_calculator=types.SimpleNamespace(path_calculator=pc)),
            nplay_headless=hp, current_graph_data=gd, _spatial_hash=None, _subcell_lookup=None, _deterministic_mask_applied_count=0)

        def observe():
            """(position, switch bit, inert bits, direction, hard bits, from-graph bit) as _get_action_mask_with_path_update does"""
            p = hp.ninja_position()
            hp.sim._action_masking_mode = "hard"
            hp.sim._path_straightness_direction = None
            inert = bits(np.array(hp.get_action_mask(), dtype=np.int8))
            c0 = env._deterministic_mask_applied_count
            d = detect(env)
            hp.sim._path_straightness_direction = d
            hard = bits(np.array(hp.get_action_mask(), dtype=np.int8))
            hp.sim._path_straightness_direction = None
            return [p[0], p[1]], int(hp.exit_switch_activated()), inert, DIRS[d], hard, env._deterministic_mask_applied_count - c0

        def rollout(prefix, controls, ticks):
            hp.reset()
            rows, trows, term = [observe()], [], []
            for h, j in controls:
                done = 0
                for _ in range(ticks):
                    hp.tick(h, j)
                    if hp.sim.ninja.state in (6, 7, 8):
                        done = 1
                        break
                term.append(done)
                row = observe()   # the observation of this step (the terminal one if done)
                if done:
                    trows.append(row)
                    hp.reset()
                    row = observe()   # what a vector env returns after the auto-reset
                rows.append(row)
            out["%sact%d" % (prefix, k)] = np.array([INPUT_TO_ACTION[c] for c in controls], dtype=np.uint8)
            out["%sterm%d" % (prefix, k)] = np.array(term, dtype=np.uint8)
            for pre, rr in ((prefix, rows), (prefix + "t", trows)):
                out["%spos%d" % (pre, k)] = np.array([r[0] for r in rr], dtype=np.float64).reshape(-1, 2)
                for col, (name, dt) in enumerate([("sw", np.uint8), ("inert", np.uint8), ("dir", np.int8), ("hard", np.uint8),
                                                  ("graph", np.uint8)], start=1):
                    out["%s%s%d" % (pre, name, k)] = np.array([r[col] for r in rr], dtype=dt)
            for r in rows + trows:
                cover["roll"][r[1], r[3]] += 1
            return sum(term)

        acts = np.random.default_rng(52000 + k).integers(0, 6, size=STEPS)
        ep_a = rollout("a", [mgr.ACTIONS[a] for a in acts], 4)
        idx = int(tag.rsplit(":", 1)[1])
        assert np.array_equal(np.asarray(m, dtype=np.float64), corpus["m%d" % idx].astype(np.float64)), tag
        ep_b = rollout("b", [controls(int(b)) for b in corpus["in%d" % idx]], 1)
        hp.reset()

        # ---- probes: the detector on a stand-in nplay_headless (it reads the position and the switch bit only)
        probe = types.SimpleNamespace(pos=(0.0, 0.0), sw=False)
        stand_in = types.SimpleNamespace(ninja_position=lambda: probe.pos, exit_switch_activated=lambda: probe.sw,
                                         exit_switch_position=hp.exit_switch_position, exit_door_position=hp.exit_door_position)
        env.nplay_headless = stand_in
        adj = gd["adjacency"]

        def branch(p):   # which branch of find_ninja_node the probe takes (coverage bookkeeping only, not stored)
            qx, qy = p[0] - 24, p[1] - 24
            if any((x - qx) ** 2 + (y - qy) ** 2 <= 100.0 for x, y in adj):
                return "node"
            if any(abs(x + 24 - p[0]) < 24 and abs(y + 24 - p[1]) < 24 for x, y in adj):
                return "box"
            return "none"

        def run(points):
            d = np.zeros((2, len(points)), dtype=np.int8)
            g = np.zeros((2, len(points)), dtype=np.uint8)
            for s in (0, 1):
                goal = hp.exit_door_position() if s else hp.exit_switch_position()
                for i, p in enumerate(points):
                    probe.pos, probe.sw = (float(p[0]), float(p[1])), bool(s)
                    c0 = env._deterministic_mask_applied_count
                    r = detect(env)
                    d[s, i], g[s, i] = DIRS[r], env._deterministic_mask_applied_count - c0
                    cover["probe"][s, d[s, i]] += 1
                    if ((goal[0] - p[0]) ** 2 + (goal[1] - p[1]) ** 2) ** 0.5 < 12.0:
                        cover["near"].add(int(d[s, i]))
                    elif s == 0:
                        b = branch(p)
                        cover["no_node"] += b == "none"
                        cover["box"] += b == "box"
            return d, g

        d, g = run([(x, y) for x in lx for y in ly])
        out["latdir%d" % k], out["latgraph%d" % k] = d.reshape(2, nx, ny), g.reshape(2, nx, ny)
        nodes = list(adj.keys())
        pts = [(x + 24.0, y + 24.0) for x, y in nodes]
        for x, y in nodes[::max(1, len(nodes) // 6)][:6]:
            for r in (9.9, 10.1):
                pts += [(x + 24.0 + r, y + 24.0), (x + 24.0 - r, y + 24.0), (x + 24.0, y + 24.0 + r), (x + 24.0, y + 24.0 - r)]
        for goal in (hp.exit_switch_position(), hp.exit_door_position()):
            for r in (11.9, 12.0, 12.1):
                pts += [(goal[0] + r, goal[1]), (goal[0] - r, goal[1]), (goal[0], goal[1] + r), (goal[0], goal[1] - r)]
                e = r / 5.0 ** 0.5
                pts += [(goal[0] + sx * 2.0 * e, goal[1] + sy * e) for sx in (-1, 1) for sy in (-1, 1)]
                pts += [(goal[0] + r * np.cos(t), goal[1] + r * np.sin(t)) for t in np.linspace(0.1, 2 * np.pi + 0.1, 16, endpoint=False)]
            pts += [(goal[0] + dx, goal[1] + dy) for dx in (-6.0, -2.0, 0.0, 2.0, 6.0) for dy in (-2.0, 0.0, 1.0, 3.0)]
        out["ppos%d" % k] = np.array(pts, dtype=np.float64)
        out["pdir%d" % k], out["pgraph%d" % k] = run(pts)
        out["m%d" % k] = np.asarray(m, dtype=np.float64)
        tags.append(tag)
        print(k, tag, "episodes", ep_a, ep_b, "nodes", len(nodes), "probes", 2 * (nx * ny + len(pts)), flush=True)

    assert not failures, failures[0]
    print("probe rows by (switch bit, direction):", cover["probe"].tolist())
    print("rollout rows by (switch bit, direction):", cover["roll"].tolist())
    print("near-goal branch returned", sorted(cover["near"]), "no-node probes", cover["no_node"], "box-fallback probes", cover["box"])
    assert (cover["probe"] >= 50).all()
    for s in (0, 1):
        assert cover["roll"][s, 1] + cover["roll"][s, 2] >= 1 and cover["roll"][s, 3] >= 1 and cover["roll"][s, 0] >= 1
    assert cover["near"] >= {0, 1, 2} and cover["no_node"] > 0 and cover["box"] > 0
    out["names"] = np.frombuffer("\n".join(tags).encode(), dtype=np.uint8)
    p = os.path.join(HERE, "pathmask.npz")
    np.savez_compressed(p, **out)
    print("pathmask.npz", os.path.getsize(p), "(minimal.npz:", os.path.getsize(os.path.join(HERE, "minimal.npz")), ")")
    assert os.path.getsize(p) <= os.path.getsize(os.path.join(HERE, "minimal.npz"))


if __name__ == "__main__":
    main()
