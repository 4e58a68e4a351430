"""Cost of seeding the cell index from replays for DESIGN.md 22: every replay of tests/golden/corpus.npz (all recorded wins) on
the level set of their distinct maps, N = 4096 envs, routes on, as wall time around work that ends in a synchronise; three
alternating windows, medians.  Two ways to the same index:

  seed   NppVecEnvironment.seed_archive_from_replays (npp_archive_seed: feed + tick + route append + propose + assign + store per
         tick, no Python inside a round)
  loop   the entries that existed before it, through the public API: per round assign_levels + reset, then per tick one
         NppBatch.tick and one NppBatch.archive_explore with the tick's score and candidate mask rows (uploaded once, inside the
         window, as dense [T, N] tensors)

    python tools/seed_cost.py [--out PATH]                 # both ways, alternating; the tables are compared
    python tools/seed_cost.py --loop-only --root <a built tree of the parent commit> [--out PATH]     # the loop AT the parent commit

    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/seed_cost.py --trace
                                    # kernel durations: two seedings (the first warms), nothing else

Writes profiles/seed_cost.json (or PATH) and prints one JSON line.
"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TREE = os.path.abspath(sys.argv[sys.argv.index("--root") + 1]) if "--root" in sys.argv else ROOT   # the package that is measured
sys.path.insert(0, TREE)
from nclone_amd import demos  # noqa: E402
from nclone_amd.replay import CompactReplay  # noqa: E402
from nclone_amd.vec_env import NppVecEnvironment  # noqa: E402

LOOP_ONLY = "--loop-only" in sys.argv
OUT = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "seed_cost.json")
N, SLOTS, CAP, ROUNDS = 4096, 16384, 2048, 3

c = np.load(os.path.join(TREE, "tests", "golden", "corpus.npz"))
n_rep = len(bytes(c["names"]).decode().split("\n"))
reps = [CompactReplay(bytes(c["m%d" % i]), c["in%d" % i].tolist(), True, 1) for i in range(n_rep)]
ids, levels, lid = {}, [], []
for r in reps:
    if r.map_data not in ids:
        ids[r.map_data] = len(levels)
        levels.append(np.frombuffer(r.map_data, dtype=np.uint8))
    lid.append(ids[r.map_data])
L = np.array([len(r.input_sequence) for r in reps], dtype=np.int64)


def make_env():
    return NppVecEnvironment(levels, N, frame_skip=1, truncation_limit=10000, checkpoint_slots=SLOTS, checkpoint_cells=True,
                             record_routes=True, route_capacity=CAP)


def tables(env):
    return {k: v.cpu().numpy().reshape(-1).copy() for k, v in env.batch.archive_cells().items()}


def seed(env):
    env.batch.archive_cells_create(seed=0)   # an empty index
    t0 = time.perf_counter()
    out = env.seed_archive_from_replays(reps, max_demos_per_level=1000)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def loop(env):
    """The same rule through tick + archive_explore: the schedule of demos.plan, progress scores."""
    b = env.batch
    b.archive_cells_create(seed=0)
    t0 = time.perf_counter()
    before = b.env_levels()
    plan = demos.plan(L, 1, int(L.max()), N)
    order = plan["order"]
    for q, ticks in enumerate(plan["round_ticks"]):
        envs = order[q * N:(q + 1) * N]
        lv = np.full(N, lid[envs[0]], dtype=np.int32)
        lv[:len(envs)] = [lid[r] for r in envs]
        rows = np.zeros((int(ticks), N), dtype=np.uint8)
        score = np.zeros((int(ticks), N), dtype=np.float32)
        mask = np.zeros((int(ticks), N), dtype=np.uint8)
        for e, r in enumerate(envs):
            rows[:L[r], e] = reps[r].input_sequence
            score[:L[r], e] = (np.arange(L[r], dtype=np.float64) / float(L[r])).astype(np.float32)
            mask[:L[r], e] = 1
        d_rows, d_score, d_mask = (torch.from_numpy(a).to(b.device) for a in (rows, score, mask))
        b.assign_levels(lv)
        b.reset(mode="full")
        for f in range(int(ticks)):
            b.tick(d_rows[f:f + 1])
            b.archive_explore(score=d_score[f], mask=d_mask[f])
    b.assign_levels(before)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


env = make_env()
if "--trace" in sys.argv:
    seed(env)
    ms, _ = seed(env)
    print(json.dumps({"trace": True, "seed_ms_under_the_profiler": ms}), flush=True)
    sys.exit(0)
ways = {"loop": lambda: loop(env)} if LOOP_ONLY else {"seed": lambda: seed(env)[0], "loop": lambda: loop(env)}
for fn in ways.values():   # warm: code objects, allocator, autotuner
    fn()
same = None
if not LOOP_ONLY:
    _, info = seed(env)
    a = tables(env)
    loop(env)
    bb = tables(env)
    same = all(np.array_equal(a[k].view(np.uint32), bb[k].view(np.uint32)) for k in ("cell_slot", "cell_score", "slot_key", "n_used"))
    cells, visits_seed, visits_loop = int(a["n_used"][0]), int(a["visits"].sum()), int(bb["visits"].sum())
ms = {k: [] for k in ways}
for r in range(ROUNDS):
    for key in (list(ways) if r % 2 == 0 else list(ways)[::-1]):
        ms[key].append(ways[key]())
ticks = int(demos.plan(L, 1, int(L.max()), N)["round_ticks"].sum())
out = {"tree": "this commit" if TREE == ROOT else "parent commit", "n_envs": N, "replays": n_rep, "levels": len(levels), "replay_ticks": int(L.sum()),
       "ticks_played": ticks, "slots": SLOTS, "route_capacity": CAP, "ms": ms, "median_ms": {k: float(np.median(v)) for k, v in ms.items()},
       "us_per_tick": {k: float(np.median(v) * 1e3 / ticks) for k, v in ms.items()},
       "launches_per_tick": {"seed": 6, "loop": 5}}
if not LOOP_ONLY:
    out.update(tables_equal=bool(same), cells=cells, visits_after_seed=visits_seed, visits_after_loop=visits_loop,
               counts=np.asarray(info["counts"].cpu()).sum(axis=0).tolist())
print(json.dumps(out), flush=True)
with open(OUT, "w") as f:
    json.dump(out, f, indent=1)
