"""Cost of the demonstration player for DESIGN.md 21: the 130 replays of tests/golden/corpus.npz at frame skip 1 and 4 with all
vector keys, as HIP-event times over three alternating windows; medians.  Two ways to the same dataset:

  demo      nclone_amd.demos: the ragged table, npp_demo_play (feed + tick + observe + reachability + collect per period), on an
            existing player -- and, separately, load_demonstrations end to end (handle, level upload, tables, play) as wall time
  baseline  the EXISTING entries only: one env per replay, a dense [T, N] input tensor, tick + observe + reachability per period,
            every period's rows cloned, the dataset's rows gathered with torch indexing

Writes profiles/demo_cost.json and prints one JSON line per frame skip.

    python tools/demo_cost.py
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/demo_cost.py --trace 4
                                    # kernel durations: one play at that frame skip
"""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nclone_amd.demos import DemoPlayer, load_demonstrations  # noqa: E402
from nclone_amd.engine import NppBatch  # noqa: E402
from nclone_amd.replay import CompactReplay  # noqa: E402

TRACE = int(sys.argv[sys.argv.index("--trace") + 1]) if "--trace" in sys.argv else None
KEYS = ("game_state", "action_mask", "entity_positions", "spatial_context", "reachability_features", "mine_sdf_features", "switch_states")
BLOCK = {"game_state": "game_state", "action_mask": "action_mask", "entity_positions": "entity_pos", "spatial_context": "spatial_context",
         "reachability_features": "reachability_features", "mine_sdf_features": "mine_sdf_features", "switch_states": "switch_states",
         "positions": "positions", "flags": "flags", "status": "reach_status"}
ROUNDS = 3

c = np.load(os.path.join(ROOT, "tests", "golden", "corpus.npz"))
n_rep = len(bytes(c["names"]).decode().split("\n"))
reps = [CompactReplay(bytes(c["m%d" % i]), c["in%d" % i].tolist(), True, 1) for i in range(n_rep)]
L = np.array([len(r.input_sequence) for r in reps])


class Baseline:
    """One env per replay through the existing entries."""

    def __init__(self, fs):
        self.fs = fs
        ids, levels, lid = {}, [], []
        for r in reps:
            if r.map_data not in ids:
                ids[r.map_data] = len(levels)
                levels.append(np.frombuffer(r.map_data, dtype=np.uint8))
            lid.append(ids[r.map_data])
        self.lid = np.array(lid)
        self.rows = L // fs
        self.periods = int(self.rows.max())
        self.b = NppBatch(n_rep, autoreset=False, outputs=("spatial_context", "positions", "switch_states", "reachability_features",
                                                           "mine_sdf_features", "reach_status"))
        self.b.load_levels(levels)
        dense = np.zeros((self.periods * fs, n_rep), dtype=np.uint8)   # the dense tensor validate_replays uploads
        for k, r in enumerate(reps):
            m = min(L[k], self.periods * fs)
            dense[:m, k] = r.input_sequence[:m]
        self.dense = dense
        # dataset row -> (period, env), replay-major
        per = np.concatenate([np.arange(self.rows[r]) for r in range(n_rep)])
        env = np.concatenate([np.full(self.rows[r], r) for r in range(n_rep)])
        self.pick = torch.from_numpy(per * n_rep + env).cuda()

    def play(self):
        b, fs = self.b, self.fs
        d_in = torch.from_numpy(self.dense).to(b.device)
        b.assign_levels(self.lid)
        b.reset(mode="full")
        per = {k: [] for k in BLOCK}
        for p in range(self.periods):
            b.tick(d_in[p * fs:(p + 1) * fs])
            b.observe()
            b.reachability(with_switch_states=True)
            for k, src in BLOCK.items():
                per[k].append(b.out.t[src].clone())
        out = {}
        for k in BLOCK:
            st = torch.stack(per[k])
            out[k] = st.reshape((st.shape[0] * st.shape[1],) + tuple(st.shape[2:])).index_select(0, self.pick)
        return out


results = []
for fs in (1, 4):
    if TRACE is not None and fs != TRACE:
        continue
    player = DemoPlayer(reps, fs, 10_000, KEYS, n_rep, 0, "ones")
    planes = player.allocate()
    if TRACE is not None:
        player.play(planes)
        player.play(planes)
        player.batch.sync()
        print(json.dumps({"frame_skip": fs, "rows": player.rows_total, "plays": 2}), flush=True)
        continue
    base = Baseline(fs)
    ways = {"demo": lambda: player.play(planes), "baseline": base.play}
    for fn in ways.values():   # warm: tables, allocator
        fn()
    torch.cuda.synchronize()
    got = base.play()
    player.play(planes)
    torch.cuda.synchronize()
    same = all(torch.equal(planes[k].contiguous().view(torch.uint8), got[k].contiguous().view(torch.uint8))
               for k in BLOCK if k not in ("game_state", "action_mask", "flags"))
    same = same and torch.equal(planes["game_state"][:, :40], got["game_state"][:, :40])
    ms = {k: [] for k in ways}
    for r in range(ROUNDS):
        for key in (list(ways) if r % 2 == 0 else list(ways)[::-1]):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record(torch.cuda.current_stream())
            ways[key]()
            e1.record(torch.cuda.current_stream())
            torch.cuda.synchronize()
            ms[key].append(e0.elapsed_time(e1))
    wall = []
    for r in range(ROUNDS):
        t0 = time.perf_counter()
        ds = load_demonstrations(reps, frame_skip=fs, observation_keys=KEYS, n_envs=n_rep)
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
    periods = int((L // fs).max())
    out = {"frame_skip": fs, "replays": n_rep, "levels": len(player.levels), "rows": player.rows_total, "ticks": int(L.sum()),
           "periods": periods, "ms": ms, "demo_ms": float(np.median(ms["demo"])), "baseline_ms": float(np.median(ms["baseline"])),
           "demo_us_per_period": float(np.median(ms["demo"]) * 1e3 / periods),
           "baseline_us_per_period": float(np.median(ms["baseline"]) * 1e3 / periods),
           "load_demonstrations_wall_ms": wall, "rows_equal_the_baseline": bool(same), "dataset_rows": len(ds)}
    print(json.dumps(out), flush=True)
    results.append(out)
    player.close()
    base.b.close()

if results:
    with open(os.path.join(ROOT, "profiles", "demo_cost.json"), "w") as f:
        json.dump(results, f, indent=1)
