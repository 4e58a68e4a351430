#!/usr/bin/env python3
"""Cost of the graph observations per step: 8192 envs, auto-reset, graph observations off against on, mean us
per step from HIP events around every step, in two setups:

    fixed  config 2's level set (curriculum 0), the fixed assignment: no env ever changes level, so the graph call is the
           steady state (one launch that rewrites nothing)
    pool   c3_mixed_levels with the level pool (uniform weights, truncation at 60 frames so that episodes end often): the envs
           that draw another level get their rows rewritten

    python3 tools/graph_obs_cost.py [--envs 8192] [--steps 300] [--warmup 50] [--reps 3] [--setup both|fixed|pool]

off: npp_step.  on: npp_step + npp_graph_observation.  The step kernel's build variant is pinned (1) in both; modes alternate
`reps` times on fresh handles.  Also times 10 rewrite-all calls (every row written: 162.5 KB per env) per "on" run.  Prints one
JSON line.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from nclone_amd.engine import NppBatch  # noqa: E402
from nclone_amd.levels import c3_mixed_levels, curriculum0_levels  # noqa: E402

ROW_BYTES = 60000 + 80000 + 2500 + 20000


def run(setup, mode, n, steps, warmup, variant):
    levels = curriculum0_levels()[0] if setup == "fixed" else c3_mixed_levels()[0]
    b = NppBatch(n, autoreset=True, fast_reset=True)
    b.load_levels(levels)
    b.assign_levels((np.arange(n) // 64) % len(levels))
    b.set_step_variant(variant)
    if setup == "pool":
        b.set_truncation_limit(60)
        b.set_level_pool(np.ones(len(levels)), seed=1)
    b.reset()
    if mode == "on":
        b.graph_observation()   # tables built, every row written once
    acts = torch.from_numpy(np.random.default_rng(0).integers(0, 6, size=(warmup + steps, n)).astype(np.uint8)).to(b.device)
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(steps)]
    changed = 0
    lv = b.env_levels() if setup == "pool" else None
    for s in range(warmup + steps):
        t = s - warmup
        if t >= 0:
            ev[t][0].record(b.stream)
        b.step(acts[s], 4, want_terminal=True)
        if t >= 0:
            ev[t][1].record(b.stream)
        if mode == "on":
            b.graph_observation()
        if t >= 0:
            ev[t][2].record(b.stream)
        if setup == "pool" and t >= 0 and t % 50 == 0:   # (synchronises: outside the timed stretch of this step)
            now = b.env_levels()
            changed += int((now != lv).sum())
            lv = now
    torch.cuda.synchronize()
    tot = [ev[t][0].elapsed_time(ev[t][2]) * 1e3 for t in range(steps)]
    graph = [ev[t][1].elapsed_time(ev[t][2]) * 1e3 for t in range(steps)]
    out = {"setup": setup, "mode": mode, "step_total_us": float(np.mean(tot)), "graph_us": float(np.mean(graph)) if mode == "on" else 0.0}
    if mode == "on":
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(b.stream)
        for _ in range(10):
            b.graph_observation(rewrite_all=True)
        e1.record(b.stream)
        torch.cuda.synchronize()
        us = e0.elapsed_time(e1) * 1e3 / 10
        out["rewrite_all_us"] = us
        out["rewrite_all_tb_s"] = n * ROW_BYTES / (us * 1e-6) / 1e12
    if setup == "pool":
        out["level_changes_sampled"] = changed
    b.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=8192)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--variant", type=int, default=1)
    ap.add_argument("--setup", default="both", choices=["both", "fixed", "pool"])
    a = ap.parse_args()
    setups = ["fixed", "pool"] if a.setup == "both" else [a.setup]
    runs = [run(s, m, a.envs, a.steps, a.warmup, a.variant) for s in setups for _ in range(a.reps) for m in ("off", "on")]
    out = {"envs": a.envs, "steps": a.steps, "row_bytes_per_env": ROW_BYTES, "runs": runs}
    for s in setups:
        for m in ("off", "on"):
            out["%s_%s_us" % (s, m)] = float(np.mean([r["step_total_us"] for r in runs if r["setup"] == s and r["mode"] == m]))
        out["%s_delta_us" % s] = out["%s_on_us" % s] - out["%s_off_us" % s]
        out["%s_graph_us" % s] = float(np.mean([r["graph_us"] for r in runs if r["setup"] == s and r["mode"] == "on"]))
        out["%s_rewrite_all_us" % s] = float(np.mean([r["rewrite_all_us"] for r in runs if r["setup"] == s and r["mode"] == "on"]))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
