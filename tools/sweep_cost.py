#!/usr/bin/env python3
"""Cost of an evaluation sweep: 8192 envs on the 512-level mixed set (c3), auto-reset, episode statistics on and
accumulated behind every step, HIP events around every step + accumulation.  Modes, on fresh handles in one run:
    pool     the level pool with uniform weights over the 512 levels: the baseline the sweep is set beside (what users fall back on)
    sweep    a sweep of tile(arange(512), K) for every K of --k: the mean per-step time over the first --steps steps, then the tail --
             steps and wall time from the start to done == J, and the share of env-steps spent by envs without a job

    python3 tools/sweep_cost.py [--envs 8192] [--steps 300] [--warmup 50] [--k 1,2,3,4] [--variant 1] [--trunc dynamic]
    python3 tools/sweep_cost.py --mode sweep --k 4 --max-steps 400     # a short run to put under rocprofv3 --kernel-trace
    python3 tools/sweep_cost.py --trace DIR      # summarise the kernel_trace.csv files of such runs (sweep and pool)

The step kernel's build variant is pinned (--variant; -1 = autotune) so that both modes run the same build.  --trace reports the
mean duration of the assign and collect kernels, of the pool's draw kernel, of the episode kernel, and of the masked reset and masked
observe launches that follow an assign or a draw.  Prints one JSON line.
"""
import argparse
import csv
import glob
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def handle(n, variant, trunc):
    from nclone_amd.engine import NppBatch
    from nclone_amd.levels import c3_mixed_levels

    levels, _ = c3_mixed_levels()
    b = NppBatch(n, autoreset=True, fast_reset=True)
    b.load_levels(levels)
    b.assign_levels((np.arange(n) // 64) % len(levels))
    if trunc == "dynamic":
        b.set_dynamic_truncation(True)
    else:
        b.set_truncation_limit(int(trunc))
    b.set_step_variant(variant)
    b.set_episode_stats(True)
    return b, len(levels)


def timed_steps(b, acts, first, steps, warmup, each=None):
    """warmup untimed steps, then `steps` timed ones (step + accumulation between two events); -> per-step microseconds"""
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(2)] for _ in range(steps)]
    for s in range(warmup + steps):
        t = s - warmup
        if t >= 0:
            ev[t][0].record(b.stream)
        b.step(acts[(first + s) % len(acts)], 4, want_terminal=True)
        b.episode_accumulate()
        if t >= 0:
            ev[t][1].record(b.stream)
        if each is not None:
            each()
    torch.cuda.synchronize()
    return np.array([ev[t][0].elapsed_time(ev[t][1]) * 1e3 for t in range(steps)])


def run_pool(n, steps, warmup, variant, trunc):
    b, L = handle(n, variant, trunc)
    b.set_level_pool(np.ones(L), seed=1)
    b.draw_levels()
    b.reset()
    acts = torch.from_numpy(np.random.default_rng(0).integers(0, 6, size=(warmup + steps, n)).astype(np.uint8)).to(b.device)
    us = timed_steps(b, acts, 0, steps, warmup)
    out = {"mean_us": round(float(us.mean()), 2), "p50_us": round(float(np.median(us)), 2), "variant": b.step_variant()[0]}
    b.close()
    return out


def run_sweep(n, steps, warmup, variant, trunc, K, max_steps):
    b, L = handle(n, variant, trunc)
    J = L * K
    rows = 512
    acts = torch.from_numpy(np.random.default_rng(0).integers(0, 6, size=(rows, n)).astype(np.uint8)).to(b.device)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    b.sweep_start(np.tile(np.arange(L, dtype=np.int32), K))
    s = b.sweep_state()
    idle = torch.zeros((), dtype=torch.int64, device=b.device)

    def count_idle():
        nonlocal idle
        with torch.cuda.stream(b.stream):
            idle += (s["env_job"] < 0).sum()

    us = timed_steps(b, acts, 0, steps, warmup, each=count_idle)
    done_steps = warmup + steps
    done = int(s["counters"].cpu()[1])
    while done < J and (max_steps is None or done_steps < max_steps):
        for _ in range(16):
            b.step(acts[done_steps % rows], 4, want_terminal=True)
            b.episode_accumulate()
            count_idle()
            done_steps += 1
        with torch.cuda.stream(b.stream):
            done = int(s["counters"].cpu()[1])
    torch.cuda.synchronize()
    wall = time.perf_counter() - t0
    out = {"k": K, "jobs": J, "mean_us": round(float(us.mean()), 2), "p50_us": round(float(np.median(us)), 2), "done": done,
           "steps_to_done": done_steps, "wall_s": round(wall, 3), "idle_env_step_share": round(float(idle.item()) / (done_steps * n), 4),
           "variant": b.step_variant()[0]}
    b.close()
    return out


def trace(d):
    rows = []
    for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        with open(f) as fh:
            rows += list(csv.DictReader(fh))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    dur = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3  # noqa: E731
    m = lambda v: round(float(np.mean(v)), 2) if v else None  # noqa: E731
    by = {k: [] for k in ("npp_sweep_assign_kernel", "npp_sweep_collect_kernel", "npp_pool_draw_kernel", "npp_episode_kernel")}
    behind = {"npp_sweep_assign_kernel": ([], []), "npp_pool_draw_kernel": ([], [])}
    for i, r in enumerate(rows):
        for k in by:
            if k in r["Kernel_Name"]:
                by[k].append(dur(r))
        for k, (reset, obs) in behind.items():
            nxt = rows[i + 1:i + 3]
            if k in r["Kernel_Name"] and len(nxt) == 2 and "npp_reset_kernel" in nxt[0]["Kernel_Name"] and "npp_step_kernel" in nxt[1]["Kernel_Name"]:
                reset.append(dur(nxt[0]))
                obs.append(dur(nxt[1]))
    out = {k.replace("npp_", "").replace("_kernel", "") + "_us": m(v) for k, v in by.items()}
    out["launches"] = {k: len(v) for k, v in by.items()}
    for k, (reset, obs) in behind.items():
        tag = "sweep" if "sweep" in k else "pool"
        out[tag + "_masked_reset_us"], out[tag + "_masked_observe_us"] = m(reset), m(obs)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=8192)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--k", default="1,2,3,4")
    ap.add_argument("--variant", type=int, default=1)
    ap.add_argument("--trunc", default="dynamic")
    ap.add_argument("--mode", default="all", choices=["all", "pool", "sweep"])
    ap.add_argument("--max-steps", type=int, default=None)
    ap.add_argument("--trace", default=None)
    a = ap.parse_args()
    if a.trace:
        print(json.dumps({"tool": "sweep_cost", "trace": trace(a.trace)}))
        return
    out = {"tool": "sweep_cost", "envs": a.envs, "steps": a.steps, "warmup": a.warmup, "trunc": a.trunc, "variant": a.variant}
    if a.mode in ("all", "pool"):
        out["pool"] = run_pool(a.envs, a.steps, a.warmup, a.variant, a.trunc)
    if a.mode in ("all", "sweep"):
        out["sweep"] = [run_sweep(a.envs, a.steps, a.warmup, a.variant, a.trunc, int(k), a.max_steps) for k in a.k.split(",")]
    if a.mode == "all":
        out["pool_after"] = run_pool(a.envs, a.steps, a.warmup, a.variant, a.trunc)   # the spread of the baseline inside this run
    print(json.dumps(out))


if __name__ == "__main__":
    main()
