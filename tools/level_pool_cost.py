#!/usr/bin/env python3
"""Cost of the level pool per step: 8192 envs on the 512-level mixed set (c3), auto-reset, HIP events around every
npp_step.  Modes, alternated `reps` times on fresh handles in one run:
    fixed    every 64-env block on one level ((i // 64) % 512): NppVecEnvironment's default assignment, LDS-staged; at 8192 envs it
             covers levels 0..127 only (curriculum 0)
    fixed16  every 16-env block (one workgroup at 16 lanes per env) on one level ((i // 16) % 512): all 512 levels, still LDS-staged
    pool     the level pool with uniform weights over the 512 levels (a new level at every episode end; LDS staging off)

    python3 tools/level_pool_cost.py [--envs 8192] [--steps 300] [--warmup 50] [--reps 3] [--variant 1] [--trunc dynamic]
    python3 tools/level_pool_cost.py --trace DIR      # summarise a rocprofv3 --kernel-trace run of `--mode pool`

The step kernel's build variant is pinned (--variant; -1 = autotune) so that both modes run the same build.  --trace reads the
kernel_trace.csv files under DIR and reports, per draw launch, the draw kernel, the masked reset and the masked observe (the step
kernel launch that follows them) -- the redraw launches alone.  Prints one JSON line.
"""
import argparse
import csv
import glob
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def run(mode, n, steps, warmup, variant, trunc):
    from nclone_amd.engine import NppBatch
    from nclone_amd.levels import c3_mixed_levels

    levels, _ = c3_mixed_levels()
    b = NppBatch(n, autoreset=True, fast_reset=True)
    b.load_levels(levels)
    b.assign_levels((np.arange(n) // (16 if mode == "fixed16" else 64)) % len(levels))
    if trunc == "dynamic":
        b.set_dynamic_truncation(True)
    else:
        b.set_truncation_limit(int(trunc))
    b.set_step_variant(variant)
    if mode == "pool":
        b.set_level_pool(np.ones(len(levels)), seed=1)
        b.draw_levels()
    b.reset()
    acts = torch.from_numpy(np.random.default_rng(0).integers(0, 6, size=(warmup + steps, n)).astype(np.uint8)).to(b.device)
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(2)] for _ in range(steps)]
    ended = torch.zeros((), dtype=torch.int64, device=b.device)
    for s in range(warmup + steps):
        t = s - warmup
        if t >= 0:
            ev[t][0].record(b.stream)
        b.step(acts[s], 4, want_terminal=True)
        if t >= 0:
            ev[t][1].record(b.stream)
            with torch.cuda.stream(b.stream):
                ended += ((b.flags & 11) != 0).sum()
    torch.cuda.synchronize()
    us = np.array([ev[t][0].elapsed_time(ev[t][1]) * 1e3 for t in range(steps)])
    out = {"mean_us": round(float(us.mean()), 2), "p50_us": round(float(np.median(us)), 2),
           "resets_per_step": round(float(ended.item()) / steps, 1), "variant": b.step_variant()[0]}
    b.close()
    return out


def trace(d):
    rows = []
    for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        with open(f) as fh:
            rows += list(csv.DictReader(fh))
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    draw, reset, obs, step = [], [], [], []
    for i, r in enumerate(rows):
        if "npp_pool_draw_kernel" not in r["Kernel_Name"]:
            continue
        nxt = rows[i + 1:i + 3]
        if len(nxt) < 2 or "npp_reset_kernel" not in nxt[0]["Kernel_Name"] or "npp_step_kernel" not in nxt[1]["Kernel_Name"]:
            continue
        dur = [(int(x["End_Timestamp"]) - int(x["Start_Timestamp"])) / 1e3 for x in (r, nxt[0], nxt[1])]
        draw.append(dur[0]); reset.append(dur[1]); obs.append(dur[2])
        if i > 0 and "npp_step_kernel" in rows[i - 1]["Kernel_Name"]:
            step.append((int(rows[i - 1]["End_Timestamp"]) - int(rows[i - 1]["Start_Timestamp"])) / 1e3)
    m = lambda v: round(float(np.mean(v)), 2) if v else None  # noqa: E731
    return {"redraws": len(draw), "draw_us": m(draw), "masked_reset_us": m(reset), "masked_observe_us": m(obs),
            "redraw_total_us": m([a + b + c for a, b, c in zip(draw, reset, obs)]), "step_kernel_us": m(step)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=8192)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--variant", type=int, default=1)
    ap.add_argument("--trunc", default="dynamic")
    ap.add_argument("--mode", default="all", choices=["all", "fixed", "fixed16", "pool"])
    ap.add_argument("--trace", default=None)
    a = ap.parse_args()
    if a.trace:
        print(json.dumps({"tool": "level_pool_cost", "trace": trace(a.trace)}))
        return
    modes = ["fixed", "fixed16", "pool"] if a.mode == "all" else [a.mode]
    res = {m: [] for m in modes}
    for _ in range(a.reps):
        for m in modes:
            res[m].append(run(m, a.envs, a.steps, a.warmup, a.variant, a.trunc))
    summary = {m: {"mean_us": round(float(np.mean([r["mean_us"] for r in v])), 2), "runs": v} for m, v in res.items()}
    if len(modes) == 3:
        summary["ratio_pool_over_fixed"] = round(summary["pool"]["mean_us"] / summary["fixed"]["mean_us"], 3)
        summary["ratio_pool_over_fixed16"] = round(summary["pool"]["mean_us"] / summary["fixed16"]["mean_us"], 3)
    print(json.dumps({"tool": "level_pool_cost", "envs": a.envs, "steps": a.steps, "warmup": a.warmup, "trunc": a.trunc,
                      "variant": a.variant, **summary}))


if __name__ == "__main__":
    main()
