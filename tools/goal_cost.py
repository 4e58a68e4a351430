#!/usr/bin/env python3
"""Cost of the goal curriculum: per step at N envs on the headline level set, the mode off against the mode on, in
alternating windows of one process timed with HIP events; plus the set-up time of switching it on and the device memory the variant
levels take.

    python tools/goal_cost.py [--envs 8192] [--steps 200] [--windows 3] [--out profiles/goal_cost.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from nclone_amd.engine import NppBatch  # noqa: E402
from nclone_amd.levels import curriculum0_levels  # noqa: E402


def window(b, actions, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for k in range(steps):
        b.step(actions[k % len(actions)], want_terminal=False)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1000.0 / steps   # microseconds per step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=8192)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    levels = curriculum0_levels()[0]
    b = NppBatch(a.envs, autoreset=True)
    b.load_levels(levels)
    ids = (np.arange(a.envs) // 64) % len(levels)
    b.assign_levels(ids)
    rng = np.random.default_rng(0)
    actions = torch.from_numpy(rng.integers(0, 6, size=(64, a.envs)).astype(np.uint8)).cuda()
    res = {"envs": a.envs, "levels": len(levels), "steps_per_window": a.steps, "off_us": [], "on_us": [], "setup_s": [], "variant_bytes": []}
    window(b, actions, a.steps)   # warm-up (the step variant autotuner settles)
    window(b, actions, a.steps)
    for _ in range(a.windows):
        res["off_us"].append(window(b, actions, a.steps))
        torch.cuda.synchronize()
        free0 = torch.cuda.mem_get_info()[0]
        t0 = time.perf_counter()
        b.set_goal_curriculum(True)
        torch.cuda.synchronize()
        res["setup_s"].append(time.perf_counter() - t0)
        res["variant_bytes"].append(int(free0 - torch.cuda.mem_get_info()[0]))
        res["n_levels_on"] = b.n_levels
        window(b, actions, a.steps)   # (a new level set restarts the autotuner)
        window(b, actions, a.steps)
        res["on_us"].append(window(b, actions, a.steps))
        lv = b.goal_views()["level_words"].cpu().numpy()
        res["advances"] = int(lv[7].sum())
        res["appended"] = int(lv[8].sum())
        b.set_goal_curriculum(False)
        b.assign_levels(ids)
        window(b, actions, a.steps)
        window(b, actions, a.steps)
    res["off_median_us"] = float(np.median(res["off_us"]))
    res["on_median_us"] = float(np.median(res["on_us"]))
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
