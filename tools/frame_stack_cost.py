#!/usr/bin/env python3
"""Cost of frame stacking per step: config 3's set (mines, 8192 envs, auto-reset, player_frame every step),
stacking off against visual K and state K on, mean us per step from HIP events around every step.

    python3 tools/frame_stack_cost.py [--envs 8192] [--k 4] [--steps 300] [--warmup 50] [--reps 3] [--mode both|off|on]

off: npp_step + npp_render_player_frame.  on: npp_step + npp_frame_stack_render + npp_frame_stack_push (with the terminal
stack).  The step kernel's build variant is pinned (1) in both, so the autotuner cannot pick differently between the runs;
modes alternate `reps` times on fresh handles.  Prints one JSON line.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from nclone_amd.engine import NppBatch  # noqa: E402
from nclone_amd.levels import mine_levels  # noqa: E402


def run(mode, n, k, steps, warmup, variant):
    levels, _ = mine_levels()
    b = NppBatch(n, autoreset=True, fast_reset=True, outputs=["player_frame"])
    b.load_levels(levels)
    b.assign_levels((np.arange(n) // 64) % len(levels))
    b.set_step_variant(variant)
    term = None
    if mode == "on":
        b.set_frame_stack(k, k, "zero")
        term = torch.zeros((n, k, 41), dtype=torch.float32, device=b.device)
    b.reset()
    acts = torch.from_numpy(np.random.default_rng(0).integers(0, 6, size=(warmup + steps, n)).astype(np.uint8)).to(b.device)
    mids = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(steps)]
    ends = [torch.cuda.Event(enable_timing=True) for _ in range(steps)]
    for s in range(warmup + steps):
        t = s - warmup
        if t >= 0:
            mids[t][0].record(b.stream)
        b.step(acts[s], 4, want_terminal=True)
        if t >= 0:
            mids[t][1].record(b.stream)
        if mode == "on":
            b.render_player_frame_stacked()
            if t >= 0:
                mids[t][2].record(b.stream)
            b.frame_stack_push(11, False, term)
        else:
            b.render_player_frame()
            if t >= 0:
                mids[t][2].record(b.stream)
        if t >= 0:
            ends[t].record(b.stream)
    torch.cuda.synchronize()
    tot = [mids[t][0].elapsed_time(ends[t]) * 1e3 for t in range(steps)]
    stp = [mids[t][0].elapsed_time(mids[t][1]) * 1e3 for t in range(steps)]
    ren = [mids[t][1].elapsed_time(mids[t][2]) * 1e3 for t in range(steps)]
    push = [mids[t][2].elapsed_time(ends[t]) * 1e3 for t in range(steps)]
    flags = b.flags.cpu().numpy()
    b.close()
    return {"mode": mode, "step_total_us": float(np.mean(tot)), "step_kernel_us": float(np.mean(stp)),
            "player_frame_us": float(np.mean(ren)), "push_us": float(np.mean(push)) if mode == "on" else 0.0,
            "resets_last_step": int(((flags & 11) != 0).sum())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=8192)
    ap.add_argument("--k", type=int, default=4)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--variant", type=int, default=1)
    ap.add_argument("--mode", default="both", choices=["both", "off", "on"])
    a = ap.parse_args()
    modes = ["off", "on"] if a.mode == "both" else [a.mode]
    runs = [run(m, a.envs, a.k, a.steps, a.warmup, a.variant) for _ in range(a.reps) for m in modes]
    out = {"envs": a.envs, "k_visual": a.k, "k_state": a.k, "steps": a.steps, "runs": runs}
    for m in modes:
        out["mean_" + m + "_us"] = float(np.mean([r["step_total_us"] for r in runs if r["mode"] == m]))
    if len(modes) == 2:
        out["delta_us"] = out["mean_on_us"] - out["mean_off_us"]
    # bytes the stacking adds per step (no resets): the frame's mirror copy (the render writes 2 slots but for position 0), the
    # state ring (41 f32 read + 2 written), the terminal stack (K - 1 read + K written)
    n, k = a.envs, a.k
    out["extra_hbm_bytes_per_step"] = int(n * 7056 * (k - 1) / k + n * 41 * 4 * (3 + 2 * k - 1))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
