#!/usr/bin/env python3
"""Cost of the minimal observation mode per step: 8192 envs, auto-reset with fast reset, on the mine set and on
the 21 locked-door levels, three modes, mean us per step from HIP events around every step:

    plain    npp_step with the packed block only (no secondary observation)
    minimal  minimal mode: npp_step (spatial_context rows into the handle's buffer) + npp_minimal_observation
    full     the full-mode way to the same information: npp_step with spatial_context + npp_reachability
             (only entry points that exist without the minimal mode.  To time it on the code of a commit without the mode, copy
             this file into a checkout of that commit with its own library built and run it there with --modes plain,full: this
             tree's binding needs the two new symbols, so NPP_AMD_LIB=<an older library> does not load here)

    python3 tools/minimal_obs_cost.py [--envs 8192] [--steps 300] [--warmup 50] [--reps 3] [--modes plain,minimal,full] [--host]

The step kernel's build variant is pinned (1) in every mode; the modes alternate `reps` times on fresh handles, so the spread of
one mode over its repetitions is reported beside the means.  --host adds, per mode, the time of one step INCLUDING the copy of
what a numpy consumer needs to the host (to_host: one pinned copy + one synchronisation), from a host clock around synchronised
steps.  Prints one JSON line.
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
from nclone_amd.levels import door_levels, mine_levels  # noqa: E402

OUTPUTS = {"plain": (), "minimal": ("minimal_observation",), "full": ("spatial_context", "reachability_features", "mine_sdf_features")}
HOST = {"plain": ("action_mask", "flags", "reward", "frames"),
        "minimal": ("action_mask", "flags", "reward", "frames", "minimal_observation"),
        "full": ("game_state", "action_mask", "flags", "reward", "frames", "spatial_context", "reachability_features", "mine_sdf_features")}


def observe(b, mode):
    if mode == "minimal":
        b.minimal_observation()
    elif mode == "full":
        b.reachability()


def run(setup, mode, n, steps, warmup, variant, host):
    levels = mine_levels()[0] if setup == "mines" else door_levels()[0]
    b = NppBatch(n, autoreset=True, fast_reset=True, outputs=OUTPUTS[mode])
    b.load_levels(levels)
    b.assign_levels((np.arange(n) // 64) % len(levels))
    b.set_step_variant(variant)
    b.reset()
    b.observe()
    observe(b, mode)   # tables built
    acts = torch.from_numpy(np.random.default_rng(0).integers(0, 6, size=(warmup + steps, n)).astype(np.uint8)).to(b.device)
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(3)] for _ in range(steps)]
    for s in range(warmup + steps):
        t = s - warmup
        if t >= 0:
            ev[t][0].record(b.stream)
        b.step(acts[s], 4, want_terminal=True)
        if t >= 0:
            ev[t][1].record(b.stream)
        observe(b, mode)
        if t >= 0:
            ev[t][2].record(b.stream)
    torch.cuda.synchronize()
    tot = [ev[t][0].elapsed_time(ev[t][2]) * 1e3 for t in range(steps)]
    obs = [ev[t][1].elapsed_time(ev[t][2]) * 1e3 for t in range(steps)]
    out = {"setup": setup, "mode": mode, "step_total_us": float(np.mean(tot)), "step_median_us": float(np.median(tot)),
           "obs_call_us": float(np.mean(obs))}
    if host:
        k = min(steps, 100)
        t0 = time.perf_counter()
        for s in range(k):
            b.step(acts[warmup + s], 4, want_terminal=True)
            observe(b, mode)
            b.to_host(HOST[mode])
        out["step_with_host_copy_us"] = (time.perf_counter() - t0) * 1e6 / k
        out["host_bytes_per_env"] = int(sum(b.out.offsets[f][1] for f in HOST[mode]) // n)
    b.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=8192)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--variant", type=int, default=1)
    ap.add_argument("--modes", default="plain,minimal,full")
    ap.add_argument("--setup", default="both", choices=["both", "mines", "doors"])
    ap.add_argument("--host", action="store_true")
    a = ap.parse_args()
    modes = a.modes.split(",")
    assert all(m in OUTPUTS for m in modes)
    setups = ["mines", "doors"] if a.setup == "both" else [a.setup]
    runs = [run(s, m, a.envs, a.steps, a.warmup, a.variant, a.host) for s in setups for _ in range(a.reps) for m in modes]
    out = {"envs": a.envs, "steps": a.steps, "reps": a.reps, "lib": os.environ.get("NPP_AMD_LIB", "in-tree"), "runs": runs}
    for s in setups:
        for m in modes:
            v = [r["step_total_us"] for r in runs if r["setup"] == s and r["mode"] == m]
            out["%s_%s_us" % (s, m)] = float(np.mean(v))
            out["%s_%s_spread_us" % (s, m)] = float(max(v) - min(v))
            out["%s_%s_obs_call_us" % (s, m)] = float(np.mean([r["obs_call_us"] for r in runs if r["setup"] == s and r["mode"] == m]))
            if a.host:
                out["%s_%s_with_host_copy_us" % (s, m)] = float(np.mean([r["step_with_host_copy_us"] for r in runs
                                                                        if r["setup"] == s and r["mode"] == m]))
        if "minimal" in modes and "full" in modes:
            out["%s_minimal_minus_full_us" % s] = out["%s_minimal_us" % s] - out["%s_full_us" % s]
        if "minimal" in modes and "plain" in modes:
            out["%s_minimal_minus_plain_us" % s] = out["%s_minimal_us" % s] - out["%s_plain_us" % s]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
