"""Speed figures of path-direction action masking for DESIGN.md 19, at 8192 envs on the headline level set ("c0") and on the
locked-door set ("doors"): the step launch alone, the step with the path-mask launch behind it (mode hard), and the step with the
reachability launch behind it, as HIP-event times over 200-step windows, alternating.  Prints one JSON line per set.

    python tools/path_mask_cost.py
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/path_mask_cost.py --trace c0
                                    # kernel durations: one warm run with all three launches per step on one set
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nclone_amd import levels as level_sets  # noqa: E402
from nclone_amd.engine import NppBatch, reach_level_info  # noqa: E402

TRACE = sys.argv[sys.argv.index("--trace") + 1] if "--trace" in sys.argv else None
n, W, K, ROUNDS = 8192, (300 if TRACE else 1300), 200, (1 if TRACE else 3)
SETS = {"c0": level_sets.curriculum0_levels, "doors": level_sets.door_levels}
rng = np.random.default_rng(0)
acts = torch.from_numpy(rng.integers(0, 6, size=(W + 3 * ROUNDS * K, n)).astype(np.uint8)).cuda()

for name, fn in SETS.items():
    if TRACE and name != TRACE:
        continue
    levels = [m for m in fn()[0] if reach_level_info(m)["supported"]]   # (both launches refuse levels with several exit switches)
    out = {"set": name, "levels": len(levels), "envs": n}

    def make(mode, outputs):
        b = NppBatch(n, autoreset=True, outputs=outputs)
        b.load_levels(levels)
        b.assign_levels((np.arange(n) // 64) % len(levels))
        if mode:
            b.set_action_masking(mode)
        return b

    if TRACE:   # one batch, every launch per step: the trace then holds the three kernels over the same states
        b = make("hard", ["work", "path_direction", "reachability_features", "mine_sdf_features"])
        for k in range(W + K):
            b.step(acts[k], 4, want_terminal=False)
            b.reachability()
            b.path_action_mask()
        b.sync()
        st = {k: v.cpu().numpy() for k, v in b.path_mask_stats().items()}
        out["applied_share"] = float(st["applied"].sum() + st["last_applied"].sum()) / float(st["observed"].sum() + st["last_observed"].sum())
        print(json.dumps(out), flush=True)
        continue
    batches = {"step": make(None, ["work"]), "hard": make("hard", ["work", "path_direction"]),
               "reach": make(None, ["work", "reachability_features", "mine_sdf_features"])}
    after = {"step": lambda b: None, "hard": lambda b: b.path_action_mask(), "reach": lambda b: b.reachability()}
    for key, b in batches.items():
        for k in range(W):
            b.step(acts[k], 4, want_terminal=False)
            after[key](b)
        b.sync()
    us = {k: [] for k in batches}
    k0 = W
    for r in range(ROUNDS):
        order = list(batches) if r % 2 == 0 else list(batches)[::-1]
        for key in order:
            b = batches[key]
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record(b.stream)
            for k in range(K):
                b.step(acts[k0 + k], 4, want_terminal=False)
                after[key](b)
            e1.record(b.stream)
            torch.cuda.synchronize()
            us[key].append(e0.elapsed_time(e1) * 1e3 / K)
            k0 += K
    out["us_per_step"] = us
    out["path_mask_us"] = float(np.median(us["hard"]) - np.median(us["step"]))
    out["reachability_us"] = float(np.median(us["reach"]) - np.median(us["step"]))
    out["env_steps_per_s"] = {k: n / (np.median(v) * 1e-6) for k, v in us.items()}
    st = {k: v.cpu().numpy() for k, v in batches["hard"].path_mask_stats().items()}
    out["applied_share"] = float(st["applied"].sum() + st["last_applied"].sum()) / float(st["observed"].sum() + st["last_observed"].sum())
    for b in batches.values():
        b.close()
    print(json.dumps(out), flush=True)
