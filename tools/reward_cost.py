"""Speed figures of reward mode "pbrs" for DESIGN.md 20, at 8192 envs on the headline level set ("c0") and on the locked-door set
("doors"): the step launch alone, the step with the reward launch behind it, and the step with the reward and the reachability
launches behind it, as HIP-event times over 200-step windows, alternating; medians.  Writes profiles/reward_cost.json and prints
one JSON line per set.

    python tools/reward_cost.py
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/reward_cost.py --trace c0
                                    # kernel durations: one warm run with all three launches per step on one set
"""
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nclone_amd import _native as nat  # noqa: E402
from nclone_amd import levels as level_sets  # noqa: E402
from nclone_amd.engine import NppBatch  # noqa: E402

TRACE = sys.argv[sys.argv.index("--trace") + 1] if "--trace" in sys.argv else None
n, W, K, ROUNDS = 8192, (300 if TRACE else 1300), 200, (1 if TRACE else 3)
SETS = {"c0": level_sets.curriculum0_levels, "doors": level_sets.door_levels}
rng = np.random.default_rng(0)
acts = torch.from_numpy(rng.integers(0, 6, size=(W + 3 * ROUNDS * K, n)).astype(np.uint8)).cuda()
lib = nat.lib()


def accepted(m):
    """the mode takes the level (npp_reachability does, and the reference's own level constants are finite)"""
    m = np.ascontiguousarray(m, dtype=np.float64)
    out = np.zeros(3)
    return lib.npp_reward_level_constants_host(m.ctypes.data_as(C.POINTER(C.c_double)), m.size, out.ctypes.data_as(C.c_void_p), None) == 0


results = []
for name, fn in SETS.items():
    if TRACE and name != TRACE:
        continue
    every = fn()[0]
    levels = [m for m in every if accepted(m)]
    out = {"set": name, "levels": len(levels), "levels_refused": len(every) - len(levels), "envs": n}

    def make(pbrs, outputs):
        b = NppBatch(n, autoreset=True, outputs=outputs)
        b.load_levels(levels)
        b.assign_levels((np.arange(n) // 64) % len(levels))
        b.reset()
        if pbrs:
            b.set_reward_mode("pbrs")
        return b

    status = torch.zeros(n, dtype=torch.int32, device="cuda")
    if TRACE:   # one batch, every launch per step: the trace then holds the three kernels over the same states
        b = make(True, ["work", "reward_components", "reachability_features", "mine_sdf_features"])
        kinds = np.zeros(4, dtype=np.int64)
        for k in range(W + K):
            b.step(acts[k], 4, want_terminal=False)
            b.step_reward(status_out=status if k >= W else None)
            b.reachability()
            if k >= W:
                kinds += np.bincount(status.cpu().numpy(), minlength=4)
        b.sync()
        out["branch_share"] = dict(zip(("miss", "hit", "hit_no_hop", "terminal"), (kinds / kinds.sum()).tolist()))
        print(json.dumps(out), flush=True)
        continue
    batches = {"step": make(False, ["work"]), "reward": make(True, ["work", "reward_components"]),
               "reward_reach": make(True, ["work", "reward_components", "reachability_features", "mine_sdf_features"])}

    def reward_reach(b):
        b.step_reward()
        b.reachability()

    after = {"step": lambda b: None, "reward": lambda b: b.step_reward(), "reward_reach": reward_reach}
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
    out["reward_us"] = float(np.median(us["reward"]) - np.median(us["step"]))
    out["reward_and_reachability_us"] = float(np.median(us["reward_reach"]) - np.median(us["step"]))
    out["env_steps_per_s"] = {k: n / (np.median(v) * 1e-6) for k, v in us.items()}
    batches["reward"].step(acts[0], 4, want_terminal=False)
    batches["reward"].step_reward(status_out=status)
    kinds = np.bincount(status.cpu().numpy(), minlength=4)
    out["branch_share"] = dict(zip(("miss", "hit", "hit_no_hop", "terminal"), (kinds / kinds.sum()).tolist()))
    for b in batches.values():
        b.close()
    print(json.dumps(out), flush=True)
    results.append(out)

if results:
    with open(os.path.join(ROOT, "profiles", "reward_cost.json"), "w") as f:
        json.dump(results, f, indent=1)
