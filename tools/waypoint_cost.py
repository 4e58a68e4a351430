"""Speed figures of the sequential path waypoints of reward mode "pbrs" for DESIGN.md 23, at 8192 envs on the headline level set
("c0") and on the locked-door set ("doors"): the step launch alone, the step with the reward launch behind it, and the step with the
waypoint and the reward launches behind it, as HIP-event times over 200-step windows, three alternating windows per variant; medians.
Writes profiles/waypoint_cost.json (or --out PATH) and prints one JSON line per set.

    python tools/waypoint_cost.py [--out PATH] [--label TEXT]
    python tools/waypoint_cost.py --no-waypoints --label parent     # a build without the option (the parent commit's tree): the
                                    # first two variants only, for the "+ reward" figure of both builds taken in one session
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/waypoint_cost.py --trace c0
                                    # kernel durations: one warm run with both launches per step on one set
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


def _arg(name, default=None):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


TRACE = _arg("--trace")
WAYPOINTS = "--no-waypoints" not in sys.argv
n, W, K, ROUNDS = 8192, (300 if TRACE else 1300), 200, (1 if TRACE else 3)
SETS = {"c0": level_sets.curriculum0_levels, "doors": level_sets.door_levels}
VARIANTS = ("step", "reward", "waypoints") if WAYPOINTS else ("step", "reward")
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
    out = {"set": name, "label": _arg("--label", "this"), "levels": len(levels), "levels_refused": len(every) - len(levels), "envs": n}

    def make(variant):
        b = NppBatch(n, autoreset=True, outputs=["work"] if variant == "step" else ["work", "reward_components"])
        b.load_levels(levels)
        b.assign_levels((np.arange(n) // 64) % len(levels))
        b.reset()
        if variant != "step":
            b.set_reward_mode("pbrs")
        if variant == "waypoints":
            b.set_reward_waypoints(True)
        return b

    info = torch.zeros((n, 3), dtype=torch.int32, device="cuda")
    if TRACE:   # one batch, both launches per step: the trace then holds the two kernels over the same states
        b = make("waypoints")
        collected = 0
        for k in range(W + K):
            b.step(acts[k], 4, want_terminal=False)
            b.step_reward(wp_info_out=info if k >= W else None)
            if k >= W:
                collected += int((info[:, 0] >= 0).sum())
        b.sync()
        out["collections_per_env_step"] = collected / (K * n)
        out["waypoints_per_level"] = [len(b.level_waypoints(i)[0]) for i in range(len(levels))]
        print(json.dumps(out), flush=True)
        continue
    batches = {v: make(v) for v in VARIANTS}
    after = {"step": lambda b: None, "reward": lambda b: b.step_reward(), "waypoints": lambda b: b.step_reward()}
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
    if WAYPOINTS:
        out["waypoints_us"] = float(np.median(us["waypoints"]) - np.median(us["reward"]))
        b = batches["waypoints"]
        b.step(acts[0], 4, want_terminal=False)
        b.step_reward(wp_info_out=info)
        out["collections_per_env_step"] = float((info[:, 0] >= 0).sum()) / n
        wl = [len(b.level_waypoints(i)[0]) for i in range(len(levels))]
        out["waypoints_per_level"] = {"min": int(min(wl)), "median": float(np.median(wl)), "max": int(max(wl))}
    out["env_steps_per_s"] = {k: n / (np.median(v) * 1e-6) for k, v in us.items()}
    for b in batches.values():
        b.close()
    print(json.dumps(out), flush=True)
    results.append(out)

if results:
    with open(_arg("--out", os.path.join(ROOT, "profiles", "waypoint_cost.json")), "w") as f:
        json.dump(results, f, indent=1)
