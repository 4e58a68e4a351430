"""Speed figures of the episode statistics for DESIGN.md 24, at 8192 envs on the headline level set ("c0") and on the locked-door set
("doors"): the step launch alone, the step with the accumulation behind it, and the same with the six component planes, as HIP-event
times over 200-step windows, three alternating windows per variant; medians.  Then the accumulation launch alone on synthetic rows:
no env ends, every env ends with the levels spread wavefront by wavefront, every env ends with the levels mixed inside each
wavefront, every env ends on one level (the worst case for the table's atomics).
Writes profiles/episode_cost.json (or --out PATH) and prints one JSON line per set.

    python tools/episode_cost.py [--out PATH] [--label TEXT]
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/episode_cost.py --trace c0
                                    # kernel durations: one warm run with the accumulation (with components) behind every step
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from nclone_amd import levels as level_sets  # noqa: E402
from nclone_amd.engine import NppBatch  # noqa: E402


def _arg(name, default=None):
    return sys.argv[sys.argv.index(name) + 1] if name in sys.argv else default


TRACE = _arg("--trace")
n, W, K, ROUNDS = 8192, (300 if TRACE else 1300), 200, (1 if TRACE else 3)
SETS = {"c0": level_sets.curriculum0_levels, "doors": level_sets.door_levels}
VARIANTS = ("step", "episode", "episode_components")
rng = np.random.default_rng(0)
acts = torch.from_numpy(rng.integers(0, 6, size=(W + 3 * ROUNDS * K, n)).astype(np.uint8)).cuda()
comps = torch.zeros((n, 6), dtype=torch.float32, device="cuda")   # (the kernel's traffic does not depend on the values)


def timed(stream, fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record(stream)
    for k in range(reps):
        fn(k)
    e1.record(stream)
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


results = []
for name, fn in SETS.items():
    if TRACE and name != TRACE:
        continue
    levels = fn()[0]
    out = {"set": name, "label": _arg("--label", "this"), "levels": len(levels), "envs": n}

    def make(variant):
        b = NppBatch(n, autoreset=True, outputs=["work"])
        b.load_levels(levels)
        b.assign_levels((np.arange(n) // 64) % len(levels))
        if variant != "step":
            b.set_episode_stats(True)
        b.reset()
        return b

    after = {"step": lambda b: None, "episode": lambda b: b.episode_accumulate(),
             "episode_components": lambda b: b.episode_accumulate(components=comps)}
    if TRACE:
        b = make("episode_components")
        for k in range(W + K):
            b.step(acts[k], 4, want_terminal=False)
            b.episode_accumulate(components=comps)
        b.sync()
        out["episodes"] = int(b.episode_level_table()[:, 0].sum())
        print(json.dumps(out), flush=True)
        continue
    batches = {v: make(v) for v in VARIANTS}
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

            def one(k, b=b, key=key):
                b.step(acts[k0 + k], 4, want_terminal=False)
                after[key](b)

            us[key].append(timed(b.stream, one, K))
            k0 += K
    out["us_per_step"] = us
    out["episode_us"] = float(np.median(us["episode"]) - np.median(us["step"]))
    out["episode_components_us"] = float(np.median(us["episode_components"]) - np.median(us["step"]))
    out["env_steps_per_s"] = {k: n / (np.median(v) * 1e-6) for k, v in us.items()}
    b = batches["episode"]
    out["episodes_per_step"] = float(b.episode_level_table()[:, 0].sum()) / (W + ROUNDS * K)
    # the launch alone, on rows of the tool's own: frames 4 everywhere; flags 0, or NPP_F_DEAD for every env
    frames = torch.full((n,), 4, dtype=torch.int16, device="cuda")
    reward = torch.zeros(n, dtype=torch.float32, device="cuda")
    quiet, dead = torch.zeros(n, dtype=torch.uint8, device="cuda"), torch.full((n,), 2, dtype=torch.uint8, device="cuda")
    alone = {}
    for tag, flags, assign in (("no_end", quiet, None), ("all_end_spread", dead, None), ("all_end_mixed", dead, np.arange(n) % len(levels)),
                               ("all_end_one_level", dead, np.zeros(n))):
        if assign is not None:   # spread: 64 consecutive envs per level (wave-uniform); mixed: consecutive envs on consecutive levels
            b.assign_levels(assign.astype(np.int32))
        for c, cname in ((None, ""), (comps, "_components")):
            def call(k, flags=flags, c=c):
                b.episode_accumulate(flags, frames, reward, components=c)

            timed(b.stream, call, 20)
            alone[tag + cname] = sorted(timed(b.stream, call, K) for _ in range(3))[1]
    out["accumulate_alone_us"] = alone
    for b in batches.values():
        b.close()
    print(json.dumps(out), flush=True)
    results.append(out)

if results:
    with open(_arg("--out", os.path.join(ROOT, "profiles", "episode_cost.json")), "w") as f:
        json.dump(results, f, indent=1)
