"""Speed figures of the action routes for DESIGN.md 18: the per-step cost of the append at 8192 envs on the headline set (HIP
events over 200-step windows, routes off and on alternating), and npp_archive_store of 64 and of 8192 entries at route length 16 against a
length near the capacity.  Prints one JSON line per part.

    python tools/route_cost.py
    rocprofv3 --kernel-trace --stats --output-format csv -d OUT -- python tools/route_cost.py --store-only --lens 2496
                                    # kernel durations of the store at one route length (the calls themselves are enqueue-bound)
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

out = {}
STORE_ONLY = "--store-only" in sys.argv
LENS = [int(v) for v in sys.argv[sys.argv.index("--lens") + 1].split(",")] if "--lens" in sys.argv else [16, 2496]
n, W, K, ROUNDS = 8192, (0 if STORE_ONLY else 1300), 200, (0 if STORE_ONLY else 4)
levels, _tags = level_sets.curriculum0_levels()
rng = np.random.default_rng(0)
acts = torch.from_numpy(rng.integers(0, 6, size=(W + 2 * ROUNDS * K, n)).astype(np.uint8)).cuda()
batches = {}
for name, cap in (("off", 0), ("on", 2500)):
    b = NppBatch(n, autoreset=True, outputs=["work"])
    b.load_levels(levels)
    b.assign_levels((np.arange(n) // 64) % len(levels))
    if cap:
        b.set_routes(cap)
    for k in range(W):
        b.step(acts[k], 4, want_terminal=False)
    b.sync()
    batches[name] = b
out["variant"] = {k: b.step_variant() for k, b in batches.items()}
us = {"off": [], "on": []}
k0 = W
for r in range(ROUNDS):
    for name in (("off", "on") if r % 2 == 0 else ("on", "off")):
        b = batches[name]
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record(b.stream)
        for k in range(K):
            b.step(acts[k0 + k], 4, want_terminal=False)
        e1.record(b.stream)
        torch.cuda.synchronize()
        us[name].append(e0.elapsed_time(e1) * 1e3 / K)
    k0 += K
if not STORE_ONLY:
    out["step_us_routes_off"] = us["off"]
    out["step_us_routes_on"] = us["on"]
    out["append_us_per_step"] = float(np.median(us["on"]) - np.median(us["off"]))
hdr = batches["on"].route_views()[1].cpu().numpy()
out["route_len_mean_after_run"] = float(hdr[:, 0].mean())
for b in batches.values():
    b.close()
print(json.dumps(out), flush=True)

# archive store: 64 entries, short routes against routes near the capacity
store = {}
NS = 8192
for label, steps in [("len%d" % v, v) for v in LENS]:
    b = NppBatch(NS, autoreset=False)
    b.load_levels(levels[:1])
    b.assign_levels(np.zeros(NS, dtype=np.int32))
    b.set_truncation_limit(100000)
    b.set_routes(2500)
    b.archive_create(NS)
    b.reset()
    b.step_many(torch.zeros((steps, NS), dtype=torch.uint8, device="cuda"), 1)   # NOOP at the spawn, one frame per action
    lens = b.route_views()[1].cpu().numpy()[:, 0]
    ids = torch.arange(NS, dtype=torch.int32, device="cuda")
    store[label] = {"route_len_min": int(lens.min()), "route_len_max": int(lens.max()), "record_bytes": b.archive_record_bytes()}
    for entries in (64, NS):
        sel = ids[:entries].contiguous()
        for _ in range(20):
            b.archive_store(sel, sel)
        t = []
        for _ in range(5):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record(b.stream)
            for _ in range(100):
                b.archive_store(sel, sel)
            e1.record(b.stream)
            torch.cuda.synchronize()
            t.append(e0.elapsed_time(e1) * 1e3 / 100)
        store[label]["store_us_per_call_%d_entries" % entries] = t
    b.close()
out["archive_store"] = store
print(json.dumps(out), flush=True)
