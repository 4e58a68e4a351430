#!/usr/bin/env python3
"""Cost of the frame augmentation per step: 8192 envs, visual stack K in {1, 4}, p in {0, 0.5, 1}: the time of one
npp_frame_augment launch from HIP events around it, the bytes it reads and writes, and, for scale, the time of a plain
device-to-device copy of the same bytes (the sources into the destinations with tensor.copy_) measured in the same run.

    python3 tools/frame_aug_cost.py [--envs 8192] [--warmup 20] [--iters 100] [--reps 3] [--intensity medium]

The sources are one rendered observation per configuration (curriculum 0 levels, a few random steps so that the stack holds
different frames); the launch is repeated on it, every call with a new draw (the call count advances).  At p = 0 every frame
takes the copy path.  Configurations alternate `reps` times.  Prints one JSON line.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from nclone_amd.engine import NppBatch  # noqa: E402
from nclone_amd.levels import curriculum0_levels  # noqa: E402

PF, GV = 84 * 84, 176 * 100


def setup(n, k):
    levels = curriculum0_levels()[0]
    b = NppBatch(n, autoreset=True, fast_reset=True, outputs=("global_view",))
    b.load_levels(levels)
    b.assign_levels((np.arange(n) // 64) % len(levels))
    b.set_frame_stack(k, 0, "zero")
    b.reset()
    acts = torch.from_numpy(np.random.default_rng(0).integers(0, 6, size=(k + 2, n)).astype(np.uint8)).to(b.device)
    for s in range(k + 2):
        b.step(acts[s], 4)
        b.render_player_frame_stacked()
        b.render_global_view()
        b.join()
        b.frame_stack_push(11, s == 0)
    return b


def timed(b, fn, warmup, iters):
    for _ in range(warmup):
        fn()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(iters + 1)]
    ev[0].record(b.stream)
    for i in range(iters):
        fn()
        ev[i + 1].record(b.stream)
    torch.cuda.synchronize()
    us = np.array([ev[i].elapsed_time(ev[i + 1]) * 1e3 for i in range(iters)])
    return float(np.median(us)), float(us.min()), float(us.max())


def run(n, k, p, intensity, warmup, iters):
    b = setup(n, k)
    b.set_frame_augmentation(True, p, intensity, seed=1)
    b.frame_augment()
    apf, agv = b.frame_augment_views()
    pf, _ = b.frame_stack_views()
    gv = b.out.t["global_view"]
    nbytes = n * (k * PF + GV)
    with b._ctx():
        aug = timed(b, b.frame_augment, warmup, iters)

        def copy():
            apf.copy_(pf)
            agv.copy_(gv)

        cp = timed(b, copy, warmup, iters)
        b.frame_augment()   # (leave the buffers as the feature leaves them)
    b.close()
    return {"k": k, "p": p, "bytes_read": nbytes, "bytes_written": nbytes, "augment_us": aug[0], "augment_us_min": aug[1],
            "augment_us_max": aug[2], "copy_us": cp[0], "copy_us_min": cp[1], "copy_us_max": cp[2],
            "augment_tb_s": 2 * nbytes / (aug[0] * 1e-6) / 1e12, "copy_tb_s": 2 * nbytes / (cp[0] * 1e-6) / 1e12}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=8192)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--intensity", default="medium")
    a = ap.parse_args()
    runs = [run(a.envs, k, p, a.intensity, a.warmup, a.iters) for _ in range(a.reps) for k in (1, 4) for p in (0.0, 0.5, 1.0)]
    out = {"envs": a.envs, "iters": a.iters, "intensity": a.intensity, "runs": runs}
    for k in (1, 4):
        for p in (0.0, 0.5, 1.0):
            sel = [r for r in runs if r["k"] == k and r["p"] == p]
            out["k%d_p%g" % (k, p)] = {"augment_us": float(np.mean([r["augment_us"] for r in sel])),
                                       "copy_us": float(np.mean([r["copy_us"] for r in sel])), "bytes_moved": 2 * sel[0]["bytes_read"]}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
