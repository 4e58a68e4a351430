#!/usr/bin/env python
"""Times of the checkpoint archive on the door set at 8192 envs, with HIP events on the handle's stream: the median
of `--reps` single launches after a warm-up, in microseconds.

  restore_all_us      npp_restore(NULL), the one-slot snapshot every handle has had: the yardstick
  snapshot_us         npp_snapshot, the store of that slot
  archive_store_us    npp_archive_store of n entries (env e -> slot e)
  archive_restore_us  npp_archive_restore of n entries under a random permutation (inside each level: a slot restores only into
                      envs of its level)
  archive_restore_256_us  npp_archive_restore of 256 entries, a typical per-step restart
  replay_reset_us     the existing reset(options={"checkpoint": seq}) with a 100-action sequence (median of --replay-reps calls,
                      host time included: it is what the caller waits for)
  record_bytes        size of one slot's record

Prints one JSON line.  Needs the GPU; there is no fallback."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def median_us(stream, fn, reps, warmup):
    for _ in range(warmup):
        fn()
    stream.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    with torch.cuda.stream(stream):
        for a, b in ev:
            a.record(stream)
            fn()
            b.record(stream)
    stream.synchronize()
    return float(np.median([a.elapsed_time(b) for a, b in ev])) * 1000.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=8192)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--replay-reps", type=int, default=10)
    args = ap.parse_args()
    from nclone_amd.levels import door_levels
    from nclone_amd.vec_env import NppVecEnvironment

    levels, _ = door_levels()
    n = args.envs
    env = NppVecEnvironment(levels, n, checkpoint_slots=n, truncation_limit=10000)
    b = env.batch
    level_ids = b.env_levels()
    rng = np.random.default_rng(0)
    env.reset(seed=0)
    for _ in range(40):   # the states to store are spread over the levels, not the spawn
        env.step(rng.integers(0, 6, size=n).astype(np.uint8))
    perm = np.arange(n, dtype=np.int32)
    for l in np.unique(level_ids):
        e = np.flatnonzero(level_ids == l)
        perm[e] = rng.permutation(e)
    with b._ctx():
        ids = torch.arange(n, dtype=torch.int32, device=b.device)
        d_perm = torch.from_numpy(perm).to(b.device)
        few = torch.from_numpy(rng.choice(n, size=min(256, n), replace=False).astype(np.int32)).to(b.device)
        few_slots = d_perm[few.long()].contiguous()
    b.snapshot()
    status = b.archive_store(ids, ids, status=True)
    assert not status.any().item()
    assert not b.archive_restore(ids, d_perm, status=True).any().item()
    out = {"envs": n, "levels": len(levels), "reps": args.reps, "record_bytes": b.archive_record_bytes()}
    out["restore_all_us"] = median_us(b.stream, lambda: b.restore(), args.reps, args.warmup)
    out["snapshot_us"] = median_us(b.stream, lambda: b.snapshot(), args.reps, args.warmup)
    out["archive_store_us"] = median_us(b.stream, lambda: b.archive_store(ids, ids), args.reps, args.warmup)
    out["archive_restore_us"] = median_us(b.stream, lambda: b.archive_restore(ids, d_perm), args.reps, args.warmup)
    out["archive_restore_256_us"] = median_us(b.stream, lambda: b.archive_restore(few, few_slots), args.reps, args.warmup)
    seq = rng.integers(0, 6, size=100).astype(np.uint8)

    def replay():
        env.reset(options={"checkpoint": seq})

    out["replay_reset_us"] = median_us(b.stream, replay, args.replay_reps, 2)
    print(json.dumps(out))
    env.close()


if __name__ == "__main__":
    main()
