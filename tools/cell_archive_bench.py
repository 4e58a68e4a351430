#!/usr/bin/env python
"""Times of the cell index over the checkpoint archive on the door set at 8192 envs and 8192 slots, with HIP events
on the handle's stream: the median of `--reps` calls after a warm-up, in microseconds.  They are event-to-event times of whole
calls -- three launches for explore, two for select, their launch floors included -- not kernel durations.

  step_us                    one npp_step of the same handle, for scale
  explore_reset_us           npp_archive_explore right after a reset: every env of a level proposes for ONE key (maximum
                             contention); after the first call every env loses, so nothing is stored
  explore_reset_store_us     the same with a score that rises from call to call: every cell's winner is stored again each call
  explore_spread_us          npp_archive_explore after `--steps` random steps (the envs spread over many cells), nothing stored
  explore_spread_store_us    the same with the rising score: every occupied cell is stored again each call
  select_256_us / select_all_us   npp_archive_select for 256 masked envs / for all envs
  torch_*                    a torch restatement of the same rule, written below the way a user without these calls writes it
                             (scatter_reduce for the best score and the lowest env per key, a cumulative sum for the slot numbers,
                             NppBatch.archive_store for the records; cumsum + searchsorted + torch's own generator for the pick),
                             on the same device tensors.  It is the yardstick: the parent has no such call.

Prints one JSON line.  Needs the GPU; there is no fallback."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CELLS = 2200


def median_us(stream, fn, reps, warmup):
    for r in range(warmup):
        fn(r)
    stream.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    with torch.cuda.stream(stream):
        for r, (a, b) in enumerate(ev):
            a.record(stream)
            fn(warmup + r)
            b.record(stream)
    stream.synchronize()
    return float(np.median([a.elapsed_time(b) for a, b in ev])) * 1000.0


class TorchCells:
    """The rule in torch ops, without a host synchronisation: tables with one spare entry at the end that masked-out writes go to."""

    def __init__(self, b, n_levels, n_slots, doors):
        d = b.device
        self.b, self.n, self.K, self.n_slots = b, b.n, n_levels * CELLS, n_slots
        self.best = torch.full((self.K + 1,), -float("inf"), dtype=torch.float32, device=d)
        self.cell_slot = torch.full((self.K + 1,), -1, dtype=torch.int32, device=d)
        self.visits = torch.zeros(self.K + 1, dtype=torch.int32, device=d)
        self.chosen = torch.zeros(self.K + 1, dtype=torch.int32, device=d)
        self.n_used = torch.zeros(1, dtype=torch.int32, device=d)
        self.ids = torch.arange(self.n, dtype=torch.int32, device=d)
        self.door = torch.tensor(doors, dtype=torch.float64, device=d)   # [n_levels, 2]
        self.gen = torch.Generator(device=d)
        self.gen.manual_seed(0)

    def explore(self, x, y, state, sw, level, score):
        K, n = self.K, self.n
        cx, cy = torch.floor(x / 24.0).long(), torch.floor(y / 24.0).long()
        dxy = torch.stack([x, y], dim=1) - self.door[level]
        near = sw & (torch.sqrt(dxy[:, 0] * dxy[:, 0] + dxy[:, 1] * dxy[:, 1]) < 72.0)
        ok = (state <= 5) & (cx >= 0) & (cx < 44) & (cy >= 0) & (cy < 25) & ~near & ~torch.isnan(score)
        key = torch.where(ok, level * CELLS + (sw.long() * 25 + cy) * 44 + cx, K)
        self.visits.index_add_(0, key, torch.ones_like(key, dtype=torch.int32))
        top = torch.full((K + 1,), -float("inf"), dtype=torch.float32, device=x.device).scatter_reduce_(0, key, score, "amax")
        cand = ok & (score == top[key]) & (score > self.best[key])
        first = torch.full((K + 1,), n, dtype=torch.int64, device=x.device).scatter_reduce_(
            0, torch.where(cand, key, K), self.ids.long(), "amin")
        win = cand & (first[key] == self.ids)
        old = self.cell_slot[key]
        new = win & (old < 0)
        slot = torch.where(new, self.n_used + torch.cumsum(new, 0, dtype=torch.int32) - 1, old)
        win = win & (slot < self.n_slots)
        wkey = torch.where(win, key, K)
        self.cell_slot[wkey] = torch.where(win, slot, -1)
        self.best[wkey] = torch.where(win, score, -float("inf"))
        self.n_used.copy_(torch.clamp(self.n_used + new.sum(dtype=torch.int32), max=self.n_slots))
        self.b.archive_store(self.ids, torch.where(win, slot, -1))

    def select(self, envs, level):
        w = torch.where(self.cell_slot[:-1] >= 0,
                        torch.floor(1048576.0 / torch.sqrt((self.visits[:-1] + self.chosen[:-1] + 1).double())).long(), 0)
        cdf = torch.cumsum(w, 0)
        per_level = w.view(-1, CELLS).sum(1)
        hi = torch.cumsum(per_level, 0)[level]   # the draw runs over the env's own level: [lo, hi) of the global prefix sums
        lo = hi - per_level[level]
        t = lo + (torch.rand(len(envs), dtype=torch.float64, device=w.device, generator=self.gen) * (hi - lo).double()).long()
        k = torch.searchsorted(cdf, t, right=True).clamp_(max=self.K - 1)
        self.chosen.index_add_(0, k, torch.ones_like(k, dtype=torch.int32))
        return torch.where(hi > lo, self.cell_slot[k], -1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=8192)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--steps", type=int, default=200)
    args = ap.parse_args()
    from nclone_amd.engine import NppBatch
    from nclone_amd.levels import door_levels

    def door_of(m):   # the exit door observations report: the door of the last exit switch in map order
        import ctypes as C

        from nclone_amd import _native as nat

        m = np.ascontiguousarray(np.asarray(m, dtype=np.float64).ravel())
        rows, cnt = np.zeros((4096, 6)), C.c_int(0)
        nat.check(None, nat.lib().npp_compile_level_entities(m.ctypes.data_as(C.POINTER(C.c_double)), len(m),
                                                             rows.ctypes.data_as(C.POINTER(C.c_double)), len(rows), C.byref(cnt)))
        d = [r for r in rows[:cnt.value] if int(r[0]) == 3]
        return (d[-1][1], d[-1][2]) if d else (-1e9, -1e9)

    levels, _ = door_levels()
    n, reps, warm = args.envs, args.reps, args.warmup
    b = NppBatch(n, autoreset=True)
    b.load_levels(levels)
    b.assign_levels((np.arange(n) // 64) % len(levels))
    b.set_truncation_limit(10000)
    b.archive_create(n)
    doors = [door_of(m) for m in levels]
    rng = np.random.default_rng(0)
    with b._ctx():
        acts = torch.from_numpy(rng.integers(0, 6, size=(args.steps, n)).astype(np.uint8)).to(b.device)
        rising = [torch.full((n,), float(r), dtype=torch.float32, device=b.device) for r in range(2 * (reps + warm))]
        few = torch.zeros(n, dtype=torch.uint8, device=b.device)
        few_ids = torch.from_numpy(np.sort(rng.choice(n, size=min(256, n), replace=False))).to(b.device)
        few[few_ids] = 1
        level = torch.from_numpy(b.env_levels().astype(np.int64)).to(b.device)
    out = {"envs": n, "levels": len(levels), "slots": n, "reps": reps, "step_variant": None}
    b.reset()
    out["step_us"] = median_us(b.stream, lambda r: b.step(acts[r % args.steps]), reps, warm)

    def state_tensors():
        f, i = b.dump_state()
        with b._ctx():
            dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(b.device)   # noqa: E731
            return (dev(f[:, 0]), dev(f[:, 1]), dev(i[:, 0]), dev(i[:, 13] != 1), level, dev(-i[:, 22].astype(np.float32)))

    for phase in ("reset", "spread"):
        b.reset()
        if phase == "spread":
            for t in range(args.steps):
                b.step(acts[t])
        b.archive_cells_create(seed=1)
        out["explore_%s_us" % phase] = median_us(b.stream, lambda r: b.archive_explore(), reps, warm)
        out["explore_%s_store_us" % phase] = median_us(b.stream, lambda r: b.archive_explore(score=rising[r]), reps, warm)
        out["cells_%s" % phase] = int(b.archive_cells()["n_used"].item())
        if phase == "spread":
            out["select_256_us"] = median_us(b.stream, lambda r: b.archive_select(few), reps, warm)
            out["select_all_us"] = median_us(b.stream, lambda r: b.archive_select(), reps, warm)
        b.archive_cells_create(enable=False)   # the torch restatement stores through archive_store
        x, y, state, sw, lvl, frames = state_tensors()
        with b._ctx():
            T = TorchCells(b, len(levels), n, doors)
            out["torch_explore_%s_us" % phase] = median_us(b.stream, lambda r: T.explore(x, y, state, sw, lvl, frames), reps, warm)
            out["torch_explore_%s_store_us" % phase] = median_us(b.stream, lambda r: T.explore(x, y, state, sw, lvl, rising[r]), reps, warm)
            out["torch_cells_%s" % phase] = int(T.n_used.item())
            if phase == "spread":
                all_ids = T.ids.long()
                out["torch_select_256_us"] = median_us(b.stream, lambda r: T.select(few_ids, lvl[few_ids]), reps, warm)
                out["torch_select_all_us"] = median_us(b.stream, lambda r: T.select(all_ids, lvl), reps, warm)
    out["step_variant"] = b.step_variant()[0]
    print(json.dumps(out))
    b.close()


if __name__ == "__main__":
    main()
