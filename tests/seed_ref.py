"""A plain Python restatement of seeding the cell index from replays (include/npp_amd.h npp_archive_seed), for
tests/test_seed_host.py and tests/test_gpu_seed.py.  It builds the expected tables from the checkpoints the REFERENCE's seeder
returned (tests/golden/seed.npz, make_golden_seed.py): positions and switch states are the reference's, the schedule is
nclone_amd.demos.plan, the keys come from npp_archive_cell_keys_host, scores compare as ordered bits (cell_archive_ref) and slots
are numbered in call order.  Nothing here runs a simulation."""
import ctypes as C
import os

import numpy as np

from tests import cell_archive_ref as cref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ACTION_OF_BYTE = [0, 3, 2, 5, 1, 4, 0, 0]   # map_input_to_action (replay_executor.py:42-58)


def fixture():
    return np.load(os.path.join(ROOT, "tests", "golden", "seed.npz"))


def byte_mismatch(b):
    """The action of byte b does not press decode_input_to_controls(b)'s controls."""
    return b == 7 or (b >= 8 and (b & 7) not in (0, 6))


def route_of(inputs, f):
    return np.array([ACTION_OF_BYTE[b] if b < 8 else 0 for b in inputs[:f + 1]], dtype=np.uint8)


class Replays:
    """The fixture's replays as the env method sees them: levels = the distinct maps of the replays in `load` (in that order),
    status per replay (0 played, 1 map not loaded, 2 failure, 3 over the cap), and per played replay its eligible ticks: frame ->
    (key, position, switch) from the reference's checkpoints.  The reference's checkpoint AT the break tick of a death is dropped
    (the index takes no dead state)."""

    def __init__(self, z, load=(0, 1, 2), max_per_level=10):
        from nclone_amd import _native as nat

        self.z = z
        R = len(z["src"])
        self.inputs = [z["in%d" % r] for r in range(R)]
        self.maps = [bytes(z["m%d" % r]) for r in range(R)]
        self.levels, ids = [], {}
        for r in load:
            if self.maps[r] not in ids:
                ids[self.maps[r]] = len(self.levels)
                self.levels.append(np.frombuffer(self.maps[r], dtype=np.uint8))
        self.status = np.zeros(R, dtype=np.int32)
        self.level = np.full(R, -1, dtype=np.int32)
        per = {}
        for r in range(R):
            if not z["success"][r]:
                self.status[r] = 2
            elif self.maps[r] not in ids:
                self.status[r] = 1
            elif per.get(ids[self.maps[r]], 0) >= max_per_level:
                self.status[r] = 3
            else:
                per[ids[self.maps[r]]] = per.get(ids[self.maps[r]], 0) + 1
                self.level[r] = ids[self.maps[r]]
        self.played = [r for r in range(R) if self.status[r] == 0]
        lib = nat.lib()
        self.ticks = {}
        for r in self.played:
            sel = np.flatnonzero(z["cp_replay"] == r)
            frames = z["cp_frame"][sel]
            if int(z["end_state"][r]) in (6, 7):
                sel = sel[frames != int(z["break_tick"][r])]
            xy = np.ascontiguousarray(z["cp_pos"][sel], dtype=np.float64)
            state = np.zeros(len(sel), dtype=np.int32)
            sw = np.where(z["cp_switch"][sel] != 0, 0, 1).astype(np.int32)   # npp_dump_state column 13: 1 until collected
            keys = np.full(len(sel), -7, dtype=np.int32)
            m = np.ascontiguousarray(np.frombuffer(self.maps[r], dtype=np.uint8).astype(np.float64))
            rc = lib.npp_archive_cell_keys_host(m.ctypes.data_as(C.POINTER(C.c_double)), len(m), int(self.level[r]), xy.ctypes.data_as(C.c_void_p),
                                                state.ctypes.data_as(C.c_void_p), sw.ctypes.data_as(C.c_void_p), len(sel), keys.ctypes.data_as(C.c_void_p))
            assert rc == 0
            self.ticks[r] = {int(z["cp_frame"][i]): (int(k), z["cp_pos"][i].copy(), int(z["cp_switch"][i])) for i, k in zip(sel, keys) if k >= 0}

    def compact(self):
        from nclone_amd.replay import CompactReplay

        return [CompactReplay(self.maps[r], self.inputs[r].tolist(), bool(self.z["success"][r]), 1) for r in range(len(self.maps))]


def score_of(mode, r, f, L, table=None):
    if mode == "progress":
        return np.float32(np.float64(f) / np.float64(L))
    if mode == "frames":
        return np.float32(-np.float32(f + 1))
    return np.float32(table[r][f])


class Expected:
    """The index after seeding `reps.played` over n_envs envs with n_slots slots.  slot_src[s] = (replay, frame) of the record in slot
    s; counts[r] = candidates, eligible, stored, archive full; events = (replay, frame, slot, replaced replay or -1) per store."""

    def __init__(self, reps, n_envs, n_slots, mode="progress", table=None, n_levels=None):
        from nclone_amd import demos

        self.reps = reps
        K = (len(reps.levels) if n_levels is None else n_levels) * cref.CELLS_PER_LEVEL
        self.best = np.zeros(K, dtype=np.uint64)   # ordered bits of the incumbent's score, 0 = empty
        self.cell_slot = np.full(K, -1, dtype=np.int32)
        self.cell_score = np.zeros(K, dtype=np.float32)
        self.slot_key = np.full(n_slots, -1, dtype=np.int32)
        self.n_used = 0
        self.slot_src = {}
        self.counts = np.zeros((len(reps.maps), 4), dtype=np.int32)
        self.events = []
        lengths = np.array([len(reps.inputs[r]) for r in reps.played], dtype=np.int64)
        plan = demos.plan(lengths, 1, int(lengths.max()) if len(lengths) else 0, n_envs)
        order = [reps.played[k] for k in plan["order"]]
        for q, ticks in enumerate(plan["round_ticks"]):
            envs = order[q * n_envs:(q + 1) * n_envs]   # env e of the round plays envs[e]
            for f in range(int(ticks)):
                top = {}   # key -> (ordered bits, env): the largest, ties to the lowest env
                for e, r in enumerate(envs):
                    L = len(reps.inputs[r])
                    if f >= L:
                        continue
                    self.counts[r, 0] += 1
                    s = score_of(mode, r, f, L, table)
                    if f not in reps.ticks[r] or np.isnan(s):
                        continue
                    self.counts[r, 1] += 1
                    k = reps.ticks[r][f][0]
                    ob = cref.ordered_bits(s)
                    if k not in top or ob > top[k][0]:
                        top[k] = (ob, e, r, s)
                for k, (ob, e, r, s) in sorted(top.items(), key=lambda kv: kv[1][1]):   # ascending env
                    if ob <= int(self.best[k]):
                        continue   # an incumbent wins ties
                    slot = int(self.cell_slot[k])
                    if slot < 0:
                        if self.n_used >= n_slots:
                            self.counts[r, 3] += 1
                            continue
                        slot = self.n_used
                        self.n_used += 1
                        self.cell_slot[k] = slot
                        self.slot_key[slot] = k
                    self.events.append((r, f, slot, self.slot_src[slot][0] if slot in self.slot_src else -1))
                    self.best[k] = ob
                    self.cell_score[k] = s
                    self.slot_src[slot] = (r, f)
                    self.counts[r, 2] += 1

    @property
    def overflow(self):
        return int(self.counts[:, 3].sum())
