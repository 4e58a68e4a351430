"""A plain Python / numpy restatement of the cell index over the checkpoint archive (include/npp_amd.h npp_archive_cells_create;
DESIGN.md 17), for tests/test_cell_archive_host.py and tests/test_gpu_cell_archive.py.  It works on npp_dump_state rows: f64
columns 0, 1 (x, y; 2, 3 for the meta row) and i32 columns 0 (ninja state), 13 (exit switch state), 22 (frame), 27 (level).  The
door position comes from the map through npp_compile_level_entities.  Integers are Python integers (pool_mix, (u * T) >> 64), the
weight is math.sqrt and / on floats: nothing here shares code with the library."""
import bisect
import ctypes as C
import math

import numpy as np

GRID_W, GRID_H = 44, 25
CELLS_PER_LEVEL = 2 * GRID_W * GRID_H
M64 = (1 << 64) - 1
STORED, SKIPPED, NOT_ELIGIBLE, LOST, FULL = 0, 1, 5, 6, 7


def pool_mix(z):
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def door_of(map_data):
    """(x, y) of the exit door that observations report (the door of the last exit switch in map order), or None."""
    from nclone_amd import _native as nat

    m = np.ascontiguousarray(np.asarray(map_data, dtype=np.float64).ravel())
    rows = np.zeros((4096, 6), dtype=np.float64)
    n = C.c_int(0)
    rc = nat.lib().npp_compile_level_entities(m.ctypes.data_as(C.POINTER(C.c_double)), len(m), rows.ctypes.data_as(C.POINTER(C.c_double)),
                                              len(rows), C.byref(n))
    assert rc == 0
    doors = [r for r in rows[:n.value] if int(r[0]) == 3]   # kind 3 = exit door; each is followed by its switch
    return (float(doors[-1][1]), float(doors[-1][2])) if doors else None


def key_in_level(state, sw_state, x, y, door):
    """The key of a state inside its level, or -1 when it is not eligible."""
    if not 0 <= state <= 5:
        return -1
    if not (math.isfinite(x) and math.isfinite(y)):
        return -1
    cx, cy = math.floor(x / 24.0), math.floor(y / 24.0)
    if not (0 <= cx < GRID_W and 0 <= cy < GRID_H):
        return -1
    sw = 1 if sw_state != 1 else 0
    if sw == 1 and door is not None:
        dx, dy = x - door[0], y - door[1]
        if math.sqrt(dx * dx + dy * dy) < 72.0:
            return -1
    return (sw * GRID_H + cy) * GRID_W + cx


def ordered_bits(score):
    b = int(np.array([score], dtype=np.float32).view(np.uint32)[0])
    return b ^ (0xFFFFFFFF if b >> 31 else 0x80000000)


def weight(visits, chosen):
    return int(math.floor(1048576.0 / math.sqrt(float(int(visits) + int(chosen) + 1))))


def pick_in_level(cell_slot, visits, chosen, seed, call, env):
    """The slot env `env` draws from ONE level's tables in select call number `call` (-1: no occupied key); also the key."""
    run, cum = 0, []
    for k in range(CELLS_PER_LEVEL):
        if cell_slot[k] >= 0:
            run += weight(visits[k], chosen[k])
        cum.append(run)
    return _pick(cum, seed, call, env, cell_slot)


def _pick(cum, seed, call, env, cell_slot):
    total = cum[-1]
    if total == 0:
        return -1, -1
    u = pool_mix(pool_mix(((env << 32) | call) & M64) ^ (seed & M64))
    t = (u * total) >> 64
    k = bisect.bisect_right(cum, t)   # the first key whose inclusive prefix sum is > t
    assert k < len(cum) and cum[k] > t and (k == 0 or cum[k - 1] <= t)
    return int(cell_slot[k]), k


class CellArchiveRef:
    """The tables and the two calls.  doors: door_of() per level."""

    def __init__(self, doors, n_slots, seed=0):
        self.doors, self.n_slots, self.seed, self.call = list(doors), int(n_slots), int(seed), 0
        K = len(self.doors) * CELLS_PER_LEVEL
        self.best = np.zeros(K, dtype=np.uint32)          # ordered bits of the incumbent's score, 0 = empty
        self.cell_slot = np.full(K, -1, dtype=np.int32)
        self.cell_score = np.zeros(K, dtype=np.float32)
        self.visits = np.zeros(K, dtype=np.uint32)
        self.chosen = np.zeros(K, dtype=np.uint32)
        self.slot_key = np.full(self.n_slots, -1, dtype=np.int32)
        self.n_used = 0
        self.slot_f = np.zeros((self.n_slots, 4), dtype=np.float64)   # the meta rows of the stored states
        self.slot_i = np.zeros((self.n_slots, 6), dtype=np.int32)
        self.slot_env = np.full(self.n_slots, -1, dtype=np.int64)     # (who stored last: for the tests' own bookkeeping)

    def keys(self, f, i):
        """Global key per row, -1 = not eligible by state, cell or exit filter."""
        out = np.full(len(f), -1, dtype=np.int64)
        for e in range(len(f)):
            lvl = int(i[e, 27])
            k = key_in_level(int(i[e, 0]), int(i[e, 13]), float(f[e, 0]), float(f[e, 1]), self.doors[lvl])
            if k >= 0:
                out[e] = lvl * CELLS_PER_LEVEL + k
        return out

    def explore(self, f, i, score=None, mask=None):
        n = len(f)
        if score is None:
            score = (-i[:, 22].astype(np.float32)).astype(np.float32)
        score = np.asarray(score, dtype=np.float32)
        status = np.full(n, NOT_ELIGIBLE, dtype=np.int32)
        keys = self.keys(f, i)
        top = {}   # key -> (ob, env): the largest ob, ties to the lowest env
        for e in range(n):
            if mask is not None and not mask[e]:
                status[e] = SKIPPED
                continue
            if keys[e] < 0 or math.isnan(float(score[e])):
                continue
            k = int(keys[e])
            status[e] = LOST
            self.visits[k] += 1
            ob = ordered_bits(score[e])
            if k not in top or ob > top[k][0]:
                top[k] = (ob, e)
        for k, (ob, e) in sorted(top.items(), key=lambda kv: kv[1][1]):   # ascending env index
            if ob <= int(self.best[k]):
                continue   # an incumbent wins ties
            slot = int(self.cell_slot[k])
            if slot < 0:
                if self.n_used >= self.n_slots:
                    status[e] = FULL
                    continue
                slot = self.n_used
                self.n_used += 1
                self.cell_slot[k] = slot
                self.slot_key[slot] = k
            self.best[k] = ob
            self.cell_score[k] = score[e]
            status[e] = STORED
            self.slot_f[slot] = f[e, :4]
            self.slot_i[slot] = (1, i[e, 27], i[e, 22], math.floor(f[e, 0] / 24.0), math.floor(f[e, 1] / 24.0), int(i[e, 13] != 1))
            self.slot_env[slot] = e
        return status

    def select(self, levels, mask=None):
        """levels [n]: the level every env plays.  All picks use the weights of before the call."""
        n = len(levels)
        out = np.full(n, -1, dtype=np.int32)
        cums, hits = {}, []
        for e in range(n):
            if mask is not None and not mask[e]:
                continue
            lvl = int(levels[e])
            if lvl not in cums:
                lo = lvl * CELLS_PER_LEVEL
                run, cum = 0, []
                for k in range(lo, lo + CELLS_PER_LEVEL):
                    if self.cell_slot[k] >= 0:
                        run += weight(self.visits[k], self.chosen[k])
                    cum.append(run)
                cums[lvl] = cum
            slot, k = _pick(cums[lvl], self.seed, self.call, e, self.cell_slot[lvl * CELLS_PER_LEVEL:])
            out[e] = slot
            if k >= 0:
                hits.append(lvl * CELLS_PER_LEVEL + k)
        for k in hits:
            self.chosen[k] += 1
        self.call += 1
        return out
