"""Python restatement of the episode-statistics rule (nclone_amd/csrc/npp_episode.hpp; include/npp_amd.h npp_set_episode_stats;
DESIGN.md 24), written from the header's description: integers plus float additions in step order, so the device kernels, the host
entry npp_episode_apply_host and this model agree bit for bit.  tests/test_episode_host.py holds the host entry against it,
tests/test_gpu_episode.py the kernels."""
import math

import numpy as np

STEPS, FRAMES, SWITCH_STEP, SWITCH_FRAMES, LEVEL, BITS = range(6)
FIN, FIN_FLAGS, N_FINISHED, NI = 6, 12, 13, 14
RET, COMP, DFIN, ND = 0, 1, 7, 14
CLOSED, FROM_RESTORE, TICKED = 1, 2, 4
F_WON, F_DEAD, F_SWITCH, F_TRUNCATED, F_MINE, F_IMPACT = 1, 2, 4, 8, 16, 32
END = F_WON | F_DEAD | F_TRUNCATED
COLUMNS = ("episodes", "won", "dead", "truncated", "dead_mine", "dead_impact", "switch", "steps", "frames", "won_frames", "return_fix",
           "restored", "abandoned")
COL = {name: k for k, name in enumerate(COLUMNS)}
COLS = 16
EV_ROW, EV_RESET, EV_RESTORE, EV_TICK, EV_INIT, EV_CLEAR = range(6)   # event kinds of npp_episode_apply_host
M64 = (1 << 64) - 1


def return_fix(ret):
    """floor(clamp(ret, +-2^42) * 2^20 + 0.5) as a two's-complement 64-bit word; NaN counts as 0"""
    if ret != ret:
        ret = 0.0
    ret = min(max(ret, -(2.0 ** 42)), 2.0 ** 42)
    return math.floor(ret * 1048576.0 + 0.5) & M64


def fix_to_float(word):
    """a return_fix sum back as a float"""
    word = int(word) & M64
    return float(word - (1 << 64) if word >> 63 else word) / 1048576.0


class Record:
    def __init__(self):
        self.i = [0] * NI
        self.d = [0.0] * ND
        self.i[LEVEL] = self.i[FIN + LEVEL] = -1

    def start(self, level, bits, comps=True):
        self.i[STEPS:BITS + 1] = [0, 0, 0, 0, level, bits]
        self.d[RET] = 0.0
        if comps:
            self.d[COMP:COMP + 6] = [0.0] * 6

    def copy(self):
        r = Record()
        r.i, r.d = list(self.i), list(self.d)
        return r


def new_table(n_levels):
    return [[0] * COLS for _ in range(n_levels)]


def deltas(rec):
    d = [0] * COLS
    e = rec.i[FIN:FIN + 6]
    if e[BITS] & FROM_RESTORE:
        d[COL["restored"]] = 1
        return d
    f = rec.i[FIN_FLAGS]
    won, dead = bool(f & F_WON), bool(f & F_DEAD)
    d[COL["episodes"]] = 1
    d[COL["won"]] = int(won)
    d[COL["dead"]] = int(dead)
    d[COL["truncated"]] = int(bool(f & F_TRUNCATED))
    d[COL["dead_mine"]] = int(dead and bool(f & F_MINE))
    d[COL["dead_impact"]] = int(dead and bool(f & F_IMPACT))
    d[COL["switch"]] = int(e[SWITCH_STEP] != 0)
    d[COL["steps"]] = e[STEPS]
    d[COL["frames"]] = e[FRAMES]
    d[COL["won_frames"]] = e[FRAMES] if won else 0
    d[COL["return_fix"]] = return_fix(rec.d[DFIN + RET])
    return d


def _add(table, level, d):
    if 0 <= level < len(table):
        table[level] = [(a + b) & M64 for a, b in zip(table[level], d)]


def row(rec, table, f, x, reward, comps, level_now, autoreset):
    """one step row; reward and comps are the f32 values as Python floats; comps None = the component doubles are left alone.
    True when the row finished an episode."""
    if x == 0 or rec.i[BITS] & CLOSED:
        return False
    if rec.i[STEPS] == 0:
        rec.i[LEVEL] = level_now
    rec.i[STEPS] += 1
    rec.i[FRAMES] += x
    rec.d[RET] += reward
    if comps is not None:
        for k in range(6):
            rec.d[COMP + k] += comps[k]
    if f & F_SWITCH and rec.i[SWITCH_STEP] == 0:
        rec.i[SWITCH_STEP] = rec.i[STEPS]
        rec.i[SWITCH_FRAMES] = rec.i[FRAMES]
    if not f & END:
        return False
    rec.i[FIN:FIN + 6] = rec.i[0:6]
    rec.i[FIN_FLAGS] = f
    rec.i[N_FINISHED] = (rec.i[N_FINISHED] + 1) & 0xFFFFFFFF
    rec.d[DFIN + RET] = rec.d[RET]
    if comps is not None:
        rec.d[DFIN + COMP:DFIN + COMP + 6] = rec.d[COMP:COMP + 6]
    _add(table, rec.i[FIN + LEVEL], deltas(rec))
    if autoreset:
        rec.start(level_now, 0, comps is not None)
    else:
        rec.i[BITS] |= CLOSED
    return True


def event(rec, table, kind, level_now=0):
    if kind == EV_INIT:
        rec.__init__()
        return
    if kind == EV_TICK:
        rec.i[BITS] |= TICKED
        return
    if kind != EV_CLEAR and rec.i[STEPS] > 0 and not rec.i[BITS] & (CLOSED | FROM_RESTORE):
        d = [0] * COLS
        d[COL["abandoned"]] = 1
        _add(table, rec.i[LEVEL], d)
    rec.start(level_now, FROM_RESTORE if kind == EV_RESTORE else 0)


def apply_events(rec, table, autoreset, events, rows):
    """events int[count][8] and rows f32[count][8] as npp_episode_apply_host takes them; True when a row finished an episode"""
    any_end = False
    for ev, r in zip(events, rows):
        if ev[0] == EV_ROW:
            comps = [float(v) for v in r[1:7]] if ev[4] else None
            any_end |= row(rec, table, int(ev[1]), int(ev[2]), float(r[0]), comps, int(ev[3]), autoreset)
        else:
            event(rec, table, int(ev[0]), int(ev[1]))
    return any_end


def random_events(rng, n_levels, count, comps):
    """a seeded list that takes every branch now and then: rows of 0 frames, ends, rows after a truncation, a switch on the first
    step of an episode, level changes, resets of empty and of running records, restores, ticks"""
    events = np.zeros((count, 8), dtype=np.int32)
    rows = np.zeros((count, 8), dtype=np.float32)
    level = int(rng.integers(0, n_levels))
    for i in range(count):
        u = rng.random()
        if u < 0.82:
            f = 0
            v = rng.random()
            if v < 0.05:
                f |= F_WON | F_SWITCH
            elif v < 0.12:
                f |= F_DEAD | int(rng.choice([0, F_MINE, F_IMPACT]))
            elif v < 0.17:
                f |= F_TRUNCATED
            if rng.random() < 0.12:
                f |= F_SWITCH
            if f & END and rng.random() < 0.5:
                level = int(rng.integers(0, n_levels))   # the level pool drew before the row is accumulated
            x = 0 if rng.random() < 0.06 else int(rng.integers(1, 5))
            events[i, :5] = [EV_ROW, f, x, level, 1 if comps else 0]
            rows[i, 0] = np.float32(rng.normal() * 10.0 ** float(rng.integers(-3, 3)))
            rows[i, 1:7] = rng.normal(size=6).astype(np.float32)
        else:
            kind = int(rng.choice([EV_RESET, EV_RESET, EV_RESET, EV_RESTORE, EV_TICK, EV_CLEAR]))
            if kind in (EV_RESET, EV_RESTORE) and rng.random() < 0.4:
                level = int(rng.integers(0, n_levels))
            events[i, :2] = [kind, level]
            if kind == EV_RESET and rng.random() < 0.3 and i + 1 < count:   # ... and once more, on the record it just emptied
                events[i + 1, :2] = [EV_RESET, level]
    return events, rows


class Model:
    """N envs and a table, fed whole rows (the batch's flags / frames / reward tensors) and the events the test performs"""

    def __init__(self, n, n_levels, autoreset):
        self.n, self.autoreset = n, autoreset
        self.rec = [Record() for _ in range(n)]
        self.table = new_table(n_levels)

    def accumulate(self, flags, frames, reward, levels, comps=None):
        """flags / frames / reward: [n] or [n_steps][n]; levels: env_level after the launch; -> ended u8[n]"""
        flags, frames, reward = np.atleast_2d(flags), np.atleast_2d(frames), np.atleast_2d(reward)
        if comps is not None:
            comps = np.asarray(comps, dtype=np.float32).reshape(flags.shape[0], self.n, 6)
        ended = np.zeros(self.n, dtype=np.uint8)
        for e in range(self.n):
            for s in range(flags.shape[0]):
                c = [float(v) for v in comps[s, e]] if comps is not None else None
                if row(self.rec[e], self.table, int(flags[s, e]), int(frames[s, e]), float(reward[s, e]), c, int(levels[e]), self.autoreset):
                    ended[e] = 1
        return ended

    def event(self, kind, levels, mask=None):
        for e in range(self.n):
            if mask is None or mask[e]:
                event(self.rec[e], self.table, kind, int(levels[e]))

    def planes(self):
        i32 = np.array([r.i for r in self.rec], dtype=np.int64).T
        i32 = np.where(i32 >= 1 << 31, i32 - (1 << 32), i32).astype(np.int32)
        return i32, np.array([r.d for r in self.rec], dtype=np.float64).T

    def table_i64(self):
        return np.array(self.table, dtype=np.uint64).view(np.int64)
