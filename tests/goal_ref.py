"""Plain Python restatement of the goal curriculum's bookkeeping rule (include/npp_amd.h npp_set_goal_curriculum),
independent of nclone_amd/csrc/npp_goal.hpp: what npp_goal_apply_host and the two device kernels must equal, word for word.

State, in the layout of npp_goal_view: level words int32 [10, n_base], ring uint32 [n_base, words], env words int32 [5, N]."""
import numpy as np

STAGE, PENDING, NUM_STAGES, VARIANT0, FILL, HEAD, WINS, ADVANCES, APPENDED, STALE = range(10)
EPISODES, SWITCHES, COMPLETIONS, SEEN, PREV = range(5)
F_WON, F_SWITCH = 1, 4
END_BITS = 1 | 2 | 8


def need_for(window, threshold):
    """the smallest w with w / window >= threshold (Python floats are the C doubles)"""
    for w in range(window + 1):
        if float(w) / float(window) >= threshold:
            return w
    return window + 1


class GoalRef:
    def __init__(self, num_stages, n_envs, window, need, auto_advance=True):
        """num_stages: per base level; the variants follow the base levels, level by level, stage by stage"""
        self.nb, self.n, self.window, self.need, self.auto = len(num_stages), n_envs, window, need, auto_advance
        self.lv = np.zeros((10, self.nb), dtype=np.int32)
        self.ring = np.zeros((self.nb, (window + 31) // 32), dtype=np.uint32)
        self.env = np.zeros((5, n_envs), dtype=np.int32)
        self.lv[PENDING] = -1
        self.base_of, self.stage_of = list(range(self.nb)), [-1] * self.nb
        for b, ns in enumerate(num_stages):
            self.lv[NUM_STAGES, b] = ns
            self.lv[VARIANT0, b] = len(self.base_of) if ns > 0 else b
            for s in range(ns):
                self.base_of.append(b)
                self.stage_of.append(s)
        self.base_of, self.stage_of = np.array(self.base_of, dtype=np.int32), np.array(self.stage_of, dtype=np.int32)
        self.events = dict(advance=0, wrap=0, stale=0, pending=0, pinned=0)

    def level_for(self, level_now):
        b = int(self.base_of[level_now])
        return int(self.lv[VARIANT0, b] + self.lv[STAGE, b]) if self.lv[NUM_STAGES, b] > 0 else b

    def set_stage(self, stage, level=None):
        for b in (range(self.nb) if level is None else [level]):
            ns = int(self.lv[NUM_STAGES, b])
            if ns > 0:
                self.lv[PENDING, b] = min(stage, ns - 1)

    def apply(self, flags, env_level, drawn=None, count=True, end_bits=END_BITS):
        """one application; env_level int32 [N] is updated in place; returns the changed mask"""
        lv, env = self.lv, self.env
        ended = [(int(f) & end_bits) != 0 for f in flags]
        # 1. append, in env order
        for e in range(self.n):
            f = int(flags[e])
            if ended[e]:
                env[PREV, e] = env_level[e]
            if not count:
                if ended[e]:
                    env[SEEN, e] = 0   # an explicit restart abandons the episode and its latch
                continue
            if ended[e]:
                won = bool(f & F_WON)
                env[EPISODES, e] += 1
                env[SWITCHES, e] += int(won or env[SEEN, e] != 0)
                env[COMPLETIONS, e] += int(won)
                env[SEEN, e] = 0
                b, s = int(self.base_of[env_level[e]]), int(self.stage_of[env_level[e]])
                if lv[NUM_STAGES, b] == 0:
                    continue
                if s != lv[STAGE, b]:
                    lv[STALE, b] += 1
                    self.events["stale"] += 1
                    continue
                head = int(lv[HEAD, b])
                bit = np.uint32(1 << (head & 31))
                if lv[FILL, b] == self.window:
                    lv[WINS, b] -= int((self.ring[b, head >> 5] & bit) != 0)
                    self.events["wrap"] += 1
                else:
                    lv[FILL, b] += 1
                if won:
                    self.ring[b, head >> 5] |= bit
                    lv[WINS, b] += 1
                else:
                    self.ring[b, head >> 5] &= ~bit
                lv[HEAD, b] = 0 if head + 1 == self.window else head + 1
                lv[APPENDED, b] += 1
            elif (f & F_SWITCH) and env[SEEN, e] == 0:
                env[SEEN, e] = 1
        for b in range(self.nb):
            ns = int(lv[NUM_STAGES, b])
            # 2. advance
            if count and self.auto and lv[FILL, b] == self.window and lv[WINS, b] >= self.need:
                if lv[STAGE, b] < ns - 1:
                    lv[STAGE, b] += 1
                    lv[ADVANCES, b] += 1
                    lv[FILL, b] = lv[HEAD, b] = lv[WINS, b] = 0
                    self.events["advance"] += 1
                elif ns > 0:
                    self.events["pinned"] += 1
            # 3. a pending stage
            if lv[PENDING, b] >= 0:
                lv[STAGE, b] = min(int(lv[PENDING, b]), ns - 1) if ns > 0 else 0
                lv[PENDING, b] = -1
                self.events["pending"] += 1
        changed = np.zeros(self.n, dtype=np.uint8)
        for e in range(self.n):
            if ended[e]:
                if drawn is not None:
                    env_level[e] = drawn[e]
                env_level[e] = self.level_for(int(env_level[e]))
                changed[e] = env_level[e] != env[PREV, e]
        return changed
