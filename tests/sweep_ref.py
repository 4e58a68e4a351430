"""The evaluation sweep's rule (include/npp_amd.h, npp_sweep_start) restated in numpy, written from the header's text and
independent of nclone_amd/csrc/npp_sweep.hpp: what npp_sweep_assign_host and the two device kernels must equal, word for word.

  start    env e < min(n, J) takes job e and is put on jobs[e]; the others are idle; next = min(n, J)
  assign   after a step, over the envs in env order: an env whose flags show an episode end and that holds a job remembers it in
           prev_job and takes job next + rank (rank among such envs of this step, next as before the step), or goes idle when that is
           past the list; next += the number of such envs
  collect  the envs with a prev_job hand their finished episode to that job's row; done += 1 each; prev_job is cleared"""
import numpy as np

END_BITS = 1 | 2 | 8   # won | dead | truncated


class SweepModel:
    def __init__(self, n, jobs, env_level, trunc=None, level_trunc=None):
        self.n = int(n)
        self.jobs = np.asarray(jobs, dtype=np.int32).copy()
        self.J = len(self.jobs)
        self.env_level = np.asarray(env_level, dtype=np.int32).copy()
        self.trunc = None if trunc is None else np.asarray(trunc, dtype=np.int32).copy()
        self.level_trunc = None if level_trunc is None else np.asarray(level_trunc, dtype=np.int32)
        self.env_job = np.full(self.n, -1, dtype=np.int32)
        self.prev_job = np.full(self.n, -1, dtype=np.int32)
        self.next = 0
        self.done = 0
        self.rows = {}   # job -> whatever collect() was handed for it
        self.env_of = np.full(self.J, -1, dtype=np.int32)

    def start(self):
        """-> the envs that got a job (each is reset on its job's level, whether or not the level is another one)"""
        m = min(self.n, self.J)
        self.env_job[:m] = np.arange(m, dtype=np.int32)
        self.next = m
        self.env_level[:m] = self.jobs[:m]
        if self.level_trunc is not None:
            self.trunc[:m] = self.level_trunc[self.jobs[:m]]
        return np.arange(m, dtype=np.int32)

    def assign(self, flags, bits=END_BITS):
        """-> changed u8[n]: 1 where the env goes on to a job on another level than it played"""
        flags = np.asarray(flags).astype(np.int64)
        changed = np.zeros(self.n, dtype=np.uint8)
        rank = 0
        before = self.next
        for e in range(self.n):
            if not (flags[e] & bits) or self.env_job[e] < 0:
                continue
            self.prev_job[e] = self.env_job[e]
            j = before + rank
            rank += 1
            if j < self.J:
                self.env_job[e] = j
                changed[e] = self.jobs[j] != self.env_level[e]
                self.env_level[e] = self.jobs[j]
                if self.level_trunc is not None:
                    self.trunc[e] = self.level_trunc[self.jobs[j]]
            else:
                self.env_job[e] = -1
        self.next = before + rank
        return changed

    def collect(self, record_of_env):
        """record_of_env(e) -> the finished episode env e reported in this step; stored as the row of the job that ended"""
        for e in np.flatnonzero(self.prev_job >= 0):
            j = int(self.prev_job[e])
            assert j not in self.rows, ("job finished twice", j)
            self.rows[j] = record_of_env(int(e))
            self.env_of[j] = e
            self.done += 1
        self.prev_job[:] = -1
