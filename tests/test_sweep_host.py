"""The evaluation sweep without a GPU: npp_sweep_assign_host (the rule of csrc/npp_sweep.hpp, built into the library's host part)
against the numpy restatement of tests/sweep_ref.py, the per-level reduction of evaluation_results() on a hand-made table, and the
new entries of the C header."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests.sweep_ref import END_BITS, SweepModel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def native():
    from nclone_amd import build_native

    build_native.build()
    from nclone_amd import _native

    return _native


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _host_assign(native, flags, jobs, counters, env_job, prev_job, env_level, trunc, level_trunc, changed, bits=END_BITS):
    lt = None if level_trunc is None else _p(level_trunc)
    return native.lib().npp_sweep_assign_host(_p(flags), bits, len(flags), _p(jobs), len(jobs), _p(counters), _p(env_job), _p(prev_job),
                                              _p(env_level), None if trunc is None else _p(trunc), lt,
                                              0 if level_trunc is None else len(level_trunc), _p(changed))


def _flags_row(rng, n, share):
    """a flags row: `share` of the envs end (one of won / dead / truncated, with other bits around), the rest carry non-ending bits"""
    ends = rng.random(n) < share if 0.0 < share < 1.0 else np.full(n, share >= 1.0)
    end_bit = rng.choice(np.array([1, 2, 8, 2 | 16, 2 | 32], dtype=np.uint8), size=n)
    noise = rng.choice(np.array([0, 4, 16, 32, 4 | 16], dtype=np.uint8), size=n)
    return np.where(ends, end_bit | (noise & 4), noise).astype(np.uint8)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 1025])
@pytest.mark.parametrize("share", [0.0, 0.05, 1.0])
@pytest.mark.parametrize("queue", ["full", "dry_inside", "dry"])
def test_assign_host_matches_restatement(native, n, share, queue):
    rng = np.random.default_rng(1000 * n + int(share * 100) + len(queue))
    n_levels = 7
    level_trunc = rng.integers(40, 200, size=n_levels).astype(np.int32)
    # the list is long enough for every env's next job | ends in the middle of the first all-ending row | is used up at the start
    J = {"full": 6 * n + 3, "dry_inside": n + max(1, n // 2), "dry": max(1, n - n // 3)}[queue]
    jobs = rng.integers(0, n_levels, size=J).astype(np.int32)
    env_level = rng.integers(0, n_levels, size=n).astype(np.int32)
    for dyn in (False, True):
        trunc = rng.integers(40, 200, size=n).astype(np.int32)
        m = SweepModel(n, jobs, env_level, trunc=trunc if dyn else None, level_trunc=level_trunc if dyn else None)
        m.start()
        assert m.next == min(n, J) and np.array_equal(m.env_job[:m.next], np.arange(m.next))
        counters = np.array([m.next, 0, J], dtype=np.int32)
        env_job, prev_job, lvl = m.env_job.copy(), m.prev_job.copy(), m.env_level.copy()
        tr = m.trunc.copy() if dyn else None
        for step in range(5):
            flags = _flags_row(rng, n, share)
            changed = np.full(n, 7, dtype=np.uint8)
            want = m.assign(flags)
            assert _host_assign(native, flags, jobs, counters, env_job, prev_job, lvl, tr, level_trunc if dyn else None, changed) == native.NPP_OK
            assert np.array_equal(changed, want), (step, "changed")
            assert np.array_equal(env_job, m.env_job) and np.array_equal(prev_job, m.prev_job), (step, "jobs")
            assert np.array_equal(lvl, m.env_level), (step, "levels")
            assert counters.tolist() == [m.next, 0, J], step
            if dyn:
                assert np.array_equal(tr, m.trunc), (step, "trunc")
            m.collect(lambda e: e)
            prev_job[:] = -1
        if share == 1.0:
            # every env that holds a job ends in every row: the ranks are the env order, and the list is handed out front to back
            assert sorted(m.rows) == list(range(min(J, 5 * n)))
        if share == 0.0:
            assert m.next == min(n, J) and not m.rows


def test_assign_host_edges(native):
    """zero-length rows, J at and past next, idle envs, an env that ends without a job, bad arguments"""
    lib = native.lib()
    jobs = np.array([3, 3, 1, 0], dtype=np.int32)
    counters = np.array([4, 0, 4], dtype=np.int32)
    assert lib.npp_sweep_assign_host(None, END_BITS, 0, _p(jobs), 4, _p(counters), None, None, None, None, None, 0, None) == native.NPP_OK
    assert counters.tolist() == [4, 0, 4]
    # n = 3, J = 4, next = 3: of two ending envs the first takes the last job, the second finds the list used up and goes idle
    counters[:] = [3, 0, 4]
    env_job, prev_job = np.array([0, 1, 2], dtype=np.int32), np.full(3, -1, dtype=np.int32)
    lvl, changed = np.array([3, 3, 1], dtype=np.int32), np.zeros(3, dtype=np.uint8)
    flags = np.array([8, 4, 2 | 16], dtype=np.uint8)
    assert _host_assign(native, flags, jobs, counters, env_job, prev_job, lvl, None, None, changed) == native.NPP_OK
    assert env_job.tolist() == [3, 1, -1] and prev_job.tolist() == [0, -1, 2]
    assert lvl.tolist() == [0, 3, 1] and changed.tolist() == [1, 0, 0] and counters.tolist() == [5, 0, 4]
    # the idle env ends again: it holds no job, so nothing moves; env 1 ends on a dry list and goes idle as well
    prev_job[:] = -1
    flags = np.array([0, 1, 8], dtype=np.uint8)
    assert _host_assign(native, flags, jobs, counters, env_job, prev_job, lvl, None, None, changed) == native.NPP_OK
    assert env_job.tolist() == [3, -1, -1] and prev_job.tolist() == [-1, 1, -1] and changed.tolist() == [0, 0, 0]
    assert lvl.tolist() == [0, 3, 1] and counters.tolist() == [6, 0, 4]
    # a job that lands on the level the env already plays: assigned, not changed
    counters[:] = [1, 0, 4]
    env_job, lvl = np.array([0], dtype=np.int32), np.array([3], dtype=np.int32)
    prev_job, changed = np.full(1, -1, dtype=np.int32), np.ones(1, dtype=np.uint8)
    assert _host_assign(native, np.array([1], dtype=np.uint8), jobs, counters, env_job, prev_job, lvl, None, None, changed) == native.NPP_OK
    assert env_job.tolist() == [1] and lvl.tolist() == [3] and changed.tolist() == [0]
    # refusals
    bad = np.array([9], dtype=np.int32)
    assert _host_assign(native, np.zeros(1, dtype=np.uint8), jobs, counters, bad, prev_job, lvl, None, None, changed) == native.NPP_ERR_INVALID
    assert lib.npp_sweep_assign_host(None, END_BITS, -1, _p(jobs), 4, _p(counters), None, None, None, None, None, 0, None) == native.NPP_ERR_INVALID
    assert lib.npp_sweep_assign_host(None, END_BITS, 0, _p(jobs), 4, None, None, None, None, None, None, 0, None) == native.NPP_ERR_INVALID


def test_evaluation_reduction_hand_made():
    from nclone_amd.vec_env import reduce_evaluation

    levels, K = [5, 2, 5], 2   # a level may stand in the list twice: each place is a column of its own
    done = [True, True, True, True, False, True]
    won = [True, False, True, False, True, True]      # (the pending job's values must not count)
    ret = [1.0, -0.5, 0.25, 3.0, 100.0, 0.125]
    frames = [60, 12, 40, 20, 999, 44]
    per = reduce_evaluation(levels, K, done, won, ret, frames)
    assert per["level"].tolist() == [5, 2, 5] and per["episodes"].tolist() == [2, 1, 2]
    assert per["success_rate"].tolist() == [0.5, 0.0, 1.0]
    assert per["mean_return"].tolist() == [2.0, -0.5, 0.1875]
    assert per["mean_frames"].tolist() == [40.0, 12.0, 42.0]
    assert all(per[k].dtype == np.float64 for k in ("success_rate", "mean_return", "mean_frames"))
    # no finished episode at all: zeros, no division warning turned into a NaN
    per = reduce_evaluation([1, 4], 1, [False, False], [True, True], [9.0, 9.0], [5, 5])
    assert per["episodes"].tolist() == [0, 0] and per["success_rate"].tolist() == [0.0, 0.0] and per["mean_return"].tolist() == [0.0, 0.0]
    # the sum runs over the episodes in order, in float64: the bits of a left-to-right sum
    r = np.array([0.1, 0.2, 0.3], dtype=np.float64)
    assert reduce_evaluation([0], 3, [True] * 3, [False] * 3, r, [1, 1, 1])["mean_return"][0] == ((r[0] + r[1]) + r[2]) / 3.0


def test_header_declares_and_library_exports_the_sweep(native):
    hdr = open(os.path.join(ROOT, "include", "npp_amd.h")).read()
    lib = C.CDLL(native.LIB_PATH)
    for name in ("npp_sweep_start", "npp_sweep_stop", "npp_sweep_view", "npp_sweep_assign_host"):
        assert re.search(r"\bint %s\(" % name, hdr), name
        assert name in native.EXPORTS and hasattr(lib, name), name
    declared = sorted(set(re.findall(r"\b(npp_[a-z_0-9]+)\s*\(", hdr)))
    assert sorted(native.EXPORTS) == declared
    # a NULL handle is refused without touching anything
    L = native.lib()
    jobs = np.zeros(1, dtype=np.int32)
    assert L.npp_sweep_start(None, _p(jobs), 1) == native.NPP_ERR_INVALID
    assert L.npp_sweep_stop(None) == native.NPP_ERR_INVALID
    assert L.npp_sweep_view(None, None, None, None, None, None) == native.NPP_ERR_INVALID
