// npp_sweep.hpp -- the evaluation sweep (include/npp_amd.h, npp_sweep_start): a fixed list of jobs, each one episode
// on one level, handed to the envs in list order as their episodes end (the reference's eval_mode, env_map_loader.py:138-162, walks
// its test suite the same way, one env at a time).  The rule lives here, shared by the device kernels (npp_sweep.hip) and the
// host-only entry point (npp_host.cpp: npp_sweep_assign_host) and restated in tests/sweep_ref.py.  No HIP header: the host side also
// builds with plain g++.  Integers only.
//
// State: jobs i32[J] (level ids in the caller's order) | counters i32[3] = next (jobs handed out; it runs past J by the envs that
// found the queue dry), done (finished jobs), n_jobs | env_job i32[n] (the job the env plays, -1 = idle) | prev_job i32[n] (the job
// whose episode ended in the last step, -1 = none; consumed by the collect) | one result row per job, as planes i32[SWEEP_RI][J]
// and f64[SWEEP_RD][J].
#pragma once
#include <cstdint>

#include "npp_state.hpp"   // NPP_HD

namespace npp {

// result planes.  i32: the six words of the finished episode (npp_episode.hpp EpWord: steps, frames, switch_step, switch_frames,
// level, bits), the flags byte of its ending step, the env that played it, status (0 = not finished yet, 1 = done).
// f64: the return and the six component sums.
constexpr int SWEEP_R_FLAGS = 6, SWEEP_R_ENV = 7, SWEEP_R_STATUS = 8, SWEEP_RI = 9, SWEEP_RD = 7;
constexpr int SWEEP_NEXT = 0, SWEEP_DONE = 1, SWEEP_NJOBS = 2;

// Start: env e < min(n, J) takes job e, the others are idle; next = min(n, J)
NPP_HD inline int sweep_start_job(int env, int n_jobs) { return env < n_jobs ? env : -1; }

// an env takes part in a step's walk when its episode ended and it holds a job
NPP_HD inline bool sweep_ends_job(int flags, int bits, int env_job) { return (flags & bits) != 0 && env_job >= 0; }

// the job of the env of rank `rank` among those of the walk (env order), `next` as it was before the step; -1 = the queue is dry
NPP_HD inline int sweep_take(int next, int rank, int n_jobs) {
    const int j = next + rank;
    return j < n_jobs ? j : -1;
}

// The whole walk over a flags row, in env order (what npp_sweep_assign_kernel computes with a ballot prefix).  level_trunc may be
// null (dynamic truncation off: trunc is then not touched and may be null).  Returns the number of envs that ended a job; the caller
// adds it to next.
inline int sweep_assign_row(const uint8_t *flags, int bits, int n, const int32_t *jobs, int n_jobs, int next, int32_t *env_job,
                            int32_t *prev_job, int32_t *env_level, int32_t *trunc, const int32_t *level_trunc, uint8_t *changed) {
    int total = 0;
    for (int e = 0; e < n; e++) {
        uint8_t ch = 0;
        if (sweep_ends_job(flags[e], bits, env_job[e])) {
            prev_job[e] = env_job[e];
            const int j = sweep_take(next, total++, n_jobs);
            env_job[e] = j;
            if (j >= 0) {
                const int32_t lvl = jobs[j];
                ch = lvl != env_level[e];
                env_level[e] = lvl;
                if (level_trunc) trunc[e] = level_trunc[lvl];
            }
        }
        changed[e] = ch;
    }
    return total;
}

}  // namespace npp
