// npp_sweep.hip -- the evaluation sweep's two launches (include/npp_amd.h, npp_sweep_start; the rule: npp_sweep.hpp),
// only while a sweep is on:
//   npp_sweep_assign_kernel    behind the step, in the place of the level pool's draw (npp_capi.cpp: pool_redraw).  ONE workgroup of
//                              256 lanes walks the step's flags row in env order, 1024 envs a round, as npp_goal_update_kernel does:
//                              an env that ended a job gets its rank among such envs (ballot prefix inside a wavefront, a four-entry
//                              scan across wavefronts, a running total across rounds) and takes job next + rank, or goes idle when
//                              the queue is dry.  It writes env_job, prev_job, env_level, trunc and the changed mask the masked reset
//                              and observe launches read.  No atomic: the same bits in every run.
//   npp_sweep_collect_kernel   behind the episode accumulation (npp_episode_accumulate, n_steps == 1): one lane per env copies the
//                              finished half of the env's episode record into the result row of the job that ended.  `done` is an
//                              integer atomic whose result is not used.
#include <hip/hip_runtime.h>

#include "npp_episode.hpp"
#include "npp_internal.hpp"
#include "npp_sweep.hpp"

namespace npp {
namespace {

static_assert(SWEEP_RD == EP_DWORDS && SWEEP_R_FLAGS == EP_WORDS, "a result row is the finished half of an episode record");

__global__ __launch_bounds__(256) void npp_sweep_assign_kernel(SweepArgs a) {
    __shared__ int wave_count[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int next = a.counters[SWEEP_NEXT];   // as it was before this step: only this workgroup writes it, behind the walk
    int total = 0;
    // 1024 envs per round: the four chunks' flags, jobs and levels are loaded together, ahead of their use, so a round pays the
    // memory latency once; the chunks are then ranked one after the other, which keeps the ranks in env order
    constexpr int K = 4;
    for (int base = 0; base < a.n; base += 256 * K) {
        int fk[K], jk[K], lk[K];
#pragma unroll
        for (int k = 0; k < K; k++) {
            const int env = base + k * 256 + tid;
            fk[k] = env < a.n ? a.flags[env] : 0;
            jk[k] = env < a.n ? a.env_job[env] : -1;
            lk[k] = env < a.n ? a.env_level[env] : 0;
        }
#pragma unroll
        for (int k = 0; k < K; k++) {
            const int env = base + k * 256 + tid;
            const bool ends = env < a.n && sweep_ends_job(fk[k], a.bits, jk[k]);
            // every lane of the workgroup reaches the ballot and both barriers, whatever env < n says
            const unsigned long long m = __ballot(ends);
            if (lane == 0) wave_count[wave] = __popcll(m);
            __syncthreads();
            int off = total;
            for (int w = 0; w < wave; w++) off += wave_count[w];
            total += wave_count[0] + wave_count[1] + wave_count[2] + wave_count[3];
            if (env < a.n) {
                uint8_t changed = 0;
                if (ends) {
                    const int j = sweep_take(next, off + __popcll(m & ((1ull << lane) - 1ull)), a.n_jobs);
                    a.prev_job[env] = jk[k];
                    a.env_job[env] = j;
                    if (j >= 0) {
                        const int lvl = a.jobs[j];
                        changed = lvl != lk[k];
                        a.env_level[env] = lvl;
                        if (a.level_trunc) a.trunc[env] = a.level_trunc[lvl];
                    }
                }
                a.changed[env] = changed;
            }
            __syncthreads();   // wave_count is rewritten by the next chunk
        }
    }
    if (tid == 0) a.counters[SWEEP_NEXT] = next + total;
}

__global__ __launch_bounds__(256) void npp_sweep_collect_kernel(SweepArgs a) {
    const int env = blockIdx.x * 256 + threadIdx.x;
    if (env >= a.n) return;
    const int job = a.prev_job[env];
    if (job < 0) return;
    if (job < a.n_jobs) {
        const size_t J = (size_t)a.n_jobs;
#pragma unroll
        for (int k = 0; k < EP_WORDS; k++) a.res_i32[k * J + job] = a.ep_i32[(size_t)(EP_FIN + k) * a.n + env];
        a.res_i32[SWEEP_R_FLAGS * J + job] = a.ep_i32[(size_t)EP_FIN_FLAGS * a.n + env];
        a.res_i32[SWEEP_R_ENV * J + job] = env;
        a.res_i32[SWEEP_R_STATUS * J + job] = 1;
#pragma unroll
        for (int k = 0; k < SWEEP_RD; k++) a.res_f64[k * J + job] = a.ep_f64[(size_t)(EP_DFIN + k) * a.n + env];
        (void)atomicAdd(a.counters + SWEEP_DONE, 1);
    }
    a.prev_job[env] = -1;
}

}  // namespace

hipError_t launch_sweep_assign(const SweepArgs &a, hipStream_t s) {
    if (a.n <= 0) return hipSuccess;
    hipLaunchKernelGGL(npp_sweep_assign_kernel, dim3(1), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_sweep_collect(const SweepArgs &a, hipStream_t s) {
    if (a.n <= 0) return hipSuccess;
    hipLaunchKernelGGL(npp_sweep_collect_kernel, dim3((a.n + 255) / 256), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace npp
