// npp_episode.hip -- episode statistics (include/npp_amd.h, npp_set_episode_stats): the accumulation that runs behind a step
// launch and the events of the other entry points (reset, restore, raw ticks, a new level set).  The rule is npp_episode.hpp's;
// these kernels only fetch its inputs.  One thread per env, no LDS: the env's record (14 words and 14 doubles; 14 words and 2
// doubles without components) is held in registers, the rows of the launch are walked in order, and the record is stored once.
// The step kernels know nothing of this: the accumulation reads the flags, frames and reward rows they (and npp_step_reward) wrote.
//
// The level table is added to with 64-bit integer atomics whose result is not used: integer adds commute, so the table does not
// depend on the order of arrival.  At a row on which lanes of the wavefront end an episode, the lanes are grouped by level (ballot
// + broadcast of the first lane's level); a group of EP_PRESUM_MIN lanes or more sums its columns across the wavefront and its
// first lane adds the non-zero sums, smaller groups add straight from their lanes (at most 11 non-zero columns each).  Measured
// (DESIGN.md 24): without the pre-sum 8192 envs ending on one row of one level take 320 us, all on one 128-byte table row.  No
// float atomics anywhere.
#include <hip/hip_runtime.h>

#include "npp_episode.hpp"
#include "npp_internal.hpp"

namespace npp {
namespace {

template <bool COMPS>
__device__ inline void ep_load(const EpisodeArgs &a, int env, EpRecord &r) {
#pragma unroll
    for (int k = 0; k < EP_NI; k++) r.i[k] = a.i32[(size_t)k * a.n + env];
    if (COMPS) {
#pragma unroll
        for (int k = 0; k < EP_ND; k++) r.d[k] = a.f64[(size_t)k * a.n + env];
    } else {
        r.d[EP_RET] = a.f64[(size_t)EP_RET * a.n + env];
        r.d[EP_DFIN + EP_RET] = a.f64[(size_t)(EP_DFIN + EP_RET) * a.n + env];
    }
}

template <bool COMPS>
__device__ inline void ep_store(const EpisodeArgs &a, int env, const EpRecord &r) {
#pragma unroll
    for (int k = 0; k < EP_NI; k++) a.i32[(size_t)k * a.n + env] = r.i[k];
    if (COMPS) {
#pragma unroll
        for (int k = 0; k < EP_ND; k++) a.f64[(size_t)k * a.n + env] = r.d[k];
    } else {
        a.f64[(size_t)EP_RET * a.n + env] = r.d[EP_RET];
        a.f64[(size_t)(EP_DFIN + EP_RET) * a.n + env] = r.d[EP_DFIN + EP_RET];
    }
}

constexpr int EP_PRESUM_MIN = 4;

__device__ inline unsigned long long wave_sum(unsigned long long v) {
#pragma unroll
    for (int m = 1; m < WAVE; m <<= 1) v += __shfl_xor(v, m, WAVE);
    return v;
}

// The finished episodes of the wavefront's lanes with `end` into their levels' rows; a level outside the table (an episode that
// never saw a row) adds nothing.  Called by every lane of the wavefront that has not left the kernel, in step (the loop below runs
// on wave-uniform values only).
__device__ inline void ep_table_add(const EpisodeArgs &a, const EpRecord &r, bool end) {
    int level = end ? r.i[EP_FIN + EP_LEVEL] : -1;
    if ((unsigned)level >= (unsigned)a.n_levels) level = -1;
    unsigned long long todo = __ballot(level >= 0);
    if (!todo) return;
    uint64_t d[EP_COLS];
    if (level >= 0) ep_deltas(r, d);
    else
        for (int k = 0; k < EP_COLS; k++) d[k] = 0;
    const int lane = threadIdx.x & (WAVE - 1);
    while (todo) {
        const int first = __ffsll(todo) - 1;
        const int lv = __shfl(level, first, WAVE);
        const bool mine = level == lv;
        const unsigned long long group = __ballot(mine);
        unsigned long long *row = a.table + (size_t)lv * EP_COLS;
        if (__popcll(group) >= EP_PRESUM_MIN) {
#pragma unroll
            for (int k = 0; k < EPC_USED; k++) {
                const unsigned long long sum = wave_sum(mine ? (unsigned long long)d[k] : 0ull);
                if (lane == first && sum) (void)atomicAdd(row + k, sum);
            }
        } else if (mine) {
#pragma unroll
            for (int k = 0; k < EPC_USED; k++)
                if (d[k]) (void)atomicAdd(row + k, (unsigned long long)d[k]);
        }
        todo &= ~group;
    }
}

template <bool COMPS>
__global__ __launch_bounds__(256) void npp_episode_kernel(EpisodeArgs a) {
    const int env = blockIdx.x * 256 + threadIdx.x;
    if (blockIdx.x * 256 + (threadIdx.x & ~(WAVE - 1)) >= a.n) return;   // a wavefront wholly past the end
    const bool valid = env < a.n;   // the lanes past the end of a partial wavefront stay for the wave-wide table sum and touch nothing
    EpRecord r;
    ep_init(r);
    int level_now = -1;
    if (valid) {
        ep_load<COMPS>(a, env, r);
        level_now = a.env_level[env];
    }
    bool any = false;
    for (int s = 0; s < a.n_steps; s++) {
        bool end = false;
        if (valid) {
            const size_t o = (size_t)s * a.n + env;
            float c[EP_NCOMP] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            if (COMPS) {   // six floats, 24 bytes per env: three 8-byte loads
                const float2 *p = reinterpret_cast<const float2 *>(a.comps + o * EP_NCOMP);
#pragma unroll
                for (int k = 0; k < 3; k++) { const float2 v = p[k]; c[2 * k] = v.x; c[2 * k + 1] = v.y; }
            }
            end = ep_row<COMPS>(r, a.flags[o], a.frames[o], a.reward[o], c, level_now, a.autoreset != 0);
        }
        ep_table_add(a, r, end);
        any |= end;
    }
    if (!valid) return;
    ep_store<COMPS>(a, env, r);
    if (a.ended) a.ended[env] = any ? 1 : 0;
}

__global__ __launch_bounds__(256) void npp_episode_event_kernel(EpisodeArgs a, int event) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    int env = i;
    if (a.envs) {   // a list of envs, entry i skipped when its status is not 0 (npp_archive_restore)
        if (i >= a.count) return;
        if (a.env_status && a.env_status[i] != 0) return;
        env = a.envs[i];
        if (env < 0 || env >= a.n) return;
    } else {
        if (env >= a.n) return;
        if (a.mask && a.mask[env] == 0) return;
    }
    if (event == EP_EV_TICK) { a.i32[(size_t)EP_BITS * a.n + env] |= EP_TICKED; return; }
    EpRecord r;
    if (event == EP_EV_INIT) ep_init(r);
    else ep_load<true>(a, env, r);
    const int charged = ep_event(r, event, a.env_level[env]);
    if ((unsigned)charged < (unsigned)a.n_levels) (void)atomicAdd(a.table + (size_t)charged * EP_COLS + EPC_ABANDONED, 1ull);
    ep_store<true>(a, env, r);
}

}  // namespace

hipError_t launch_episode(const EpisodeArgs &a, hipStream_t s) {
    if (a.n <= 0 || a.n_steps <= 0) return hipSuccess;
    if (a.comps) hipLaunchKernelGGL(npp_episode_kernel<true>, dim3((a.n + 255) / 256), dim3(256), 0, s, a);
    else hipLaunchKernelGGL(npp_episode_kernel<false>, dim3((a.n + 255) / 256), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_episode_event(const EpisodeArgs &a, int event, hipStream_t s) {
    const int items = a.envs ? a.count : a.n;
    if (a.n <= 0 || items <= 0) return hipSuccess;
    hipLaunchKernelGGL(npp_episode_event_kernel, dim3((items + 255) / 256), dim3(256), 0, s, a, event);
    return hipGetLastError();
}

}  // namespace npp
