// npp_goal.hip -- the goal curriculum's bookkeeping behind the step (include/npp_amd.h, npp_set_goal_curriculum; the rule:
// npp_goal.hpp).  Two launches, only while the mode is on:
//   npp_goal_update_kernel   ONE workgroup of 256 lanes.  It walks the step's flags row in env order, 1024 envs a round: every lane
//                            does its env's half of the rule (counters, switch latch) and the envs whose episode ended are compacted,
//                            still in env order, into a list of (base level, stage, won) (ballot prefix inside a wavefront, a four-entry scan across wavefronts).
//                            Then one lane per base level walks that short list, appends the outcomes of its level to the level's
//                            ring, and applies the advance and a pending stage.  Nothing depends on the order in which lanes arrive
//                            and no atomic is used, so the result is the same bits in every run.
//   npp_goal_assign_kernel   one lane per env, after the level pool's draw: an env that ended goes to the variant of its level's stage.
// The level pool's draw (npp_pool.hip) stands between the two; the envs under the mask written here are then reset and observed by
// the launches the pool uses (npp_capi.cpp: pool_redraw).
#include <hip/hip_runtime.h>

#include "npp_goal.hpp"
#include "npp_internal.hpp"

namespace npp {
namespace {

__global__ __launch_bounds__(256) void npp_goal_update_kernel(GoalArgs a) {
    __shared__ int wave_count[4];
    const GoalState &g = a.g;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int total = 0;
    // 1024 envs per round: the four chunks' flags and levels are loaded together, ahead of their use, so a round pays the memory
    // latency once; the chunks are then compacted one after the other, which keeps the list in env order
    constexpr int K = 4;
    for (int base = 0; base < g.n; base += 256 * K) {
        int fk[K], lk[K];
#pragma unroll
        for (int k = 0; k < K; k++) {
            const int env = base + k * 256 + tid;
            fk[k] = env < g.n ? a.flags[env] : 0;
            lk[k] = env < g.n ? a.env_level[env] : 0;
        }
#pragma unroll
        for (int k = 0; k < K; k++) {
            const int env = base + k * 256 + tid, f = fk[k], lvl = lk[k];
            const bool ended = env < g.n && (f & a.bits) != 0;
            if (env < g.n) {
                if (a.count) goal_env_row(g, env, f, ended, lvl);
                else if (ended) goal_env_restart(g, env, lvl);
            }
            // what the level walk needs of an ended env is loaded here, by 256 lanes at once, not by the walking lane
            const int e_base = ended ? g.base_of[lvl] : 0, e_stage = ended ? g.stage_of[lvl] : 0;
            const unsigned long long m = __ballot(ended);
            if (lane == 0) wave_count[wave] = __popcll(m);
            __syncthreads();
            int off = total;
            for (int w = 0; w < wave; w++) off += wave_count[w];
            if (ended && a.count) {
                const int at = off + __popcll(m & ((1ull << lane) - 1ull));
                a.list[at] = e_base;
                a.list[g.n + at] = e_stage * 2 + (f & GOAL_F_WON);   // (stage -1 of a base level: -2 | won, never equal to a stage)
            }
            total += wave_count[0] + wave_count[1] + wave_count[2] + wave_count[3];
            __syncthreads();   // wave_count is rewritten by the next chunk; the list is read below by other lanes
        }
    }
    if (!a.count) total = 0;
    for (int l = tid; l < g.n_base; l += 256) {
        if (goal_lv(g, GL_NUM_STAGES, l) > 0 && total > 0) {
            int b = a.list[0], sw = a.list[g.n];   // the next entry's two words are loaded before this one's are used
            for (int i = 0; i < total; i++) {
                const int nb = i + 1 < total ? a.list[i + 1] : -1, nsw = i + 1 < total ? a.list[g.n + i + 1] : 0;
                if (b == l) goal_append(g, l, sw >> 1, (sw & 1) != 0);
                b = nb;
                sw = nsw;
            }
        }
        goal_finish(g, l, a.count != 0);
    }
}

__global__ __launch_bounds__(256) void npp_goal_assign_kernel(GoalArgs a) {
    const GoalState &g = a.g;
    const int env = blockIdx.x * 256 + threadIdx.x;
    if (env >= g.n) return;
    uint8_t changed = 0;
    if (a.flags[env] & a.bits) {
        const int now = a.env_level[env], prev = goal_env(g, GE_PREV, env);
        const int next = goal_level_for(g, now);
        if (next != now) {
            a.env_level[env] = next;
            if (a.level_trunc) a.trunc[env] = a.level_trunc[next];
        }
        changed = next != prev;
    }
    a.changed[env] = changed;
}

}  // namespace

hipError_t launch_goal_update(const GoalArgs &a, hipStream_t s) {
    hipLaunchKernelGGL(npp_goal_update_kernel, dim3(1), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_goal_assign(const GoalArgs &a, hipStream_t s) {
    hipLaunchKernelGGL(npp_goal_assign_kernel, dim3((a.g.n + 255) / 256), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace npp
