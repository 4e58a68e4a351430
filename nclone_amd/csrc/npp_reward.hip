// npp_reward.hip -- reward mode "pbrs" (include/npp_amd.h, npp_set_reward_mode / npp_step_reward): the reference's step reward for
// every env, in a launch of its own behind the step.  The rule is npp_reward.hpp's; this kernel fetches its inputs, runs it and
// stores the env's reward state back.
// One lane per env, 256-lane blocks, no LDS.  A lane's work: (level id, x, y, the flags byte, the frames word, word E of the state,
// the 13 + 7 state planes -- all independent, all coalesced across lanes: SoA planes and rows of consecutive envs) -> (the level's
// ReachHdr and RewardLevel) -> the rule: always one gather of four node records at the integer position (the fallback distance),
// on a cell change a second one at the exact position and the feature code's queries, on a position-cache miss of the exit phase
// nothing more (it shares the integer gather).  Bytes per env: 132 state in + 132 out, 16 position, ~16 rows, 192-384 records,
// 4-28 out ~ 0.7 KB -> 5.6 MB per launch at 8192 envs: latency bound, like npp_path_mask_kernel.
#include <hip/hip_runtime.h>

#include "npp_internal.hpp"
#include "npp_reward.hpp"

namespace npp {
namespace {

__device__ __forceinline__ void reward_state_load(const RewardArgs &a, size_t N, size_t e, RewardState &S) {
    const double *d = a.sd + e;
    S.d_sw = d[0 * N]; S.d_ex = d[1 * N]; S.pc_dist = d[2 * N]; S.last_x = d[3 * N]; S.last_y = d[4 * N]; S.c_dist = d[5 * N];
    S.prev_potential = d[6 * N]; S.ms_sw = d[7 * N]; S.ms_ex = d[8 * N]; S.path_len = d[9 * N]; S.prev_x = d[10 * N]; S.prev_y = d[11 * N];
    S.optimal = d[12 * N];
    const uint32_t *w = a.si + e;
    S.key = w[0 * N]; S.pc_node = (int32_t)w[1 * N]; S.pc_hop = (int32_t)w[2 * N]; S.c_node = (int32_t)w[3 * N]; S.c_hop = (int32_t)w[4 * N];
    S.bits = w[5 * N]; S.epoch2 = w[6 * N];
}

__device__ __forceinline__ void reward_state_store(const RewardArgs &a, size_t N, size_t e, const RewardState &S) {
    double *d = a.sd + e;
    d[0 * N] = S.d_sw; d[1 * N] = S.d_ex; d[2 * N] = S.pc_dist; d[3 * N] = S.last_x; d[4 * N] = S.last_y; d[5 * N] = S.c_dist;
    d[6 * N] = S.prev_potential; d[7 * N] = S.ms_sw; d[8 * N] = S.ms_ex; d[9 * N] = S.path_len; d[10 * N] = S.prev_x; d[11 * N] = S.prev_y;
    d[12 * N] = S.optimal;
    uint32_t *w = a.si + e;
    w[0 * N] = S.key; w[1 * N] = (uint32_t)S.pc_node; w[2 * N] = (uint32_t)S.pc_hop; w[3 * N] = (uint32_t)S.c_node; w[4 * N] = (uint32_t)S.c_hop;
    w[5 * N] = S.bits; w[6 * N] = S.epoch2;
}

// the dictionary npp_reachability shares (ReachMiss): a reset of the env since the last call of either kernel empties it, exactly as
// npp_reach_kernel does it (the episode counter is S_EPISODE of word E)
__device__ __forceinline__ ReachMiss reward_shared_dictionary(const RewardArgs &a, size_t e, uint32_t word_e) {
    ReachMiss M{nullptr, nullptr, 1u};
    if (a.md.stamp) {
        const uint32_t ep = (uint32_t)field_get(word_e, S_EPISODE);
        uint32_t epoch = a.md.epoch[e];
        if (epoch == 0u || a.md.last_episode[e] != ep) {
            epoch++;
            if (epoch == 0u) epoch = 1u;
            a.md.epoch[e] = epoch;
            a.md.last_episode[e] = ep;
        }
        M.stamp = a.md.stamp + e * REACH_CELLS;
        M.raw = a.md.raw + e * REACH_CELLS;
        M.epoch = epoch;
    }
    return M;
}

__global__ __launch_bounds__(256) void npp_reward_kernel(RewardArgs a) {
    const int env = blockIdx.x * 256 + threadIdx.x;
    if (env >= a.n) return;
    const size_t N = (size_t)a.n, e = (size_t)env;
    // everything that depends on the env index alone
    const int lvl = a.env_level[e];
    const double px = a.f64[(size_t)F_X * N + e], py = a.f64[(size_t)F_Y * N + e];
    const unsigned flags = a.flags[e];
    const int frames = a.frames[e];
    const uint32_t word_e = a.u32[(size_t)U_E * N + e];
    RewardState S;
    reward_state_load(a, N, e, S);
    // the level's headers
    const LevelHdr &L = a.hdr[lvl];
    const ReachHdr &H = a.rh[lvl];
    const int obs_switch = L.obs_switch;
    const RewardLevel RL = a.rl[lvl];
    const RewardParams P{a.params[0], a.params[1], a.params[2], a.params[3], a.params[4], a.params[5]};
    const ReachTabs T{&H, a.rblob + H.base};
    const int sw_now = exit_switch_activated(exit_switch_state(a.ent_bits, N, e, obs_switch)) ? 1 : 0;
    ReachMiss M = reward_shared_dictionary(a, e, word_e);
    ReachMiss M2{a.stamp2 ? a.stamp2 + e * REACH_CELLS : nullptr, a.raw2 ? a.raw2 + e * REACH_CELLS : nullptr, 1u};
    // (waypoints on: the bonus npp_waypoint_kernel wrote for this step; off: the rule takes the path it took without the option)
    double wp_bonus = 0.0;
    if (a.wp_bonus) wp_bonus = a.wp_bonus[e];
    const RewardOut o = reward_step(T, RL, P, S, px, py, sw_now, flags, frames, (unsigned)a.end_bits, &M, &M2, a.wp_bonus != nullptr, wp_bonus);
    reward_state_store(a, N, e, S);
    a.reward[e] = (float)o.reward;
    if (a.comps) {
        float *c = a.comps + e * 6;
        c[0] = (float)o.pbrs; c[1] = (float)o.dist_milestone; c[2] = (float)o.switch_milestone; c[3] = (float)o.approach;
        c[4] = (float)o.terminal; c[5] = (float)o.potential;
    }
    if (a.status) a.status[e] = o.kind;
}

// an episode start outside the step kernel (npp_reset, a level assignment, a restore, a state injection) or the mode being switched
// on (`init`): the reward state of the envs under the mask (null = all) restarts on the state they are in, which is observed as the
// next step's prev_obs
__global__ __launch_bounds__(256) void npp_reward_restart_kernel(RewardArgs a, int init) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    int env = i;
    if (a.envs) {
        if (i >= a.count) return;
        if (a.env_status && a.env_status[i] != 0) return;
        env = a.envs[i];
        if (env < 0) return;
    }
    if (env >= a.n) return;
    if (a.mask && a.mask[env] == 0) return;
    const size_t N = (size_t)a.n, e = (size_t)env;
    const int lvl = a.env_level[e];
    const double px = a.f64[(size_t)F_X * N + e], py = a.f64[(size_t)F_Y * N + e];
    const uint32_t word_e = a.u32[(size_t)U_E * N + e];
    RewardState S;
    if (init) reward_state_init(S);
    else reward_state_load(a, N, e, S);
    const LevelHdr &L = a.hdr[lvl];
    const ReachHdr &H = a.rh[lvl];
    const ReachTabs T{&H, a.rblob + H.base};
    const int sw_now = exit_switch_activated(exit_switch_state(a.ent_bits, N, e, L.obs_switch)) ? 1 : 0;
    ReachMiss M = reward_shared_dictionary(a, e, word_e);
    reward_restart(S);
    reward_observe(T, S, px, py, sw_now, &M);
    S.bits = (S.bits & ~RW_PREV_SWITCH) | (sw_now ? RW_PREV_SWITCH : 0u);
    reward_state_store(a, N, e, S);
}

}  // namespace

hipError_t launch_reward(const RewardArgs &a, hipStream_t s) {
    if (a.n <= 0) return hipSuccess;
    hipLaunchKernelGGL(npp_reward_kernel, dim3((a.n + 255) / 256), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_reward_restart(const RewardArgs &a, int init, hipStream_t s) {
    const int lanes = a.envs ? a.count : a.n;
    if (lanes <= 0) return hipSuccess;
    hipLaunchKernelGGL(npp_reward_restart_kernel, dim3((lanes + 255) / 256), dim3(256), 0, s, a, init);
    return hipGetLastError();
}

}  // namespace npp
