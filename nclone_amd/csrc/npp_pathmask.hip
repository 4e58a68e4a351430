// npp_pathmask.hip -- path-direction action masking (include/npp_amd.h, npp_set_action_masking / npp_path_action_mask): the
// reference env's per-observation detector and the "hard" mask stage, for every env, behind the launch that produced the
// observation.  The rule is npp_pathmask.hpp's; this kernel fetches its inputs and keeps the two counters.
// One lane per env, 256-lane blocks, no LDS.  A lane's work is a chain of dependent loads: (level id, x, y, the six mask bytes,
// the counters, the flags byte -- all independent, all coalesced across lanes: SoA planes and byte rows of consecutive envs) ->
// (the level's LevelHdr::obs_switch and its ReachHdr) -> (the switch's entity word; the four node records of reach_near, issued
// together) -> for the exit-door goal one entry of off_mh.  Bytes per env: 16 position + 4 level + 4 entity word + 192 records
// (+ 16) + 6 mask in / out + 16 counters in / out + 1 flags + 1 direction ~ 260 B -> 2.1 MB per launch at 8192 envs: latency bound.
#include <hip/hip_runtime.h>

#include "npp_internal.hpp"
#include "npp_pathmask.hpp"

namespace npp {
namespace {

__global__ __launch_bounds__(256) void npp_path_mask_kernel(PathMaskArgs a) {
    const int env = blockIdx.x * 256 + threadIdx.x;
    if (env >= a.n) return;
    const size_t N = (size_t)a.n, e = (size_t)env;
    // everything that depends on the env index alone
    const int lvl = a.env_level[e];
    const double px = a.f64[(size_t)F_X * N + e], py = a.f64[(size_t)F_Y * N + e];
    uint32_t observed = a.observed[e], applied = a.applied[e];
    const bool ended = a.flags && (a.flags[e] & a.end_bits) != 0;
    int8_t *mrow = a.mask ? a.mask + e * 6 : nullptr;
    int8_t m[6] = {0, 0, 0, 0, 0, 0};
    if (mrow) {
#pragma unroll
        for (int k = 0; k < 6; k++) m[k] = mrow[k];
    }
    // the level's headers
    const LevelHdr &L = a.hdr[lvl];
    const ReachHdr &H = a.rh[lvl];
    const int obs_switch = L.obs_switch;
    const ReachTabs T{&H, a.rblob + H.base};
    const int sw = exit_switch_activated(exit_switch_state(a.ent_bits, N, e, obs_switch));
    int from_graph = 0;
    const int dir = reach_path_direction(T, px, py, sw, &from_graph);
    if (a.dir) a.dir[e] = (int8_t)dir;
    if (a.status) a.status[e] = from_graph;
    if (mrow) {
        const unsigned keep = path_keep_mask(dir);
#pragma unroll
        for (int k = 0; k < 6; k++) mrow[k] = ((keep >> k) & 1u) ? m[k] : (int8_t)0;
    }
    // counters: the step before this observation ended the env's episode (and auto-reset it) -> latch, restart at this observation
    if (ended) {
        a.last_observed[e] = observed;
        a.last_applied[e] = applied;
        observed = 0u; applied = 0u;
    }
    a.observed[e] = observed + 1u;
    a.applied[e] = applied + (uint32_t)from_graph;
}

// a reset through npp_reset: the live counters of the envs under the mask (null = all) restart
__global__ __launch_bounds__(256) void npp_path_mask_restart_kernel(int n, const uint8_t *mask, uint32_t *observed, uint32_t *applied) {
    const int env = blockIdx.x * 256 + threadIdx.x;
    if (env >= n) return;
    if (mask && mask[env] == 0) return;
    observed[env] = 0u;
    applied[env] = 0u;
}

}  // namespace

hipError_t launch_path_mask(const PathMaskArgs &a, hipStream_t s) {
    if (a.n <= 0) return hipSuccess;
    hipLaunchKernelGGL(npp_path_mask_kernel, dim3((a.n + 255) / 256), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_path_mask_restart(int n, const uint8_t *mask, uint32_t *observed, uint32_t *applied, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    hipLaunchKernelGGL(npp_path_mask_restart_kernel, dim3((n + 255) / 256), dim3(256), 0, s, n, mask, observed, applied);
    return hipGetLastError();
}

}  // namespace npp
