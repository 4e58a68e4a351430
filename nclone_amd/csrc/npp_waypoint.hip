// npp_waypoint.hip -- reward mode "pbrs", sequential path waypoints (include/npp_amd.h, npp_set_reward_waypoints): the bonus of the
// step for every env, in a launch of its own behind the step and IN FRONT of npp_reward_kernel, which adds it where the reference
// does.  The rule is npp_waypoint.hpp's; this kernel fetches its inputs, runs it and stores the env's waypoint state back.
// One lane per env, 256-lane blocks, no LDS.  A lane's work: (flags byte, next expected, collected count, level id, x, y -- all
// coalesced across lanes) -> on a live step the level's header, the CSR starts of the 3 x 3 cells of 24 px around the ninja (three
// runs of up to four consecutive u16) and, per entry of those cells, one record and, only when it lies within the radius, one word of
// the env's collected set.  Waypoints stand 12 px apart along a path, so a cell holds a handful.  Bytes per env: 1 + 8 + 4 + 16 in,
// ~100 table, 8-20 out: latency bound, like npp_reward_kernel, and a fraction of its traffic.
#include <hip/hip_runtime.h>

#include "npp_internal.hpp"
#include "npp_waypoint.hpp"

namespace npp {
namespace {

__global__ __launch_bounds__(256) void npp_waypoint_kernel(WaypointArgs a) {
    const int env = blockIdx.x * 256 + threadIdx.x;
    if (env >= a.n) return;
    const size_t N = (size_t)a.n, e = (size_t)env;
    const unsigned flags = a.flags[e];
    uint32_t *st = a.state + e;   // word w of the env's state: st[w * N]
    uint32_t next = st[(size_t)WP_WORDS * N], count = st[(size_t)(WP_WORDS + 1) * N];
    const bool ended = (flags & (unsigned)a.end_bits) != 0;
    const bool live = !(flags & 3u)   /* NPP_F_WON | NPP_F_DEAD */ && !ended;
    WaypointOut o;
    o.bonus = 0.0;
    o.index = -1;
    if (live) {
        const int lvl = a.env_level[e];
        const double px = a.f64[(size_t)F_X * N + e], py = a.f64[(size_t)F_Y * N + e];
        const WaypointTabs T{a.wh + lvl, a.wblob};
        const WaypointParams P{a.params[0], a.params[1], a.params[2], 0.0};
        o = waypoint_step(T, P, st, N, next, count, px, py, (flags & 4u) ? 1 : 0   /* NPP_F_SWITCH */);
    }
    if (a.info_out) {   // (on a step that ended the episode: what the calculator held before its reset())
        int32_t *q = a.info_out + e * 3;
        q[0] = o.index; q[1] = (int32_t)next; q[2] = (int32_t)count;
    }
    if (ended) waypoint_restart(st, N, next, count);
    if (ended || o.index >= 0) {
        st[(size_t)WP_WORDS * N] = next;
        st[(size_t)(WP_WORDS + 1) * N] = count;
    }
    a.bonus[e] = o.bonus;
    if (a.bonus_out) a.bonus_out[e] = (float)o.bonus;
}

// an episode start outside the step kernel, or the waypoints being switched on: RewardCalculator.reset() for the envs under the mask
// (null = all) or in the list, as npp_reward_restart_kernel selects them
__global__ __launch_bounds__(256) void npp_waypoint_restart_kernel(WaypointArgs a) {
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
    const size_t N = (size_t)a.n;
    uint32_t next, count;
    waypoint_restart(a.state + env, N, next, count);
    a.state[(size_t)WP_WORDS * N + env] = next;
    a.state[(size_t)(WP_WORDS + 1) * N + env] = count;
}

}  // namespace

hipError_t launch_waypoint(const WaypointArgs &a, hipStream_t s) {
    if (a.n <= 0) return hipSuccess;
    hipLaunchKernelGGL(npp_waypoint_kernel, dim3((a.n + 255) / 256), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_waypoint_restart(const WaypointArgs &a, hipStream_t s) {
    const int lanes = a.envs ? a.count : a.n;
    if (lanes <= 0) return hipSuccess;
    hipLaunchKernelGGL(npp_waypoint_restart_kernel, dim3((lanes + 255) / 256), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace npp
