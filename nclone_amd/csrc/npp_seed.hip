// npp_seed.hip -- seeding the cell index from recorded replays (include/npp_amd.h, npp_archive_seed; the rows: npp_seed.hpp;
// DESIGN.md 22).  Two kernels around the existing tick, propose, assign and store launches of one tick, one thread per env:
//   npp_seed_feed_kernel   counts what the explore of the tick before decided for the env's replay, then reads the ragged input
//                          table at tick f and writes the env's rows of the coming tick: input byte, action, candidate mask,
//                          score, route-mismatch latch
//   npp_seed_route_kernel  (routes on) appends the action of a candidate's tick to the env's current route, as one step of frame
//                          skip 1 would -- without npp_tick's "not replayable" bit, which is set from the latch alone
// The step kernels and the cell kernels know nothing of this.  The counters are integer atomic adds whose return value is not
// used; an env holds one replay per round, so no counter depends on the order in which threads arrive.
#include <hip/hip_runtime.h>

#include "npp_internal.hpp"
#include "npp_route.hpp"
#include "npp_seed.hpp"

namespace npp {
namespace {

__global__ __launch_bounds__(256) void npp_seed_feed_kernel(SeedArgs a) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= a.n) return;
    const int r = a.slot[e];
    if (a.status && a.counts && r >= 0) {   // explore's verdict on the tick before: 1 = no candidate (mask byte 0)
        const int st = a.status[e];
        int32_t *c = a.counts + (size_t)r * 4;
        if (st != 1) {
            (void)__hip_atomic_fetch_add(&c[0], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (st == 0 || st == 6 || st == 7) (void)__hip_atomic_fetch_add(&c[1], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (st == 0) (void)__hip_atomic_fetch_add(&c[2], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (st == 7) (void)__hip_atomic_fetch_add(&c[3], 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    if (!a.feed) return;
    uint8_t b = 0, cand = 0;   // an idle env, and every tick past a replay's end: zero input, never a candidate
    float score = 0.f;
    uint8_t latch = a.tick == 0 ? (uint8_t)0 : a.latch[e];
    if (r >= 0) {
        const int64_t o = a.offsets[r], len = a.offsets[r + 1] - o;
        if (a.tick < len) {
            b = a.inputs[o + a.tick];
            cand = 1;
            score = a.score_mode == SEED_TABLE ? a.scores[o + a.tick] : seed_score(a.score_mode, a.tick, len);
            if (seed_byte_mismatch(b)) latch = 1;
        }
    }
    a.staging[e] = b;
    a.action[e] = demo_action_of_byte(b);
    a.mask[e] = cand;
    a.score[e] = score;
    a.latch[e] = latch;
}

// The header update is route_step's (npp_route.hpp) for one executed frame at frame skip 1; R_FRAMES counts the ticks, so it is
// f + 1 whatever the capacity dropped.
__global__ __launch_bounds__(256) void npp_seed_route_kernel(SeedArgs a) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= a.n || !a.mask[e]) return;
    const size_t N = (size_t)a.n;
    const int level = a.env_level[e];
    const int state = state_load(a.u32, N, e, S_STATE), cause = state_load(a.u32, N, e, S_CAUSE);
    const bool sw = exit_switch_activated(exit_switch_state(a.ent, N, e, a.hdr[level].obs_switch));
    const int flags = (state == 8 ? 1 : 0) | (state == 6 || state == 7 ? 2 : 0) | (sw ? 4 : 0) | (cause == 1 ? 16 : 0) | (cause == 2 ? 32 : 0);
    int32_t *h = a.route_hdr + (size_t)e * ROUTE_HDR_WORDS;
    route_step(h, a.route_act + (size_t)e * 2 * a.cap, a.cap, a.action[e], flags, 1, 1, level, false);
    if (a.latch[e]) h[R_BITS] |= ROUTE_BROKEN;
}

}  // namespace

hipError_t launch_seed_feed(const SeedArgs &a, hipStream_t s) {
    if (a.n <= 0) return hipSuccess;
    hipLaunchKernelGGL(npp_seed_feed_kernel, dim3((a.n + 255) / 256), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_seed_route(const SeedArgs &a, hipStream_t s) {
    if (a.n <= 0 || a.cap <= 0) return hipSuccess;
    hipLaunchKernelGGL(npp_seed_route_kernel, dim3((a.n + 255) / 256), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace npp
