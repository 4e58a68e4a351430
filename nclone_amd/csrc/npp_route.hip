// npp_route.hip -- action routes (include/npp_amd.h, npp_set_routes): the append that runs behind every step launch and the
// events of the other entry points (reset, raw ticks, a new level set).  The rule is npp_route.hpp's; these kernels only fetch its
// inputs.  One thread per env: the env's header (13 live words) is held in registers, the rows of the launch are walked in
// order, and at most one byte per row is stored.  The step kernels know nothing of this: the append reads the flags and frames
// rows they wrote.
#include <hip/hip_runtime.h>

#include "npp_internal.hpp"
#include "npp_route.hpp"

namespace npp {
namespace {

constexpr int LIVE_WORDS = ROUTE_CUR + 1;   // words 13-15 are always 0

__global__ __launch_bounds__(256) void npp_route_append_kernel(RouteArgs a) {
    const int env = blockIdx.x * 256 + threadIdx.x;
    if (env >= a.n) return;
    if (a.phase && a.phase_id >= 0 && a.phase[env] != (uint8_t)a.phase_id) return;   // stepped by another part of a split launch
    int32_t *row = a.hdr + (size_t)env * ROUTE_HDR_WORDS;
    int32_t h[ROUTE_HDR_WORDS];
#pragma unroll
    for (int k = 0; k < LIVE_WORDS; k++) h[k] = row[k];
    uint8_t *bufs = a.act + (size_t)env * 2 * a.cap;
    const int level = a.env_level[env];
    for (int s = 0; s < a.n_steps; s++) {
        const size_t o = (size_t)s * a.n + env;
        route_step(h, bufs, a.cap, a.actions[o], a.flags[o], a.frames[o], a.frame_skip, level, a.autoreset != 0);
    }
#pragma unroll
    for (int k = 0; k < LIVE_WORDS; k++) row[k] = h[k];
}

__global__ __launch_bounds__(256) void npp_route_event_kernel(RouteArgs a, int event) {
    const int env = blockIdx.x * 256 + threadIdx.x;
    if (env >= a.n) return;
    if (a.mask && a.mask[env] == 0) return;
    int32_t *row = a.hdr + (size_t)env * ROUTE_HDR_WORDS;
    if (event == ROUTE_EV_TICK) { route_tick(row); return; }
    int32_t h[ROUTE_HDR_WORDS];
    if (event == ROUTE_EV_INIT) {
        route_init(h);
#pragma unroll
        for (int k = 0; k < ROUTE_HDR_WORDS; k++) row[k] = h[k];
        return;
    }
#pragma unroll
    for (int k = 0; k < LIVE_WORDS; k++) h[k] = row[k];
    if (route_empty(h)) return;
    route_flip(h);
#pragma unroll
    for (int k = 0; k < LIVE_WORDS; k++) row[k] = h[k];
}

}  // namespace

hipError_t launch_route_append(const RouteArgs &a, hipStream_t s) {
    if (a.n <= 0 || a.n_steps <= 0) return hipSuccess;
    hipLaunchKernelGGL(npp_route_append_kernel, dim3((a.n + 255) / 256), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_route_event(const RouteArgs &a, int event, hipStream_t s) {
    if (a.n <= 0) return hipSuccess;
    hipLaunchKernelGGL(npp_route_event_kernel, dim3((a.n + 255) / 256), dim3(256), 0, s, a, event);
    return hipGetLastError();
}

}  // namespace npp
