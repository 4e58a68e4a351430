// npp_demo.hip -- demonstration transitions from recorded replays (include/npp_amd.h, npp_demo_create / npp_demo_play; the plan:
// npp_demo.hpp).  Two kernels around the existing tick and observation launches of one period:
//   npp_demo_feed_kernel     reads the ragged input table at every env's own cursor and writes the [fs][n] staging rows npp_tick reads
//   npp_demo_collect_kernel  moves every env's observation row from the player's rows (one per env) to its place in the packed
//                            dataset (one per transition) and writes the per-row columns
// The step kernels know nothing of this.
#include <hip/hip_runtime.h>

#include "npp_demo.hpp"
#include "npp_internal.hpp"

namespace npp {
namespace {

// one thread per (tick of the period, env)
__global__ __launch_bounds__(256) void npp_demo_feed_kernel(DemoArgs a) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= a.fs * a.n) return;
    const int k = idx / a.n, e = idx - k * a.n;
    const int r = a.slot[e];
    uint8_t b = 0;   // an idle env, and every tick past a replay's end
    if (r >= 0) {
        const int64_t o = a.offsets[r], len = a.offsets[r + 1] - o;
        const int64_t c = (int64_t)a.period * a.fs + k;
        if (c < len) b = a.inputs[o + c];
    }
    a.staging[idx] = b;
}

// consecutive lanes move consecutive elements of ONE row: a coalesced load of the env's row, a coalesced store of the dataset's
template <class T> __device__ inline void move_row(T *dst, const T *src, int64_t row, int env, int dim, int lane) {
    if (!dst) return;
    for (int i = lane; i < dim; i += WAVE) dst[row * dim + i] = src[(size_t)env * dim + i];
}

constexpr int COLLECT_WAVES = 4;

// One wavefront per env.  An env without a replay in this round, or whose replay has no row in this period, writes nothing; every
// destination element is written by exactly one lane; no atomics.
__global__ __launch_bounds__(COLLECT_WAVES * WAVE) void npp_demo_collect_kernel(DemoArgs a) {
    const int lane = threadIdx.x & (WAVE - 1);
    const int e = blockIdx.x * COLLECT_WAVES + (threadIdx.x >> 6);
    if (e >= a.n) return;
    const int r = a.slot[e];
    if (r < 0) return;
    const int rows = a.rows[r];
    if (a.period >= rows) return;
    const int64_t row = a.row_base[r] + a.period;
    const int64_t o = a.offsets[r], len = a.offsets[r + 1] - o;
    const int64_t f = (int64_t)(a.period + 1) * a.fs - 1;   // the tick the row is sampled after
    const DemoOut &d = a.out;
    if (d.game_state) {
        if (lane < 40) d.game_state[row * 41 + lane] = a.gs[(size_t)e * 41 + lane];
        // the executor's own time value (replay_executor.py:537-544): max(0, (L - sim.frame) / L), sim.frame = f + 1, in fp64,
        // rounded once by the float32 cast of the array
        if (lane == 40) d.game_state[row * 41 + 40] = (float)fmax(0.0, (double)(len - (f + 1)) / (double)len);
    }
    if (d.action_mask && lane < 6) d.action_mask[row * 6 + lane] = a.mask_ones ? (int8_t)1 : a.mask[(size_t)e * 6 + lane];
    move_row(d.entity_positions, a.epos, row, e, 6, lane);
    move_row(d.spatial_context, a.sc, row, e, 112, lane);
    move_row(d.reachability_features, a.reach, row, e, 38, lane);
    move_row(d.mine_sdf_features, a.sdf, row, e, 3, lane);
    move_row(d.switch_states, a.sw, row, e, 25, lane);
    move_row(d.positions, a.pos, row, e, 6, lane);
    // the per-row columns, one lane each
    if (lane == 0 && d.action) d.action[row] = demo_action_of_byte(a.inputs[o + f]);   // (npp_demo.hpp)
    if (lane == 1 && d.frame) d.frame[row] = (int32_t)f;
    if (lane == 2 && d.done) d.done[row] = a.period == rows - 1 ? 1 : 0;
    if (lane == 3 && d.replay) d.replay[row] = r;
    if (lane == 4 && d.level) d.level[row] = a.rep_level[r];
    if (lane == 5 && d.flags) d.flags[row] = a.flags[e] & 7u;   // NPP_F_WON | NPP_F_DEAD | NPP_F_SWITCH
    if (lane == 6 && d.status) d.status[row] = a.rstatus ? a.rstatus[e] : 0;
}

}  // namespace

hipError_t launch_demo_feed(const DemoArgs &a, hipStream_t s) {
    if (a.n <= 0 || a.fs <= 0) return hipSuccess;
    hipLaunchKernelGGL(npp_demo_feed_kernel, dim3((a.fs * a.n + 255) / 256), dim3(256), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_demo_collect(const DemoArgs &a, hipStream_t s) {
    if (a.n <= 0) return hipSuccess;
    hipLaunchKernelGGL(npp_demo_collect_kernel, dim3((a.n + COLLECT_WAVES - 1) / COLLECT_WAVES), dim3(COLLECT_WAVES * WAVE), 0, s, a);
    return hipGetLastError();
}

}  // namespace npp
