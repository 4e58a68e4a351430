// npp_stack.hip -- frame stacking of player_frame and game_state (the reference's FrameStackWrapper,
// nclone/gym_environment/frame_stack_wrapper.py:183-224 reset padding, 313-400 observation()) on handle-owned rings.
//
// Ring layout (per env, per stacked key of K entries of E elements): 2 K slots; the entry at ring position q lives in slots q
// AND q + K.  With `head` the position of the newest entry, the window [oldest .. newest] is slots head + 1 .. head + K:
// contiguous for every head, so the host hands it out as a strided view without copying (include/npp_amd.h,
// npp_frame_stack_view).  The frame ring's newest entry is written by npp_render_kernel itself (batch stride 2 K * 7056 and
// a mirror copy K * 7056 further on); this kernel does the rest of a push:
//   - game_state of this step -> state slots head and head + K;
//   - terminal_game_state_stack: the old window's last K - 1 entries, then terminal_state (reset env) or game_state;
//   - envs reset in this step: the K - 1 older window entries of both rings <- padding (zeros, or the newest entry).
// Bytes per push at N envs: N * 41 * 4 * (1 + 2 + (K - 1) + K) for the state ring and the terminal stack (13 MB at K = 4,
// N = 8192), plus 2 (K - 1) * 7056 written (and 7056 read for "repeat") per reset env for frames.
#include <hip/hip_runtime.h>

#include "npp_internal.hpp"

namespace npp {
namespace {

constexpr int GS = 41;               // NPP_GAME_STATE_DIM
constexpr int FRAME = 84 * 84;       // bytes of one player_frame entry
constexpr int FRAME_V = FRAME / 16;  // 441 uint4 per entry

// one wavefront per env: lanes 0..40 own one game_state column each, all 64 lanes pad the frame ring of a reset env
__global__ __launch_bounds__(64) void npp_stack_kernel(StackArgs a) {
    const int env = blockIdx.x;
    if (env >= a.n) return;
    const int lane = threadIdx.x;
    const bool reset = a.reset_all || (a.flags && (a.flags[env] & a.reset_bits) != 0);
    if (a.state_k && lane < GS) {
        const int K = a.state_k, p = a.shead;
        float *ring = a.state + (size_t)env * 2 * K * GS + lane;
        const float cur = a.game_state[(size_t)env * GS + lane];
        if (a.terminal_stack) {
            // read before this push writes anything: the previous window is slots p .. p + K - 1, its last K - 1 entries p + 1 ..
            float *ts = a.terminal_stack + (size_t)env * K * GS + lane;
            for (int i = 0; i < K - 1; i++) ts[i * GS] = ring[(p + 1 + i) * GS];
            ts[(K - 1) * GS] = reset ? a.terminal_state[(size_t)env * GS + lane] : cur;
        }
        ring[p * GS] = cur;
        ring[(p + K) * GS] = cur;
        if (reset) {
            const float pad = a.repeat ? cur : 0.f;
            for (int i = 1; i < K; i++) {
                const int q = p + i < K ? p + i : p + i - K;
                ring[q * GS] = pad;
                ring[(q + K) * GS] = pad;
            }
        }
    }
    if (a.visual_k > 1 && reset) {
        const int K = a.visual_k, p = a.vhead;
        uint4 *ring = reinterpret_cast<uint4 *>(a.frames + (size_t)env * 2 * K * FRAME);
        const uint4 *src = ring + (size_t)(p + K) * FRAME_V;   // the newest entry (the render kernel wrote it)
        for (int v = lane; v < FRAME_V; v += 64) {
            const uint4 pad = a.repeat ? src[v] : make_uint4(0u, 0u, 0u, 0u);
            for (int i = 1; i < K; i++) {
                const int q = p + i < K ? p + i : p + i - K;
                if (q) ring[(size_t)q * FRAME_V + v] = pad;   // slot 0 is never inside a window
                ring[(size_t)(q + K) * FRAME_V + v] = pad;
            }
        }
    }
}

}  // namespace

hipError_t launch_stack_push(const StackArgs &a, hipStream_t s) {
    hipLaunchKernelGGL(npp_stack_kernel, dim3(a.n), dim3(64), 0, s, a);
    return hipGetLastError();
}

}  // namespace npp
