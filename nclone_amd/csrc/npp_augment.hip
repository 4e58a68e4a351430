// npp_augment.hip -- frame augmentation of player_frame and global_view (include/npp_amd.h, npp_set_frame_augmentation; the
// reference's FrameStackWrapper.observation -> frame_augmentation.apply_augmentation, frame_stack_wrapper.py:343-377, 402-462).
//
// One launch covers both targets: a workgroup per (env, frame) -- the K frames of the env's player_frame window (or its one
// unstacked frame), then its global_view.  The K frames of an env share the player_frame draw (_apply_consistent_augmentation).
// Sources (frame ring / output block) are only read; the results go to buffers of the handle.
//   - a frame whose gate mask is empty is a straight 16-byte copy (global to global);
//   - any other frame is staged in LDS with 16-byte loads (7056 B or 17 600 B) and every lane produces 4 consecutive output
//     bytes of one row (both widths are multiples of 4) from at most 4 source bytes each, stored as one dword.
// The per-pixel function and the draw are npp_augment.hpp's, the code the host entry point compiles.
// Bytes per launch at N envs, K frames: N * (K * 7056 + 17 600) read and as many written (0.75 GB at N = 8192, K = 4).
#include <hip/hip_runtime.h>

#include "npp_augment.hpp"
#include "npp_internal.hpp"

namespace npp {
namespace {

constexpr int AUG_THREADS = 256;

template <int H, int W>
__device__ __forceinline__ void augment_frame(const uint8_t *src, uint8_t *dst, const AugParams &P, uint8_t *lds) {
    static_assert(H * W % 16 == 0 && W % 4 == 0, "frames are whole uint4s, rows whole dwords");
    constexpr int V = H * W / 16, D = H * W / 4, RW = W / 4;
    const uint4 *s4 = reinterpret_cast<const uint4 *>(src);
    if (P.mask == 0) {   // (uniform over the workgroup)
        uint4 *d4 = reinterpret_cast<uint4 *>(dst);
        for (int v = threadIdx.x; v < V; v += AUG_THREADS) d4[v] = s4[v];
        return;
    }
    uint4 *l4 = reinterpret_cast<uint4 *>(lds);
    for (int v = threadIdx.x; v < V; v += AUG_THREADS) l4[v] = s4[v];
    __syncthreads();
    uint32_t *d32 = reinterpret_cast<uint32_t *>(dst);
    for (int d = threadIdx.x; d < D; d += AUG_THREADS) {
        const int y = d / RW, x = (d - y * RW) * 4;
        uint32_t o = 0;
#pragma unroll
        for (int i = 0; i < 4; i++) o |= (uint32_t)aug_pixel(lds, H, W, P, y, x + i) << (8 * i);
        d32[d] = o;
    }
}

__global__ __launch_bounds__(AUG_THREADS) void npp_augment_kernel(AugArgs a) {
    __shared__ __attribute__((aligned(16))) uint8_t lds[AUG_GV_H * AUG_GV_W];
    const int per = a.k + 1;   // workgroups per env: its k player_frame entries, then global_view
    const int env = blockIdx.x / per, slot = blockIdx.x - env * per;
    if (env >= a.n) return;
    const int target = slot == a.k ? 1 : 0;
    AugParams P;
    if (a.params) {
        const int32_t *w = a.params + ((size_t)env * 2 + target) * AUG_WORDS;
        P.mask = w[0]; P.sx = w[1]; P.sy = w[2]; P.holes = w[3];
        for (int i = 0; i < 8; i++) P.hole[i >> 2][i & 3] = w[4 + i];
        P.a = w[12]; P.b = w[13];
    } else {
        P = aug_draw(a.seed, (uint32_t)env, a.count, target, a.p, a.s10);
    }
    if (target) {
        constexpr size_t E = (size_t)AUG_GV_H * AUG_GV_W;
        augment_frame<AUG_GV_H, AUG_GV_W>(a.gv_src + (size_t)env * E, a.gv_dst + (size_t)env * E, P, lds);
    } else {
        constexpr size_t E = (size_t)AUG_PF_H * AUG_PF_W;
        augment_frame<AUG_PF_H, AUG_PF_W>(a.pf_src + (size_t)env * a.pf_stride + (size_t)slot * E,
                                          a.pf_dst + ((size_t)env * a.k + slot) * E, P, lds);
    }
}

}  // namespace

hipError_t launch_frame_augment(const AugArgs &a, hipStream_t s) {
    hipLaunchKernelGGL(npp_augment_kernel, dim3((unsigned)a.n * (unsigned)(a.k + 1)), dim3(AUG_THREADS), 0, s, a);
    return hipGetLastError();
}

}  // namespace npp
