// npp_pool.hip -- the level pool (include/npp_amd.h, npp_set_level_pool): after a step, every env whose episode ended draws its
// next level (EnvMapLoader.load_map, env_map_loader.py:111-208).  This kernel only draws and writes the assignment; the envs that
// changed level are then reset by npp_reset_kernel and observed by the step kernel's observe launch, both with the device mask
// it writes (npp_capi.cpp: pool_redraw).  One thread per env; 12 + 4 bytes read and at most 13 written per env.
#include <hip/hip_runtime.h>

#include "npp_internal.hpp"
#include "npp_pool.hpp"

namespace npp {
namespace {

__global__ __launch_bounds__(256) void npp_pool_draw_kernel(PoolArgs a) {
    const int env = blockIdx.x * 256 + threadIdx.x;
    if (env >= a.n) return;
    uint8_t changed = 0;
    if (a.flags[env] & a.bits) {
        const uint32_t c = a.count[env];
        const int l = pool_pick(a.cdf, a.n_levels, a.last, a.seed, (uint32_t)env, c);
        a.count[env] = c + 1u;
        if (l != a.env_level[env]) {
            a.env_level[env] = l;
            if (a.level_trunc) a.trunc[env] = a.level_trunc[l];
            changed = 1;
        }
    }
    a.changed[env] = changed;
}

}  // namespace

hipError_t launch_pool_draw(const PoolArgs &a, hipStream_t s) {
    hipLaunchKernelGGL(npp_pool_draw_kernel, dim3((a.n + 255) / 256), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace npp
