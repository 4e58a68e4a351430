// npp_pool.hpp -- the level pool's draw (include/npp_amd.h, npp_set_level_pool), shared by the device kernel (npp_pool.hip) and
// the host-only entry point (npp_host.cpp).  No HIP header: the host side also builds with plain g++.
#pragma once
#include <cstdint>

#include "npp_state.hpp"   // NPP_HD

namespace npp {

// one splitmix64 round
NPP_HD inline uint64_t pool_mix(uint64_t z) {
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// the level env `env` draws with draw count `count`: cdf[l] = w[0] + ... + w[l] (f64, index order), last = the last level of
// non-zero weight
NPP_HD inline int pool_pick(const double *cdf, int n, int last, uint64_t seed, uint32_t env, uint32_t count) {
    const uint64_t u = pool_mix(pool_mix(((uint64_t)env << 32) | count) ^ seed);
    const double t = (double)(u >> 11) * (1.0 / 9007199254740992.0) * cdf[n - 1];
    int lo = 0, hi = n;   // first l with cdf[l] > t
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (cdf[mid] <= t) lo = mid + 1;
        else hi = mid;
    }
    return lo < n ? lo : last;
}

}  // namespace npp
