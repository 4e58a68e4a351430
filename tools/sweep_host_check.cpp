// sweep_host_check.cpp -- a stand-alone driver of npp_sweep_assign_host (include/npp_amd.h; the rule: nclone_amd/csrc/npp_sweep.hpp)
// for a sanitized CPU build: zero-length rows, J at and past next, n not a multiple of 64, idle envs, a dry list.  No GPU, no Python.
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -I include tools/sweep_host_check.cpp \
//       nclone_amd/csrc/npp_host.cpp nclone_amd/csrc/npp_level.cpp nclone_amd/csrc/npp_reach.cpp -o sweep_host_check && ./sweep_host_check
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "npp_amd.h"

#define CHECK(c)                                                          \
    do {                                                                  \
        if (!(c)) {                                                       \
            std::fprintf(stderr, "%s:%d: %s failed\n", __FILE__, __LINE__, #c); \
            return 1;                                                     \
        }                                                                 \
    } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(rng_state >> 33);
}

int main() {
    const int end_bits = 1 | 2 | 8;
    {   // zero-length row: heap arrays of size zero must not be touched
        std::vector<int32_t> jobs(3, 0), counters = {3, 0, 3};
        std::vector<uint8_t> flags, changed;
        std::vector<int32_t> env_job, prev, level;
        CHECK(npp_sweep_assign_host(flags.data(), end_bits, 0, jobs.data(), 3, counters.data(), env_job.data(), prev.data(), level.data(),
                                    nullptr, nullptr, 0, changed.data()) == NPP_OK);
        CHECK(counters[0] == 3);
        counters = {0, 0, 0};
        CHECK(npp_sweep_assign_host(nullptr, end_bits, 0, nullptr, 0, counters.data(), nullptr, nullptr, nullptr, nullptr, nullptr, 0, nullptr) ==
              NPP_OK);
    }
    const int sizes[] = {1, 63, 64, 65, 257, 1025};
    for (int n : sizes) {
        for (int variant = 0; variant < 3; variant++) {
            // the list is as long as the first hand-out (J == next at the start) | one longer | much longer
            const int n_levels = 5, J = variant == 0 ? n : variant == 1 ? n + 1 : 4 * n + 3;
            std::vector<int32_t> jobs(J), level_trunc(n_levels), env_job(n), prev(n, -1), level(n), trunc(n, 100), counters = {n, 0, J};
            for (auto &j : jobs) j = (int32_t)(rnd() % n_levels);
            for (auto &t : level_trunc) t = 40 + (int32_t)(rnd() % 100);
            for (int e = 0; e < n; e++) { env_job[e] = e; level[e] = jobs[e]; trunc[e] = level_trunc[jobs[e]]; }
            std::vector<uint8_t> flags(n), changed(n);
            int handed = n, finished = 0;
            for (int step = 0; step < 8; step++) {
                int ending = 0;
                for (int e = 0; e < n; e++) {
                    flags[e] = (uint8_t)((rnd() % 3 == 0 ? (1u << (rnd() % 2)) | (rnd() % 2 ? 8u : 0u) : 0u) | (rnd() % 2 ? 4u : 0u));
                    ending += (flags[e] & end_bits) && env_job[e] >= 0;
                }
                CHECK(npp_sweep_assign_host(flags.data(), end_bits, n, jobs.data(), J, counters.data(), env_job.data(), prev.data(), level.data(),
                                            trunc.data(), level_trunc.data(), n_levels, changed.data()) == NPP_OK);
                handed += ending;
                CHECK(counters[0] == handed);
                for (int e = 0; e < n; e++) {
                    CHECK(env_job[e] >= -1 && env_job[e] < J);
                    if (env_job[e] >= 0) CHECK(level[e] == jobs[env_job[e]] && trunc[e] == level_trunc[level[e]]);
                    if (prev[e] >= 0) { finished++; prev[e] = -1; }
                }
            }
            CHECK(finished == handed - n);
        }
    }
    std::printf("sweep_host_check: ok\n");
    return 0;
}
