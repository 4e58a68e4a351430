// Stand-alone driver of npp_demo_plan_host for a build with g++ -fsanitize=address,undefined: tests/test_demo_host.py compiles it
// TOGETHER with the host sources into one executable with the sanitizer runtimes linked statically and runs it as a program of its
// own -- no sanitizer runtime is loaded into Python.
//   demo_sanitized_main SETS   (raw little-endian int64: per set  n_replays, frame_skip, max_transitions, n_envs, then n_replays lengths)
// prints per set: rc, rows_total, scheduled, rounds, then rows / row_base / order / round_ticks, one line each.  Every output array
// is an allocation of exactly n_replays elements, so an overrun is the sanitizer's to see.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "npp_amd.h"

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    std::vector<int64_t> v;
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    int64_t x;
    while (std::fread(&x, sizeof(x), 1, f) == 1) v.push_back(x);
    std::fclose(f);
    size_t at = 0;
    while (at + 4 <= v.size()) {
        const int n = (int)v[at], fs = (int)v[at + 1], n_envs = (int)v[at + 3];
        const int64_t cap = v[at + 2];
        at += 4;
        if (n < 0 || at + (size_t)n > v.size()) return 2;
        std::vector<int64_t> len(v.begin() + at, v.begin() + at + n);
        at += (size_t)n;
        std::vector<int32_t> rows((size_t)n, -7), order((size_t)n, -7), ticks((size_t)n, -7);
        std::vector<int64_t> base((size_t)n, -7);
        int32_t counts[2] = {-7, -7};
        int64_t total = -7;
        const int rc = npp_demo_plan_host(len.data(), n, fs, cap, n_envs, rows.data(), base.data(), order.data(), ticks.data(), counts, &total);
        std::printf("%d %lld %d %d\n", rc, (long long)total, (int)counts[0], (int)counts[1]);
        for (int k = 0; k < n; k++) std::printf("%d ", (int)rows[k]);
        std::printf("\n");
        for (int k = 0; k < n; k++) std::printf("%lld ", (long long)base[k]);
        std::printf("\n");
        for (int k = 0; k < n; k++) std::printf("%d ", (int)order[k]);
        std::printf("\n");
        for (int k = 0; k < n; k++) std::printf("%d ", (int)ticks[k]);
        std::printf("\n");
    }
    return 0;
}
