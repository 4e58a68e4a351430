// Stand-alone driver of the goal curriculum's host-only entries (npp_goal_stages_host, npp_compile_level_segments_goal,
// npp_compile_level_entities_goal, npp_goal_apply_host) for a build with g++ -fsanitize=address,undefined:
// tests/test_goal_host.py compiles it TOGETHER with the host sources (npp_level.cpp, npp_reach.cpp, npp_host.cpp) into one
// executable with the sanitizer runtimes linked statically and runs it as a program of its own -- no sanitizer runtime is loaded
// into Python.
//   goal_sanitized_main MAP INTERVAL   (raw little-endian f64 map)
// prints the stage table (hex floats), compiles the variant of every stage, runs the bookkeeping rule on a small stream, then calls
// the entries on truncated copies of the map and on one whose entity counts lie.  Every buffer is exactly as large as the entry is told.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "npp_amd.h"

template <class T> static std::vector<T> slurp(const char *path) {
    std::vector<T> v;
    FILE *f = std::fopen(path, "rb");
    if (!f) { std::fprintf(stderr, "cannot open %s\n", path); std::exit(2); }
    T x;
    while (std::fread(&x, sizeof(T), 1, f) == 1) v.push_back(x);
    std::fclose(f);
    return v;
}

static int variants(const std::vector<double> &map, double interval, bool print) {
    int32_t ns = -1, plen[2] = {-1, -1};
    double dist[3], orig[4];
    const int stage_cap = 3, path_cap = 5;   // smaller than the tables: the entry must stop at what it is told
    std::vector<double> pos(4 * stage_cap);
    std::vector<int32_t> p0(2 * path_cap), p1(2 * path_cap);
    int rc = npp_goal_stages_host(map.data(), (int64_t)map.size(), interval, &ns, dist, orig, stage_cap, pos.data(), path_cap, p0.data(), p1.data(), plen);
    if (rc != 0) return rc;
    const int rows = ns > 0 ? ns : 1;
    std::vector<double> all(4 * (size_t)rows);
    rc = npp_goal_stages_host(map.data(), (int64_t)map.size(), interval, &ns, nullptr, nullptr, rows, all.data(), 0, nullptr, nullptr, nullptr);
    if (rc != 0) return rc;
    if (print) {
        std::printf("stages %d %a %a %a %d %d\n", (int)ns, dist[0], dist[1], dist[2], (int)plen[0], (int)plen[1]);
        for (int s = 0; s < rows; s++) std::printf("%a %a %a %a\n", all[4 * s], all[4 * s + 1], all[4 * s + 2], all[4 * s + 3]);
    }
    for (int s = 0; s < rows; s++) {
        const int max_rows = 8192;
        std::vector<int16_t> seg(8 * (size_t)max_rows);
        std::vector<double> ent(6 * (size_t)max_rows);
        std::vector<int32_t> order(4 * (size_t)max_rows);
        int n_seg = -1, n_ent = -1;
        uint32_t mask = 0;
        rc = npp_compile_level_segments_goal(map.data(), (int64_t)map.size(), all.data() + 4 * s, seg.data(), max_rows, &n_seg, &mask);
        if (rc != 0) return rc;
        rc = npp_compile_level_entities_goal(map.data(), (int64_t)map.size(), all.data() + 4 * s, ent.data(), max_rows, &n_ent, order.data());
        if (rc != 0) return rc;
        if (print) std::printf("variant %d %d %d\n", s, n_seg, n_ent);
    }
    return 0;
}

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    const std::vector<double> map = slurp<double>(argv[1]);
    const double interval = std::atof(argv[2]);
    const int rc = variants(map, interval, true);
    std::printf("table %d\n", rc);
    {   // the rule: 2 base levels with 3 and 0 stages, 5 envs, window 3
        const int nb = 2, nl = 5, n = 5, window = 3;
        std::vector<int32_t> lv(NPP_GOAL_LEVEL_WORDS * nb, 0), env(NPP_GOAL_ENV_WORDS * n, 0), level = {2, 2, 3, 1, 2};
        std::vector<uint32_t> ring(nb * 1, 0);
        const std::vector<int32_t> base_of = {0, 1, 0, 0, 0}, stage_of = {-1, -1, 0, 1, 2};
        lv[1 * nb + 0] = lv[1 * nb + 1] = -1;   // pending
        lv[2 * nb + 0] = 3;                     // num_stages
        lv[3 * nb + 0] = 2; lv[3 * nb + 1] = 1; // first variant
        std::vector<uint8_t> changed(n);
        int bad = 0;
        for (int step = 0; step < 12; step++) {
            std::vector<uint8_t> flags(n);
            for (int e = 0; e < n; e++) flags[e] = (uint8_t)(((step + e) % 3 == 0) ? 1 : ((step + e) % 5 == 0 ? 2 : ((step * e) & 4)));
            bad += npp_goal_apply_host(lv.data(), ring.data(), env.data(), base_of.data(), stage_of.data(), nb, nl, n, window, 2, 1, flags.data(), 11,
                                       step != 7, level.data(), nullptr, changed.data()) != 0;
        }
        std::printf("rule %d stage %d advances %d\n", bad, (int)lv[0], (int)lv[7 * nb]);
    }
    // malformed maps: every prefix length in steps of 37 values, and a map whose entity counts lie
    int refused = 0;
    for (size_t n = 0; n < map.size(); n += 37) {
        std::vector<double> cut(map.begin(), map.begin() + n);   // (its own allocation: an overrun is the sanitizer's to see)
        refused += variants(cut, interval, false) != 0;
    }
    std::vector<double> lie(map);
    if (lie.size() > 1160) { lie[1156] = 200; lie[1158] = 1e9; }
    refused += variants(lie, interval, false) != 0;
    std::printf("malformed refused %d\n", refused);
    return 0;
}
