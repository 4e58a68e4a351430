// Stand-alone driver of the path waypoints' host-only entries (npp_reward_waypoints_host, npp_reward_host_wp) for a build with
// g++ -fsanitize=address,undefined: tests/test_waypoints_host.py compiles it TOGETHER with the host sources (npp_level.cpp,
// npp_reach.cpp, npp_host.cpp) into one executable with the sanitizer runtimes linked statically and runs it as a program of its
// own -- no sanitizer runtime is loaded into Python, and the program does not care what else its environment loads.
//   waypoints_sanitized_main MAP POS FLAGS FRAMES COUNT END_BITS   (raw little-endian files: f64 map, f64[COUNT + 1][2], u8[COUNT], u16[COUNT])
// prints the table's sizes and COUNT rows (reward, bonus as hex floats, collected index), then calls both entries on truncated
// copies of the map and on one whose entity counts lie.  Every output buffer is exactly as large as the entry is told.
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

int main(int argc, char **argv) {
    if (argc != 7) return 2;
    const std::vector<double> map = slurp<double>(argv[1]), pos = slurp<double>(argv[2]);
    const std::vector<uint8_t> flags = slurp<uint8_t>(argv[3]);
    const std::vector<uint16_t> frames = slurp<uint16_t>(argv[4]);
    const int count = std::atoi(argv[5]), end_bits = std::atoi(argv[6]);
    if ((int)flags.size() != count || (int)frames.size() != count || (int)pos.size() != 2 * (count + 1)) return 2;
    NppWaypointParams wp;
    npp_waypoint_default_params(&wp);
    const int cap = 7, path_cap = 5;   // smaller than the tables: the entries must stop at what they are told
    std::vector<double> xy(2 * cap);
    std::vector<uint8_t> phase(cap);
    std::vector<int32_t> node_index(cap), p0(2 * path_cap), p1(2 * path_cap), plen(2), nodes(6);
    int32_t st = -1, n_wp = -1;
    const int rc = npp_reward_waypoints_host(map.data(), (int64_t)map.size(), wp.progress_spacing, cap, xy.data(), phase.data(), node_index.data(), &n_wp,
                                             path_cap, p0.data(), p1.data(), plen.data(), nodes.data(), &st);
    int n_pre = 0;
    if (rc == 0) {   // the phases of the whole table, through buffers of its size
        std::vector<double> xy2(2 * (size_t)n_wp + 2);
        std::vector<uint8_t> ph2((size_t)n_wp + 1);
        int32_t n2 = -1;
        if (npp_reward_waypoints_host(map.data(), (int64_t)map.size(), wp.progress_spacing, n_wp, xy2.data(), ph2.data(), nullptr, &n2, 0, nullptr, nullptr,
                                      nullptr, nullptr, nullptr) != 0 || n2 != n_wp)
            return 3;
        for (int i = 0; i < n_wp; i++) n_pre += ph2[i] == 0;
    }
    std::printf("table %d %d %d %d %d %d\n", rc, (int)st, (int)n_wp, n_pre, (int)plen[0], (int)plen[1]);
    std::vector<double> rew((size_t)count), comp(6 * (size_t)count), bonus((size_t)count);
    std::vector<uint8_t> kind((size_t)count);
    std::vector<int32_t> info(3 * (size_t)count);
    const int rr = npp_reward_host_wp(map.data(), (int64_t)map.size(), nullptr, &wp, pos.data(), pos.data() + 2, flags.data(), frames.data(), count, end_bits,
                                      rew.data(), comp.data(), kind.data(), &st, bonus.data(), info.data());
    std::printf("rewards %d\n", rr);
    if (rr == 0)
        for (int k = 0; k < count; k++) std::printf("%a %a %d\n", rew[k], bonus[k], (int)info[3 * k]);
    // malformed maps: every prefix length in steps of 37 values, and a map whose entity counts lie
    int refused = 0;
    const int few = count < 8 ? count : 8;
    for (size_t n = 0; n < map.size(); n += 37) {
        std::vector<double> cut(map.begin(), map.begin() + n);   // (its own allocation: an overrun is the sanitizer's to see)
        refused += npp_reward_waypoints_host(cut.data(), (int64_t)cut.size(), wp.progress_spacing, cap, xy.data(), phase.data(), node_index.data(), &n_wp,
                                             path_cap, p0.data(), p1.data(), plen.data(), nodes.data(), &st) != 0;
        refused += npp_reward_host_wp(cut.data(), (int64_t)cut.size(), nullptr, &wp, pos.data(), pos.data() + 2, flags.data(), frames.data(), few, end_bits,
                                      rew.data(), comp.data(), kind.data(), &st, bonus.data(), info.data()) != 0;
    }
    std::vector<double> lie(map);
    if (lie.size() > 1160) { lie[1156] = 200; lie[1158] = 1e9; }
    refused += npp_reward_waypoints_host(lie.data(), (int64_t)lie.size(), wp.progress_spacing, cap, xy.data(), phase.data(), node_index.data(), &n_wp, path_cap,
                                         p0.data(), p1.data(), plen.data(), nodes.data(), &st) != 0;
    refused += npp_reward_host_wp(lie.data(), (int64_t)lie.size(), nullptr, &wp, pos.data(), pos.data() + 2, flags.data(), frames.data(), few, end_bits,
                                  rew.data(), comp.data(), kind.data(), &st, bonus.data(), info.data()) != 0;
    std::printf("malformed refused %d\n", refused);
    return 0;
}
