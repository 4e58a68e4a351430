// Stand-alone driver of the reward mode's host-only entries (npp_reward_level_constants_host, npp_reward_host) for a build with
// g++ -fsanitize=address,undefined: tests/test_reward_host.py compiles it TOGETHER with the host sources (npp_level.cpp,
// npp_reach.cpp, npp_host.cpp) into one executable with the sanitizer runtimes linked statically and runs it as a program of its
// own -- no sanitizer runtime is loaded into Python, and the program does not care what else its environment loads.
//   reward_sanitized_main MAP POS FLAGS FRAMES COUNT END_BITS   (raw little-endian files: f64 map, f64[COUNT + 1][2], u8[COUNT], u16[COUNT])
// prints the three level constants and COUNT rewards as hex floats, then calls both entries on truncated copies of the map.
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
    double c[3];
    int32_t st = -1;
    const int rc = npp_reward_level_constants_host(map.data(), (int64_t)map.size(), c, &st);
    std::printf("constants %d %d %a %a %a\n", rc, (int)st, c[0], c[1], c[2]);
    std::vector<double> rew((size_t)count + 1), comp(6 * (size_t)count + 6);
    std::vector<uint8_t> kind((size_t)count + 1);
    const int rr = npp_reward_host(map.data(), (int64_t)map.size(), nullptr, pos.data(), pos.data() + 2, flags.data(), frames.data(), count, end_bits,
                                   rew.data(), comp.data(), kind.data(), &st);
    std::printf("rewards %d\n", rr);
    if (rr == 0)
        for (int k = 0; k < count; k++) std::printf("%a %d\n", rew[k], (int)kind[k]);
    // malformed maps: every prefix length in steps of 37 values, and a map whose entity counts lie
    int refused = 0;
    for (size_t n = 0; n < map.size(); n += 37) {
        std::vector<double> cut(map.begin(), map.begin() + n);   // (its own allocation: an overrun is the sanitizer's to see)
        refused += npp_reward_level_constants_host(cut.data(), (int64_t)cut.size(), c, &st) != 0;
        refused += npp_reward_host(cut.data(), (int64_t)cut.size(), nullptr, pos.data(), pos.data() + 2, flags.data(), frames.data(),
                                   count < 8 ? count : 8, end_bits, rew.data(), comp.data(), kind.data(), &st) != 0;
    }
    std::vector<double> lie(map);
    if (lie.size() > 1160) { lie[1156] = 200; lie[1158] = 1e9; }
    refused += npp_reward_level_constants_host(lie.data(), (int64_t)lie.size(), c, &st) != 0;
    std::printf("malformed refused %d\n", refused);
    return 0;
}
