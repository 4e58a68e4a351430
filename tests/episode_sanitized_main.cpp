// Stand-alone driver of the episode statistics' host-only entry (npp_episode_apply_host) for a build with
// g++ -fsanitize=address,undefined: tests/test_episode_host.py compiles it TOGETHER with the host sources (npp_level.cpp,
// npp_reach.cpp, npp_host.cpp) into one executable with the sanitizer runtimes linked statically and runs it as a program of its
// own -- no sanitizer runtime is loaded into Python, and the program does not care what else its environment loads.
//   episode_sanitized_main EVENTS ROWS COUNT N_LEVELS AUTORESET   (raw little-endian files: i32[COUNT][8], f32[COUNT][8])
// applies the list in one call and event by event (both must agree), prints the record and the table, then drives the entry with
// zero-length lists, no table, the largest level ids and arguments it must refuse.  Every buffer is an allocation of its exact size.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
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

static void init(std::vector<int32_t> &ri, std::vector<double> &rd) {
    const int32_t ev[8] = {4, 0, 0, 0, 0, 0, 0, 0};
    ri.assign(NPP_EP_NI, 7);
    rd.assign(NPP_EP_ND, 7.0);
    if (npp_episode_apply_host(ri.data(), rd.data(), nullptr, 0, 0, ev, nullptr, 1, nullptr) != 0) std::exit(3);
}

int main(int argc, char **argv) {
    if (argc != 6) return 2;
    const std::vector<int32_t> events = slurp<int32_t>(argv[1]);
    const std::vector<float> rows = slurp<float>(argv[2]);
    const int count = std::atoi(argv[3]), n_levels = std::atoi(argv[4]), autoreset = std::atoi(argv[5]);
    if ((int)events.size() != 8 * count || (int)rows.size() != 8 * count || n_levels < 1) return 2;
    std::vector<int32_t> ri, ri2;
    std::vector<double> rd, rd2;
    init(ri, rd);
    init(ri2, rd2);
    std::vector<uint64_t> table((size_t)n_levels * NPP_EP_COLS, 0), table2(table);
    uint8_t ended = 9;
    int rc = npp_episode_apply_host(ri.data(), rd.data(), table.data(), n_levels, autoreset, events.data(), rows.data(), count, &ended);
    int any = 0;
    for (int i = 0; i < count && rc == 0; i++) {   // event by event, each from buffers of one event
        std::vector<int32_t> ev(events.begin() + 8 * i, events.begin() + 8 * i + 8);
        std::vector<float> row(rows.begin() + 8 * i, rows.begin() + 8 * i + 8);
        uint8_t e = 9;
        rc = npp_episode_apply_host(ri2.data(), rd2.data(), table2.data(), n_levels, autoreset, ev.data(), row.data(), 1, &e);
        any |= e;
    }
    const bool same = ri == ri2 && table == table2 && std::memcmp(rd.data(), rd2.data(), sizeof(double) * NPP_EP_ND) == 0 && any == ended;
    std::printf("applied %d %d %d\n", rc, (int)ended, same ? 1 : 0);
    for (int k = 0; k < NPP_EP_NI; k++) std::printf("%d ", (int)ri[k]);
    std::printf("\n");
    for (int k = 0; k < NPP_EP_ND; k++) std::printf("%a ", rd[k]);
    std::printf("\n");
    for (size_t k = 0; k < table.size(); k++) std::printf("%llu ", (unsigned long long)table[k]);
    std::printf("\n");

    int ok = 0, refused = 0;
    // zero-length lists: nothing changes, with and without a table
    std::vector<int32_t> zi(ri);
    std::vector<double> zd(rd);
    ok += npp_episode_apply_host(zi.data(), zd.data(), nullptr, 0, 1, nullptr, nullptr, 0, nullptr) == 0 && zi == ri;
    ok += npp_episode_apply_host(zi.data(), zd.data(), table.data(), n_levels, 0, nullptr, nullptr, 0, &ended) == 0 && ended == 0;
    // the largest level id the table has, the first one past it, the largest int and a negative one: only the first may be added
    const int32_t levels[4] = {n_levels - 1, n_levels, INT32_MAX, INT32_MIN};
    for (int k = 0; k < 4; k++) {
        init(zi, zd);
        std::vector<uint64_t> t((size_t)n_levels * NPP_EP_COLS, 0);
        const int32_t ev[24] = {0, 0, 4, levels[k], 1, 0, 0, 0, 1, levels[k], 0, 0, 0, 0, 0, 0, 0, 1 | 4, 65535, levels[k], 0, 0, 0, 0};
        const std::vector<float> r(24, 0.5f);
        ok += npp_episode_apply_host(zi.data(), zd.data(), t.data(), n_levels, 1, ev, r.data(), 3, &ended) == 0 && ended == 1;
        uint64_t sum = 0;
        for (uint64_t v : t) sum += v;
        ok += k == 0 ? (t[(size_t)(n_levels - 1) * NPP_EP_COLS + NPP_EPC_ABANDONED] == 1 && t[(size_t)(n_levels - 1) * NPP_EP_COLS] == 1) : sum == 0;
        // the same without any table
        init(zi, zd);
        ok += npp_episode_apply_host(zi.data(), zd.data(), nullptr, 0, 0, ev, r.data(), 3, nullptr) == 0;
    }
    // refusals
    const int32_t bad_kind[8] = {6, 0, 0, 0, 0, 0, 0, 0}, bad_flags[8] = {0, 256, 1, 0, 0, 0, 0, 0}, bad_frames[8] = {0, 0, 65536, 0, 0, 0, 0, 0},
                  neg[8] = {-1, 0, 0, 0, 0, 0, 0, 0}, good[8] = {0, 0, 1, 0, 0, 0, 0, 0};
    const float r8[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    init(zi, zd);
    refused += npp_episode_apply_host(nullptr, zd.data(), nullptr, 0, 0, nullptr, nullptr, 0, nullptr) != 0;
    refused += npp_episode_apply_host(zi.data(), nullptr, nullptr, 0, 0, nullptr, nullptr, 0, nullptr) != 0;
    refused += npp_episode_apply_host(zi.data(), zd.data(), nullptr, 1, 0, nullptr, nullptr, 0, nullptr) != 0;
    refused += npp_episode_apply_host(zi.data(), zd.data(), nullptr, -1, 0, nullptr, nullptr, 0, nullptr) != 0;
    refused += npp_episode_apply_host(zi.data(), zd.data(), nullptr, 0, 0, nullptr, nullptr, 1, nullptr) != 0;
    refused += npp_episode_apply_host(zi.data(), zd.data(), nullptr, 0, 0, good, r8, -1, nullptr) != 0;
    refused += npp_episode_apply_host(zi.data(), zd.data(), nullptr, 0, 0, good, nullptr, 1, nullptr) != 0;
    refused += npp_episode_apply_host(zi.data(), zd.data(), nullptr, 0, 0, bad_kind, r8, 1, nullptr) != 0;
    refused += npp_episode_apply_host(zi.data(), zd.data(), nullptr, 0, 0, bad_flags, r8, 1, nullptr) != 0;
    refused += npp_episode_apply_host(zi.data(), zd.data(), nullptr, 0, 0, bad_frames, r8, 1, nullptr) != 0;
    refused += npp_episode_apply_host(zi.data(), zd.data(), nullptr, 0, 0, neg, r8, 1, nullptr) != 0;
    std::printf("edge ok %d refused %d\n", ok, refused);
    return 0;
}
