// Stand-alone driver of npp_archive_seed_rows_host for a build with g++ -fsanitize=address,undefined: tests/test_seed_host.py
// compiles it TOGETHER with the host sources into one executable with the sanitizer runtimes linked statically and runs it as a
// program of its own -- no sanitizer runtime is loaded into Python.
//   seed_sanitized_main SETS   (raw bytes: per set a little-endian u32 length, one mode byte, then the input bytes)
// prints per set: rc, then actions / route_bits / score bit patterns, one line each.  Every array, the inputs included, is an
// allocation of exactly `length` elements, so an overrun is the sanitizer's to see.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "npp_amd.h"

int main(int argc, char **argv) {
    if (argc != 2) return 2;
    std::vector<uint8_t> v;
    FILE *f = std::fopen(argv[1], "rb");
    if (!f) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    int ch;
    while ((ch = std::fgetc(f)) != EOF) v.push_back((uint8_t)ch);
    std::fclose(f);
    size_t at = 0;
    while (at + 5 <= v.size()) {
        uint32_t n;
        std::memcpy(&n, v.data() + at, 4);
        const int mode = (int)(int8_t)v[at + 4];
        at += 5;
        if (at + n > v.size()) return 2;
        std::vector<uint8_t> in(v.begin() + at, v.begin() + at + n), actions(n, 99), bits(n, 99);
        std::vector<float> scores(n, -7.0f);
        at += n;
        const int rc = npp_archive_seed_rows_host(in.data(), (int64_t)n, mode, actions.data(), bits.data(), scores.data());
        std::printf("%d\n", rc);
        for (uint32_t k = 0; k < n; k++) std::printf("%d ", (int)actions[k]);
        std::printf("\n");
        for (uint32_t k = 0; k < n; k++) std::printf("%d ", (int)bits[k]);
        std::printf("\n");
        for (uint32_t k = 0; k < n; k++) {
            uint32_t b;
            std::memcpy(&b, &scores[k], 4);
            std::printf("%u ", (unsigned)b);
        }
        std::printf("\n");
    }
    return 0;
}
