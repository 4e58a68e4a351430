// npp_augment.hpp -- frame augmentation of player_frame and global_view (include/npp_amd.h, npp_set_frame_augmentation): the draw of
// one frame's parameters and the per-pixel function, shared by the device kernel (npp_augment.hip) and the host-only entry point
// (npp_host.cpp).  No HIP header: the host side also builds with plain g++.
//
// The four transforms, order and gates are the reference's pipeline (gym_environment/frame_augmentation.py:56-103); the pixels are
// this project's own integer definition -- parity with albumentations' pixels is unpinned.
#pragma once
#include <cstdint>

#include "npp_pool.hpp"

namespace npp {

constexpr int AUG_TRANSLATE = 1, AUG_FLIP = 2, AUG_DROPOUT = 4, AUG_BC = 8;   // AugParams::mask bits
constexpr int AUG_WORDS = 14;                                                 // int32 words of one AugParams
constexpr int AUG_PF_H = 84, AUG_PF_W = 84, AUG_GV_H = 176, AUG_GV_W = 100;   // target 0 player_frame, target 1 global_view

// what one frame (or one env's whole player_frame stack) is augmented with
struct AugParams {
    int32_t mask;         // AUG_* of the gates that passed
    int32_t sx, sy;       // shift in 1/32 px
    int32_t holes;        // 1 or 2
    int32_t hole[2][4];   // h, w, y0, x0
    int32_t a, b;         // v <- (a v + b) >> 8
};
static_assert(sizeof(AugParams) == AUG_WORDS * 4, "AugParams is AUG_WORDS plain int32 words");

// the ranges of the draw for intensity scale s10 / 10 (7 light, 10 medium, 13 strong) on an H x W image, all in integers:
// Q = floor(32 * (4 s / 84) * size), holes int(6 s) .. int(12 s), A = round(25.6 s), B = round(6528 s)
struct AugLimits {
    int32_t qx, qy, hole_lo, hole_hi, A, B;
};
NPP_HD inline AugLimits aug_limits(int s10, int H, int W) {
    AugLimits L;
    L.qx = 128 * s10 * W / 840;
    L.qy = 128 * s10 * H / 840;
    L.hole_lo = 6 * s10 / 10;
    L.hole_hi = 12 * s10 / 10;
    L.A = (256 * s10 + 50) / 100;
    L.B = (6528 * s10 + 5) / 10;
    return L;
}

NPP_HD inline bool aug_gate(uint64_t word, double prob) { return (double)(word >> 11) * (1.0 / 9007199254740992.0) < prob; }
NPP_HD inline int32_t aug_uniform(uint64_t word, int32_t lo, int32_t hi) {
    return lo + (int32_t)(((word >> 32) * (uint64_t)(hi - lo + 1)) >> 32);
}

// the parameters env `env` draws at augmentation call `count` for `target`: word j = pool_mix(base + j), every word always defined
NPP_HD inline AugParams aug_draw(uint64_t seed, uint32_t env, uint32_t count, int target, double p, int s10) {
    const int H = target ? AUG_GV_H : AUG_PF_H, W = target ? AUG_GV_W : AUG_PF_W;
    const AugLimits L = aug_limits(s10, H, W);
    const uint64_t base = pool_mix(pool_mix(((uint64_t)env << 32) | count) ^ seed ^ ((uint64_t)target * 0xD1B54A32D192ED03ull));
    AugParams P;
    P.mask = (aug_gate(pool_mix(base + 0), 0.8 * p) ? AUG_TRANSLATE : 0) | (aug_gate(pool_mix(base + 3), 0.4 * p) ? AUG_FLIP : 0) |
             (aug_gate(pool_mix(base + 4), 0.5 * p) ? AUG_DROPOUT : 0) | (aug_gate(pool_mix(base + 14), 0.4 * p) ? AUG_BC : 0);
    P.sx = aug_uniform(pool_mix(base + 1), -L.qx, L.qx);
    P.sy = aug_uniform(pool_mix(base + 2), -L.qy, L.qy);
    P.holes = aug_uniform(pool_mix(base + 5), 1, 2);
    for (int i = 0; i < 2; i++) {
        const uint64_t j = base + 6 + 4 * (uint64_t)i;
        const int32_t h = aug_uniform(pool_mix(j), L.hole_lo, L.hole_hi), w = aug_uniform(pool_mix(j + 1), L.hole_lo, L.hole_hi);
        P.hole[i][0] = h;
        P.hole[i][1] = w;
        P.hole[i][2] = aug_uniform(pool_mix(j + 2), 0, H - h);
        P.hole[i][3] = aug_uniform(pool_mix(j + 3), 0, W - w);
    }
    P.a = aug_uniform(pool_mix(base + 15), 256 - L.A, 256 + L.A);
    P.b = aug_uniform(pool_mix(base + 16), -L.B, L.B);
    return P;
}

// parameters that came from a caller instead of the draw: inside the image and small enough for the 32-bit pixel arithmetic
NPP_HD inline bool aug_params_ok(const AugParams &P, int H, int W) {
    if (P.mask < 0 || P.mask > 15 || P.holes < 0 || P.holes > 2) return false;
    if (P.sx < -32 * W || P.sx > 32 * W || P.sy < -32 * H || P.sy > 32 * H) return false;
    for (int i = 0; i < 2; i++) {
        const int32_t *r = P.hole[i];
        if (r[0] < 0 || r[0] > H || r[1] < 0 || r[1] > W || r[2] < 0 || r[2] > H - r[0] || r[3] < 0 || r[3] > W - r[1]) return false;
    }
    return P.a >= 0 && P.a <= 512 && P.b >= -65536 && P.b <= 65536;
}

NPP_HD inline int aug_tap(const uint8_t *src, int H, int W, int y, int x) {
    return ((unsigned)y < (unsigned)H && (unsigned)x < (unsigned)W) ? (int)src[y * W + x] : 0;
}

// output pixel (y, x) of the H x W image `src` under P: translate (constant-border bilinear, source quantised to 1/32 px), flip,
// coarse dropout in output coordinates, brightness / contrast last
NPP_HD inline uint8_t aug_pixel(const uint8_t *src, int H, int W, const AugParams &P, int y, int x) {
    int v = 0;
    bool hole = false;
    if (P.mask & AUG_DROPOUT)
        for (int i = 0; i < 2; i++)
            hole = hole || (i < P.holes && y >= P.hole[i][2] && y < P.hole[i][2] + P.hole[i][0] && x >= P.hole[i][3] &&
                            x < P.hole[i][3] + P.hole[i][1]);
    if (!hole) {
        const int xs = (P.mask & AUG_FLIP) ? W - 1 - x : x;
        if (P.mask & AUG_TRANSLATE) {
            const int X = 32 * xs - P.sx, Y = 32 * y - P.sy;
            const int x0 = X >> 5, fx = X & 31, y0 = Y >> 5, fy = Y & 31;
            v = ((32 - fx) * (32 - fy) * aug_tap(src, H, W, y0, x0) + fx * (32 - fy) * aug_tap(src, H, W, y0, x0 + 1) +
                 (32 - fx) * fy * aug_tap(src, H, W, y0 + 1, x0) + fx * fy * aug_tap(src, H, W, y0 + 1, x0 + 1) + 512) >> 10;
        } else {
            v = src[y * W + xs];
        }
    }
    if (P.mask & AUG_BC) {
        v = (P.a * v + P.b) >> 8;
        v = v < 0 ? 0 : (v > 255 ? 255 : v);
    }
    return (uint8_t)v;
}

}  // namespace npp
