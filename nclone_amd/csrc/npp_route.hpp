// npp_route.hpp -- action routes (include/npp_amd.h, npp_set_routes): the list of actions that led each env from its spawn to where
// it is, the reference's `_action_sequence` (base_environment.py:186 creates it, :517 appends per step, :1677 clears at reset,
// :2114 appends during a checkpoint replay).  The rule lives here, shared by the device kernels (npp_route.hip, npp_archive.hip) and
// the host-only entry point (npp_host.cpp: npp_route_apply_host).  No HIP header: the host side also builds with plain g++.
// Everything is integer, so the device, the host entry and the Python restatement of the tests (tests/route_ref.py) agree bit
// for bit.
//
// Per env: a header of ROUTE_HDR_WORDS i32 and two buffers of `cap` bytes (one action, 0..5, per byte).
//   words 0-5   the CURRENT route (the episode being played)
//   words 6-11  the FINISHED route (the episode that ended last)
//   word 12     which of the two buffers holds the current route (0 / 1); the finished route's bytes are in the other
//   words 13-15 0
// One route header:
//   R_LEN     actions stored
//   R_BITS    ROUTE_OVERFLOW: an action was dropped because len == cap; ROUTE_BROKEN: the record cannot be replayed from the spawn
//             (raw ticks, or steps of different frame_skip)
//   R_FS      frame_skip of the steps, 0 while empty
//   R_FRAMES  sum of the frames executed
//   R_FLAGS   flags byte of the last executed step, 0 while empty
//   R_LEVEL   the level at the first append, -1 while empty
#pragma once
#include <cstdint>

#include "npp_state.hpp"   // NPP_HD

namespace npp {

constexpr int ROUTE_HDR_WORDS = 16, ROUTE_WORDS = 6, ROUTE_FINISHED = 6, ROUTE_CUR = 12;
enum RouteWord { R_LEN = 0, R_BITS, R_FS, R_FRAMES, R_FLAGS, R_LEVEL };
constexpr int ROUTE_OVERFLOW = 1, ROUTE_BROKEN = 2;
constexpr int ROUTE_END_FLAGS = 1 | 2 | 8;   // NPP_F_WON | NPP_F_DEAD | NPP_F_TRUNCATED: the step ended the episode
// a route inside an archive record: the six words, two zero words, then the bytes
constexpr int ROUTE_REC_HDR_WORDS = 8;

NPP_HD inline int route_round_cap(int capacity) { return (capacity + 15) / 16 * 16; }
NPP_HD inline bool route_empty(const int32_t *r) { return r[R_LEN] == 0 && r[R_BITS] == 0; }
NPP_HD inline void route_clear(int32_t *r) {
    r[R_LEN] = 0; r[R_BITS] = 0; r[R_FS] = 0; r[R_FRAMES] = 0; r[R_FLAGS] = 0; r[R_LEVEL] = -1;
}
// a new env / a new level set: both routes empty
NPP_HD inline void route_init(int32_t *h) {
    for (int k = 0; k < ROUTE_HDR_WORDS; k++) h[k] = 0;
    h[R_LEVEL] = -1;
    h[ROUTE_FINISHED + R_LEVEL] = -1;
}

// The episode is over (an auto-reset, or any reset from outside): the current route becomes the finished one and a new, empty one
// starts in the other buffer.  No bytes move.  An empty current route changes nothing: the finished route of the last real episode
// stays readable through any number of further resets.
NPP_HD inline void route_flip(int32_t *h) {
    if (route_empty(h)) return;
    for (int k = 0; k < ROUTE_WORDS; k++) h[ROUTE_FINISHED + k] = h[k];
    h[ROUTE_CUR] ^= 1;
    route_clear(h);
}

// One executed step row of the env: action a, the step's flags byte f and frame count x, the launch's frame_skip fs, the env's
// level, whether the handle auto-resets.  bufs: the env's two buffers, [2][cap].  An env that is already terminal and is not
// auto-reset executes 0 frames (npp_kernels.hip: `live`) and appends nothing.
NPP_HD inline void route_step(int32_t *h, uint8_t *bufs, int cap, int a, int f, int x, int fs, int level, bool autoreset) {
    if (x > 0) {
        if (route_empty(h)) { h[R_FS] = fs; h[R_LEVEL] = level; }
        else if (h[R_FS] != fs) h[R_BITS] |= ROUTE_BROKEN;
        if (h[R_LEN] < cap) { bufs[(size_t)(h[ROUTE_CUR] & 1) * cap + h[R_LEN]] = (uint8_t)a; h[R_LEN]++; }
        else h[R_BITS] |= ROUTE_OVERFLOW;
        h[R_FRAMES] += x;
        h[R_FLAGS] = f;
    }
    if (autoreset && (f & ROUTE_END_FLAGS)) route_flip(h);
}

// npp_tick moves the env by raw input bytes: whatever the current route holds no longer leads to the env's state
NPP_HD inline void route_tick(int32_t *h) { h[R_BITS] |= ROUTE_BROKEN; }

// A restore (npp_archive_restore / npp_restore) replaces the CURRENT route with a record's: src = its six words, bytes = its
// actions.  The finished route and word 12 stay.  (The device kernel moves the bytes itself, over consecutive lanes.)
NPP_HD inline void route_restore(int32_t *h, uint8_t *bufs, int cap, const int32_t *src, const uint8_t *bytes) {
    for (int k = 0; k < ROUTE_WORDS; k++) h[k] = src[k];
    uint8_t *dst = bufs + (size_t)(h[ROUTE_CUR] & 1) * cap;
    for (int k = 0; k < src[R_LEN] && k < cap; k++) dst[k] = bytes[k];
}

}  // namespace npp
