// npp_cells.hpp -- the cell index over the checkpoint archive (include/npp_amd.h, npp_archive_cells_create): the definitions the
// device kernels (npp_cells.hip) and the host-only entry points (npp_host.cpp) share.  No HIP header: the host side also builds
// with plain g++.  Everything that decides anything here is integer or IEEE f64 (the build has -ffp-contract=off), so the device,
// the host entries and the Python restatement of the tests agree bit for bit.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstring>

#include "npp_pool.hpp"   // pool_mix
#include "npp_state.hpp"

namespace npp {

constexpr int CELL_GRID_W = 44, CELL_GRID_H = 25;                        // 24 px cells: the tile grid of LevelHdr::off_tiles
constexpr int NPP_CELLS_PER_LEVEL = 2 * CELL_GRID_W * CELL_GRID_H;      // (switch_activated, cy, cx) = 2200 keys per level
enum CellStatus { CELL_NOT_ELIGIBLE = 5, CELL_LOST = 6, CELL_FULL = 7 };   // extend ArchiveStatus (0 stored, 1 skipped)

// The key of a state inside its level, or -1 when the state is not eligible.  ninja_state: dump column 0 (0..5 are the live
// states); sw_state: exit_switch_state (npp_state.hpp), dump column 13; has_door: the level has an
// exit door (LevelHdr::obs_door >= 0) at (door_x, door_y).  The last test is the seeder's exit filter
// (replay/demo_checkpoint_seeder.py:30, :118-153): no checkpoint nearer than 72 px to the door once the switch is on.
NPP_HD inline int cell_key_in_level(int ninja_state, int sw_state, double x, double y, bool has_door, double door_x, double door_y) {
    if (ninja_state < 0 || ninja_state > 5) return -1;
    const double qx = x / 24.0, qy = y / 24.0;
    if (!(qx >= 0.0 && qx < (double)CELL_GRID_W && qy >= 0.0 && qy < (double)CELL_GRID_H)) return -1;   // (NaN fails too)
    const int cx = (int)floor(qx), cy = (int)floor(qy);
    const int sw = exit_switch_activated(sw_state);
    if (sw && has_door) {
        const double dx = x - door_x, dy = y - door_y;
        if (sqrt(dx * dx + dy * dy) < 72.0) return -1;
    }
    return (sw * CELL_GRID_H + cy) * CELL_GRID_W + cx;
}

// float bits in an order unsigned integers compare by: -0.0 below +0.0, the infinities ordinary values, > 0 for every non-NaN
NPP_HD inline uint32_t cell_ordered_bits(uint32_t b) { return b ^ ((b >> 31) ? 0xffffffffu : 0x80000000u); }
NPP_HD inline uint32_t cell_float_bits(uint32_t ob) { return ob ^ ((ob >> 31) ? 0x80000000u : 0xffffffffu); }   // its inverse
NPP_HD inline bool cell_bits_nan(uint32_t b) { return (b & 0x7fffffffu) > 0x7f800000u; }

// Low word of a `best` entry: 0xffffffff marks the incumbent, an env's proposal is 0xfffffffe - env -- below the incumbent's for every
// env (~env would be the incumbent's own word for env 0), so an incumbent wins ties, and descending in env, so the lowest env wins
// a tie inside a call
NPP_HD inline uint32_t cell_proposal_word(uint32_t env) { return 0xfffffffeu - env; }

// Go-Explore's count rule, quantised so that sums are exact: the weight of a key that holds a slot
NPP_HD inline uint32_t cell_weight(uint32_t visits, uint32_t chosen) {
    return (uint32_t)floor(1048576.0 / sqrt((double)((uint64_t)visits + (uint64_t)chosen + 1u)));
}

NPP_HD inline uint64_t cell_mulhi(uint64_t a, uint64_t b) { return (uint64_t)(((unsigned __int128)a * b) >> 64); }   // __umul64hi

// The key inside its level that env `env` draws in select call number `call`: cdf[k] = w(0) + ... + w(k) over the level's
// NPP_CELLS_PER_LEVEL keys (T = the last entry, > 0); the first key whose inclusive prefix sum is > t
NPP_HD inline int cell_pick(const uint64_t *cdf, uint64_t seed, uint32_t env, uint32_t call) {
    const uint64_t u = pool_mix(pool_mix(((uint64_t)env << 32) | call) ^ seed);
    const uint64_t t = cell_mulhi(u, cdf[NPP_CELLS_PER_LEVEL - 1]);
    int lo = 0, hi = NPP_CELLS_PER_LEVEL - 1;   // (t < T: the last key always qualifies)
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (cdf[mid] <= t) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

}  // namespace npp
