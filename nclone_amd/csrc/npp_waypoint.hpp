// npp_waypoint.hpp -- the sequential path waypoints of reward mode "pbrs": what RewardCalculator.calculate_reward adds on a live step
// under a fresh RewardConfig() (enable_path_waypoints=True, reward_config.py:48): `_calculate_sequential_waypoint_bonus`
// (main_reward_calculator.py:2313-2484) with `RewardConfig.get_waypoint_bonus` (reward_config.py:309-399).  One function, compiled
// for the host (npp_reward_host_wp, the CPU parity test against tests/golden/waypoints.npz) and for the device
// (npp_waypoint.hip), as npp_reward.hpp is.  All arithmetic is fp64 (build with -ffp-contract=off).
//
// What the reference REALLY does (DESIGN.md 23 lists every quirk with file:line):
//   * `prev_player_pos` is overwritten with the current position (:534) before the bonus runs (:662), so `prev_dist == curr_dist` and
//     the collection rule is a function of the current position alone;
//   * at most one waypoint is collected per step: the FIRST in sequence order (pre-switch by node_index, then post-switch) that is
//     not collected, is not a post-switch waypoint while the switch is off, and lies within the radius;
//   * an out-of-sequence collection sets next-expected to index + 1, which may move it backwards;
//   * the farming penalty of the death branch reads a key that is never in the observation (:335): it is always 0.
#pragma once
#include "npp_reach_features.hpp"

namespace npp {

// npp_amd.h NppWaypointParams (the same four doubles)
struct WaypointParams {
    double collection_radius, out_of_order_scale, progress_scale, progress_spacing;
};

constexpr int WP_MAX = 512;                          // waypoints per level: the collected set is 512 bits per env
constexpr int WP_WORDS = WP_MAX / 32;
constexpr int WP_NI = WP_WORDS + 2;                  // per-env state words: the set, next expected, collected count
constexpr int WP_CW = 46, WP_CH = 27;                // 24-px cells of WORLD space (node + 24: up to 1104 x 648)
constexpr int WP_CELLS = WP_CW * WP_CH;
constexpr double WP_MAX_RADIUS = 24.0;               // the 3 x 3 cell walk covers no more
constexpr double WP_BUDGET = 30.0;                   // BASE_WAYPOINT_BUDGET, reward_config.py:362
constexpr double WP_REFERENCE_COUNT = 20.0;          // REFERENCE_WAYPOINT_COUNT, reward_config.py:363
constexpr double WP_MIN_SPAWN_DISTANCE = 20.0;       // MIN_SPAWN_DISTANCE, path_waypoint_extractor.py:270

// Per-level table as laid out in HBM: one header per level + a blob (offsets in bytes from the blob start, 4-byte aligned).
//   records  u32[count]          in sequence order: x | y << 12 | phase << 24 (world pixels, integer-valued; phase 1 = post_switch)
//   start    u16[WP_CELLS + 1]   CSR index by 24-px cell (cell = cx * WP_CH + cy)
//   list     u16[count]          sequence indices, ascending within a cell
struct WaypointHdr {
    uint32_t count, n_pre;
    uint32_t off_rec, off_start, off_list;
    uint32_t pad_[3];
};

struct WaypointTabs {
    const WaypointHdr *H;
    const unsigned char *blob;
};

struct WaypointOut {
    double bonus;   // unscaled (the reward kernel applies GLOBAL_REWARD_SCALE with the rest of the sum)
    int index;      // collected sequence index, -1 = none
};

// `v ** 2`: CPython's float power is libm pow().  The host twin calls it (through a pointer the compiler cannot fold); the device has
// no bit-compatible pow and multiplies, as the step kernel does.  A bit of the SUM can differ for ~0.1 % of
// the inputs; the comparison with the radius can only differ when the sum lies within an ulp of radius squared.
NPP_HD inline double waypoint_sq(double v) {
#if defined(__HIP_DEVICE_COMPILE__)
    return v * v;
#else
    static double (*volatile py_pow)(double, double) = static_cast<double (*)(double, double)>(pow);
    return py_pow(v, 2.0);
#endif
}

// RewardConfig.get_waypoint_bonus (reward_config.py:309-399) at curriculum stage 0
NPP_HD inline double waypoint_bonus(int idx, int total, bool in_sequence, double progress_scale, double out_of_order_scale) {
    const double t = (double)(total > 1 ? total : 1);
    const double ratio = WP_REFERENCE_COUNT / t;
    const double budget_scale = ratio < 1.0 ? ratio : 1.0;   // min(1.0, ratio)
    const double budget = WP_BUDGET * budget_scale;
    const double base = budget / t;
    const double fraction = (double)idx / (double)(total - 1 > 1 ? total - 1 : 1);
    const double multiplier = 1.0 + fraction * progress_scale;
    const double bonus = base * multiplier;
    return in_sequence ? bonus : bonus * out_of_order_scale;
}

// RewardCalculator.reset() (:1120-1123): the collected set, the sequence and the next-expected index; the level's lists stay
NPP_HD inline void waypoint_restart(uint32_t *bits, size_t stride, uint32_t &next, uint32_t &count) {
    for (int w = 0; w < WP_WORDS; w++) bits[(size_t)w * stride] = 0u;
    next = 0u;
    count = 0u;
}

// _calculate_sequential_waypoint_bonus on a live step at (px, py).  bits: the env's collected set, word w at bits[w * stride].
NPP_HD inline WaypointOut waypoint_step(const WaypointTabs &T, const WaypointParams &P, uint32_t *bits, size_t stride, uint32_t &next, uint32_t &count,
                                        double px, double py, int sw) {
    WaypointOut o;
    o.bonus = 0.0;
    o.index = -1;
    const WaypointHdr &H = *T.H;
    const int total = (int)H.count;
    if (total <= 0) return o;
    const uint32_t *rec = reinterpret_cast<const uint32_t *>(T.blob + H.off_rec);
    const uint16_t *start = reinterpret_cast<const uint16_t *>(T.blob + H.off_start);
    const uint16_t *list = reinterpret_cast<const uint16_t *>(T.blob + H.off_list);
    int cx = reach_cell24(px), cy = reach_cell24(py);
    cx = cx < 0 ? 0 : (cx > WP_CW - 1 ? WP_CW - 1 : cx);
    cy = cy < 0 ? 0 : (cy > WP_CH - 1 ? WP_CH - 1 : cy);
    const int x0 = cx > 0 ? cx - 1 : 0, x1 = cx < WP_CW - 1 ? cx + 1 : WP_CW - 1;
    const int y0 = cy > 0 ? cy - 1 : 0, y1 = cy < WP_CH - 1 ? cy + 1 : WP_CH - 1;
    int best = total;   // the minimum sequence index = the first hit of the reference's loop
    for (int ix = x0; ix <= x1; ix++)
        for (int iy = y0; iy <= y1; iy++) {
            const int cell = ix * WP_CH + iy;
            const int k1 = (int)start[cell + 1];
            for (int k = (int)start[cell]; k < k1; k++) {
                const int idx = (int)list[k];
                if (idx >= best) break;   // ascending within the cell
                const uint32_t r = rec[idx];
                if (((r >> 24) & 1u) && !sw) continue;   // post-switch waypoints are blocked until the switch is on (:2398)
                const double wx = (double)(r & 0xfffu), wy = (double)((r >> 12) & 0xfffu);
                const double dist = sqrt(waypoint_sq(px - wx) + waypoint_sq(py - wy));   // math.sqrt(dx ** 2 + dy ** 2) (:2405)
                if (!(dist <= P.collection_radius)) continue;
                if ((bits[(size_t)(idx >> 5) * stride] >> (idx & 31)) & 1u) continue;   // already collected (:2394)
                best = idx;
                break;
            }
        }
    if (best >= total) return o;
    bits[(size_t)(best >> 5) * stride] |= 1u << (best & 31);
    count++;
    const bool in_sequence = (uint32_t)best == next;
    o.bonus = waypoint_bonus(best, total, in_sequence, P.progress_scale, P.out_of_order_scale);
    o.index = best;
    next = in_sequence ? next + 1u : (uint32_t)best + 1u;   // (:2432, :2469)
    return o;
}

}  // namespace npp
