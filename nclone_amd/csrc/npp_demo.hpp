// npp_demo.hpp -- demonstration transitions from recorded replays (include/npp_amd.h, npp_demo_create): the plan
// that npp_demo_plan_host and npp_demo_create share.  Host only, no HIP header: it builds with plain g++ for the sanitized host
// library.  The kernels are npp_demo.hip's.
#pragma once
#include <algorithm>
#include <cstdint>
#include <numeric>
#include <vector>

#include "npp_state.hpp"   // NPP_HD

namespace npp {

// map_input_to_action (replay/replay_executor.py:42-58): bytes 6, 7 and above -> NOOP.  The ONE table: the collect kernel
// (npp_demo.hip), the seed feed kernel (npp_seed.hip) and npp_archive_seed_rows_host read it here.
NPP_HD inline uint8_t demo_action_of_byte(uint32_t b) { return b < 8u ? (uint8_t)((0x00415230u >> (4u * b)) & 7u) : (uint8_t)0; }

// key_flags of npp_demo_create: the observation planes the player fills (NPP_DEMO_* of include/npp_amd.h)
enum DemoKeys : unsigned {
    DEMO_GAME_STATE = 1u << 0, DEMO_ACTION_MASK = 1u << 1, DEMO_ENTITY_POS = 1u << 2, DEMO_SPATIAL = 1u << 3, DEMO_REACH = 1u << 4,
    DEMO_MINE_SDF = 1u << 5, DEMO_SWITCH_STATES = 1u << 6, DEMO_POSITIONS = 1u << 7,
    DEMO_MASK_ENV = 1u << 16,   // action_mask holds npp_observe's mask instead of the executor's all ones
    DEMO_KEYS_ALL = 0xffu | DEMO_MASK_ENV
};

// The rule of ReplayExecutor.execute_replay's sampling (replay/replay_executor.py:433-460) and of the dataset's layout:
//   rows[r]      min(L / fs, max_transitions): a transition after every tick f with (f + 1) % fs == 0; the trailing L % fs ticks and
//                the ticks behind the cap yield nothing
//   row_base[r]  exclusive prefix sum of rows in the CALLER's order: the dataset is replay-major and time-ordered whatever the schedule
//   order        the replays with rows > 0 by descending rows, ties by index; round q plays order[q * n_envs .. ) one per env
//   round_ticks  max(rows) * fs of the round (its first replay's): ticks behind a replay's last sampled row still run for the envs that
//                share the round and are never observed
struct DemoPlan {
    std::vector<int32_t> rows, order, round_ticks;
    std::vector<int64_t> row_base;
    int64_t rows_total = 0;
};

inline bool demo_plan(const int64_t *lengths, int n_replays, int fs, int64_t max_transitions, int n_envs, DemoPlan &p, const char **why) {
    *why = nullptr;
    if (n_replays < 0 || (n_replays > 0 && !lengths)) { *why = "bad arguments"; return false; }
    if (fs < 1) { *why = "frame_skip must be >= 1"; return false; }
    if (n_envs < 1) { *why = "n_envs must be >= 1"; return false; }
    if (max_transitions < 0) { *why = "max_transitions must be >= 0"; return false; }
    for (int r = 0; r < n_replays; r++) {
        if (lengths[r] < 0) { *why = "negative replay length"; return false; }
        if (std::min(lengths[r] / fs, max_transitions) > INT32_MAX / 2) { *why = "replay too long"; return false; }
    }
    p = DemoPlan();
    p.rows.resize(n_replays);
    p.row_base.resize(n_replays);
    for (int r = 0; r < n_replays; r++) {
        p.rows[r] = (int32_t)std::min(lengths[r] / fs, max_transitions);
        p.row_base[r] = p.rows_total;
        p.rows_total += p.rows[r];
        if (p.rows[r] > 0) p.order.push_back(r);
    }
    std::stable_sort(p.order.begin(), p.order.end(), [&](int32_t a, int32_t b) { return p.rows[a] > p.rows[b]; });
    for (size_t i = 0; i < p.order.size(); i += (size_t)n_envs) {
        const int64_t t = (int64_t)p.rows[p.order[i]] * fs;
        if (t > INT32_MAX) { *why = "round too long"; p = DemoPlan(); return false; }
        p.round_ticks.push_back((int32_t)t);
    }
    return true;
}

}  // namespace npp
