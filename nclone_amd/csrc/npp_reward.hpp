// npp_reward.hpp -- reward mode "pbrs": the step reward of the reference's RewardCalculator.calculate_reward
// (gym_environment/reward_calculation/main_reward_calculator.py:225-904) as base_environment.step calls it (:644-657), with
// RewardConfig(enable_path_waypoints=False), no goal curriculum and no momentum waypoints.  One function, compiled for the host
// (npp_reward_host, the CPU parity test against tests/golden/reward.npz) and for the device (npp_reward.hip), so both run the same
// arithmetic, as reach_features and reach_path_direction do.  All arithmetic is fp64 (build with -ffp-contract=off).
//
// What the reference REALLY does, which is not what its docstrings say (DESIGN.md 20 lists every quirk with file:line):
//   * the potential is answered from a position cache whenever the ninja moved less than 6 px since the last full evaluation
//     (pbrs_potentials.py:1180-1358), with ANOTHER formula: 1 - max(0, node distance - projection) / max(1500, combined path), no
//     phase split, no radii; the cached node / distance / next hop are those of the path calculator's last
//     get_geometric_distance call that went through its fast path (path_distance_calculator.py:1872-1875), i.e. the feature
//     computation's query of feature 21, made only when the (24-px cell, switch) key of the observation changed;
//   * that query always names the goal "switch" (feature_computation.py:404: the switch handed over is a dict, `getattr(dict,
//     "active", True)` is True), so in the exit phase the record never matches and the calculator falls back to find_ninja_node on
//     the INTEGER position and the level cache's "exit" tables (pbrs_potentials.py:1316-1355);
//   * a hit without next hop returns the cached DISTANCE as the potential (:1281-1287);
//   * the two raw distances of the full evaluation are those of the last feature computation (reachability_mixin.py:213-216): stale
//     within a cell by design;
//   * `state["_pbrs_last_distance_to_goal"]` is written to a copy of the observation (pbrs_potentials.py:278, 1495), so
//     calculate_reward never sees it (:686) and runs its fallback: get_distance from the integer position with cache_key "switch" /
//     "exit" (:689-715) -- a second per-episode dictionary on the miss_exit levels.  The completion-approach bonus reads that number;
//   * the distance milestones read the position cache's node distance of the step BEFORE (get_last_distance_to_goal,
//     pbrs_potentials.py:1690-1706), and only when its goal matches.
#pragma once
#include "npp_reach_features.hpp"

namespace npp {

// npp_amd.h NppRewardParams (the same six doubles)
struct RewardParams {
    double death_penalty, level_completion_reward, switch_activation_reward, time_penalty_per_step, pbrs_objective_weight, pbrs_gamma;
};

// per-level constants (npp_reach.cpp reward_level_constants): PBRSCalculator._compute_combined_path_distance
struct RewardLevel {
    double spawn_to_switch, switch_to_exit, combined;
    uint32_t supported;   // 0: the reference raises on this level, or a part of it that is not restated would run
    uint32_t pad_;
};

constexpr double REWARD_MILESTONE = 30.0;             // SUB_GOAL_REWARD_PROGRESS, reward_constants.py:236
constexpr double REWARD_MILESTONE_INTERVAL = 48.0;    // _milestone_interval_px, main_reward_calculator.py:217
constexpr double REWARD_APPROACH_RADIUS = 100.0;      // COMPLETION_APPROACH_RADIUS, main_reward_calculator.py:2521
constexpr double REWARD_APPROACH_MAX = 5.0;           // COMPLETION_APPROACH_MAX_BONUS, main_reward_calculator.py:2522
constexpr double REWARD_MIN_SCALE = 50.0;             // MIN_SCALE, pbrs_potentials.py:312
constexpr double REWARD_MIN_NORMALIZATION = 1500.0;   // MIN_NORMALIZATION, pbrs_potentials.py:1271
constexpr double REWARD_GRADIENT_REFERENCE = 200.0;   // PBRS_GRADIENT_REFERENCE_DISTANCE, reward_constants.py:350
constexpr double REWARD_GRADIENT_CAP = 7.0;           // PBRS_GRADIENT_SCALE_CAP, reward_constants.py:351
constexpr double REWARD_SCALE = 0.1;                  // GLOBAL_REWARD_SCALE, reward_constants.py:71
constexpr double REWARD_CACHE_THRESHOLD_SQ = 36.0;    // _position_cache_threshold_sq, pbrs_potentials.py:829 (recorded by the fixture)

// valid bits and small fields of RewardState::bits
enum : uint32_t {
    RW_LAST_POS = 1u << 0,      // PBRSCalculator._last_player_pos is not None
    RW_CDIST = 1u << 1,         // _cached_distance is not None
    RW_PREV_POT = 1u << 2,      // RewardCalculator.prev_potential is not None
    RW_MS_SW = 1u << 3,         // _last_milestone_distance_to_switch is not None
    RW_MS_EX = 1u << 4,         // _last_milestone_distance_to_exit is not None
    RW_PREV_POS = 1u << 5,      // prev_player_pos is not None
    RW_OPTIMAL = 1u << 6,       // optimal_path_length is not None
    RW_PREV_SWITCH = 1u << 7,   // prev_obs["switch_activated"]
    RW_LAST_GOAL = 3u << 8,     // PBRSCalculator._last_goal_id: 0 None, 1 "switch", 2 "exit"
};

// Per-env state.  On the device: SoA planes (RW_ND doubles, RW_NI words per env), allocated when the mode is switched on.
struct RewardState {
    // doubles, in plane order
    double d_sw, d_ex;                 // _cached_switch_distance / _cached_exit_distance of the last feature computation
    double pc_dist;                    // path calculator: _last_geometric_distance
    double last_x, last_y;             // PBRS position cache: _last_player_pos
    double c_dist;                     // _cached_distance
    double prev_potential;
    double ms_sw, ms_ex;               // the two milestone distances
    double path_len;                   // episode_path_length
    double prev_x, prev_y;             // prev_player_pos
    double optimal;                    // optimal_path_length
    // words, in plane order
    uint32_t key;                      // reward cache key: 0 none, else 0x80000000 | cell x | cell y << 14 | switch << 28 (as npp_reach_kernel)
    int32_t pc_node, pc_hop;           // path calculator: _last_start_node / _last_next_hop (-1 = None); its _last_goal_id is "switch"
                                       // whenever the node is set (see the header comment).  NOT reset at an episode end.
    int32_t c_node, c_hop;             // _cached_start_node / _cached_next_hop (-1 = None)
    uint32_t bits;
    uint32_t epoch2;                   // epoch of the fallback query's dictionary (never 0)
};
constexpr int RW_ND = 13, RW_NI = 7;

struct RewardOut {
    double reward;                     // scaled by GLOBAL_REWARD_SCALE
    double pbrs, dist_milestone, switch_milestone, approach, terminal, potential;   // unscaled components
    int kind;                          // 0 position-cache miss, 1 hit, 2 hit without next hop, 3 no potential was evaluated
};

NPP_HD inline void reward_state_init(RewardState &S) {
    S.d_sw = S.d_ex = INFINITY;
    S.pc_dist = 0.0; S.last_x = S.last_y = 0.0; S.c_dist = 0.0; S.prev_potential = 0.0; S.ms_sw = S.ms_ex = 0.0;
    S.path_len = 0.0; S.prev_x = S.prev_y = 0.0; S.optimal = 0.0;
    S.key = 0u; S.pc_node = S.pc_hop = -1; S.c_node = S.c_hop = -1; S.bits = 0u; S.epoch2 = 1u;
}

// RewardCalculator.reset() (:1072-1163) + PBRSCalculator.reset() (pbrs_potentials.py:1667-1683) + the env's reset: the cache key is
// dropped, the fallback's dictionary is emptied (clear_cache(), reachability_mixin.py:67-70).  The path calculator's last-call record
// survives, as in the reference.
NPP_HD inline void reward_restart(RewardState &S) {
    S.bits = 0u;
    S.c_node = S.c_hop = -1;
    S.path_len = 0.0;
    S.key = 0u;
    S.epoch2 = S.epoch2 + 1u == 0u ? 1u : S.epoch2 + 1u;
}

// The observation's part: ReachabilityMixin._compute_reachability (reachability_mixin.py:150-222).  On a key change the distance
// queries of compute_reachability_features_from_graph run in its order (feature_computation.py:402-485, 755-785), through the
// dictionary M it shares with npp_reachability, and the geometric query of feature 21 leaves the path calculator's record.
NPP_HD inline __attribute__((always_inline)) void reward_observe(const ReachTabs &T, RewardState &S, double px, double py, int sw, ReachMiss *M) {
    const ReachHdr &H = *T.H;
    const int cx = reach_cell24(px), cy = reach_cell24(py);
    const uint32_t k = 0x80000000u | ((uint32_t)(cx & 0x3fff)) | ((uint32_t)(cy & 0x3fff) << 14) | ((uint32_t)(sw ? 1 : 0) << 28);
    if (S.key == k) return;
    S.key = k;
    bool miss = false;
    const ReachNear N = reach_near(T, px, py);
    double d_sw = INFINITY, d_ex = INFINITY;
    if (H.sw_valid) d_sw = reach_goal_distance(T, N, px, py, 0, 6.0, M, false, &miss);
    if (d_sw == INFINITY && H.ex_valid) (void)reach_goal_distance(T, N, px, py, 1, 12.0, M, false, &miss);   // "next objective": third priority
    if (H.ex_valid) d_ex = reach_goal_distance(T, N, px, py, 1, 12.0, M, false, &miss);
    S.d_sw = d_sw; S.d_ex = d_ex;
    if (d_sw != INFINITY) {
        // get_geometric_distance(ninja_pos, switch_pos, ..., goal_id="switch") (path_distance_calculator.py:1487-1890): the record is
        // written on its fast path only, behind the radius early exit and with a next hop
        const double dx = px - H.goal_x[0], dy = py - H.goal_y[0];
        if (!(dx * dx + dy * dy <= 16.0 * 16.0)) {
            const int sn = reach_pick(T, N, H.goal_node[2], 0);
            if (sn >= 0) {
                const ReachNode q = reach_rec(T, N, sn);
                if (q.dist0 != INFINITY && q.hop0 >= 0) { S.pc_node = sn; S.pc_dist = q.dist0; S.pc_hop = q.hop0; }
            }
        }
    }
}

NPP_HD inline double reward_max(double a, double b) { return b > a ? b : a; }   // Python's max(a, b)
NPP_HD inline double reward_min(double a, double b) { return b < a ? b : a; }   // Python's min(a, b)

// PBRSPotentials.objective_distance_potential (pbrs_potentials.py:158-371) given the distance it is handed.  phase 0 switch, 1 exit;
// (ex, ey): goal - player on the integer positions, used when the distance is +inf
NPP_HD inline double reward_objective_potential(double distance, int phase, double spawn_to_switch, double switch_to_exit, double ex, double ey) {
    if (distance == INFINITY) distance = sqrt(ex * ex + ey * ey);
    double k, raw;
    if (!phase) k = reward_max(REWARD_MIN_SCALE, spawn_to_switch);
    else k = reward_max(REWARD_MIN_SCALE, (spawn_to_switch + switch_to_exit) * 2.0);
    const double nd = distance / k;
    if (nd <= 1.0) raw = 1.0 - nd;
    else raw = 1.0 / (1.0 + (nd - 1.0));
    const double potential = phase ? 0.5 + 0.5 * raw : 0.5 * raw;
    return reward_max(0.0, reward_min(1.0, potential));
}

// _calculate_completion_approach_bonus (main_reward_calculator.py:2486-2538); `proximity_ratio ** 2` as a product
NPP_HD inline double reward_approach_bonus(double distance_to_goal) {
    if (distance_to_goal == INFINITY) return 0.0;
    if (distance_to_goal >= REWARD_APPROACH_RADIUS) return 0.0;
    const double r = 1.0 - (distance_to_goal / REWARD_APPROACH_RADIUS);
    return REWARD_APPROACH_MAX * (r * r);
}

// (x ** 2 + y ** 2) ** 0.5 of a hop between lattice nodes: 12 for a cardinal one, 288 ** 0.5 for a diagonal one
NPP_HD inline double reward_hop_len(double pdx, double pdy) { return (pdx != 0.0 && pdy != 0.0) ? 16.970562748477139 : 12.0; }

// One call of calculate_reward for the step whose flags byte is `flags` (NPP_F_WON / NPP_F_DEAD / NPP_F_SWITCH / NPP_F_TRUNCATED of the
// state the step ended in) and which ran `frames` ticks; (px, py, sw_now) is the env's state NOW: the state the step ended in, or,
// when (flags & end_bits) -- the step kernel auto-reset the env -- the state after that reset.  M: the dictionary shared with
// npp_reachability, already on the env's current episode; M2: the arrays of the fallback query's own (its epoch is the state's).  Neither
// pointer is null; a null `stamp` inside means "no dictionary" (no level of the set takes the miss branch).  wp_on: the path
// waypoints are on and wp_bonus is the step's sequential waypoint bonus (npp_waypoint.hpp), added on a live step where the reference adds it.
NPP_HD inline __attribute__((always_inline)) RewardOut reward_step(const ReachTabs &T, const RewardLevel &RL, const RewardParams &P, RewardState &S, double px, double py,
                                                               int sw_now, unsigned flags, int frames, unsigned end_bits, ReachMiss *M, ReachMiss *M2,
                                                               bool wp_on = false, double wp_bonus = 0.0) {
    const ReachHdr &H = *T.H;
    RewardOut o;
    o.reward = o.pbrs = o.dist_milestone = o.switch_milestone = o.approach = o.terminal = o.potential = 0.0;
    o.kind = 3;
    const bool won = (flags & 1u) != 0, dead = (flags & 2u) != 0, sw = (flags & 4u) != 0;
    const bool ended = (flags & end_bits) != 0;
    const bool just = sw && !(S.bits & RW_PREV_SWITCH);
    const double milestone = just ? P.switch_activation_reward : 0.0;
    o.switch_milestone = milestone;
    if (dead) {   // :318-363
        o.terminal = P.death_penalty + milestone;
        o.reward = o.terminal * REWARD_SCALE;
    } else if (won) {   // :367-414
        double terminal = P.level_completion_reward;
        if ((S.bits & RW_OPTIMAL) && S.optimal > 0.0 && S.path_len > 0.0) {
            const double eff = S.optimal / S.path_len;
            terminal += P.level_completion_reward * 0.5 * reward_min(1.0, eff);
        }
        o.terminal = terminal;
        o.reward = (terminal + milestone) * REWARD_SCALE;
    } else if (ended) {
        // truncated and auto-reset: the reference evaluates a live step at the final position, which the reset has overwritten.  Known
        // deviation: time penalty and switch milestone only
        double reward = P.time_penalty_per_step * (double)frames;
        if (just) reward += P.switch_activation_reward;
        o.reward = reward * REWARD_SCALE;
    } else {
        reward_observe(T, S, px, py, sw ? 1 : 0, M);   // final_obs = self._get_observation()
        double reward = P.time_penalty_per_step * (double)frames;   // :419
        if (just) reward += P.switch_activation_reward;   // :429
        const int g = sw ? 1 : 0;
        const uint32_t last_goal = (S.bits & RW_LAST_GOAL) >> 8;
        {   // _check_distance_milestones (:906-970) on get_last_distance_to_goal (pbrs_potentials.py:1690-1706)
            const bool have = last_goal == (uint32_t)(g + 1) && (S.bits & RW_CDIST);
            if (have) {
                const double d = S.c_dist;
                const uint32_t vb = g ? RW_MS_EX : RW_MS_SW;
                double &ms = g ? S.ms_ex : S.ms_sw;
                if (!(S.bits & vb)) { ms = d; S.bits |= vb; }
                else if (d < ms - REWARD_MILESTONE_INTERVAL) { o.dist_milestone = REWARD_MILESTONE; ms = d; }
            }
        }
        reward += o.dist_milestone;
        // calculate_combined_potential (pbrs_potentials.py:1408-1636)
        const double combined = RL.combined != 0.0 ? RL.combined : REWARD_GRADIENT_REFERENCE;   // `x or 200.0`
        const double gradient_scale = reward_min(sqrt(combined / REWARD_GRADIENT_REFERENCE), REWARD_GRADIENT_CAP);
        const double scaled_weight = P.pbrs_objective_weight * gradient_scale;
        const double ipx = trunc(px), ipy = trunc(py);   // int(state["player_x"])
        double objective = 0.0;
        bool answered = false;
        // _get_cached_or_compute_potential (pbrs_potentials.py:1180-1358)
        if ((S.bits & RW_LAST_POS) && last_goal == (uint32_t)(g + 1) && (S.bits & RW_CDIST) && S.c_node >= 0) {
            const double dx = px - S.last_x, dy = py - S.last_y;
            if (dx * dx + dy * dy < REWARD_CACHE_THRESHOLD_SQ) {
                answered = true;
                o.kind = S.c_hop >= 0 ? 1 : 2;
                objective = S.c_dist;   // no next hop: "this is actually cached potential in this case" -- it is the distance
                if (S.c_hop >= 0) {
                    const double snx = (double)(reach_node_x(S.c_node) + 24), sny = (double)(reach_node_y(S.c_node) + 24);
                    const double pdx = (double)(reach_node_x(S.c_hop) + 24) - snx, pdy = (double)(reach_node_y(S.c_hop) + 24) - sny;
                    const double plen = reward_hop_len(pdx, pdy);
                    const double dirx = pdx / plen, diry = pdy / plen;
                    const double projection = (px - snx) * dirx + (py - sny) * diry;
                    const double interpolated = reward_max(0.0, S.c_dist - projection);
                    const double norm = reward_max(REWARD_MIN_NORMALIZATION, RL.combined);
                    objective = reward_max(0.0, reward_min(1.0, 1.0 - interpolated / norm));
                }
            }
        }
        if (!answered) {
            o.kind = 0;
            const int gx = g ? H.goal_x[1] : H.goal_x[0], gy = g ? H.goal_y[1] : H.goal_y[0];
            if (gx == 0 && gy == 0) objective = 0.0;
            else objective = reward_objective_potential(g ? S.d_ex : S.d_sw, g, RL.spawn_to_switch, RL.switch_to_exit, (double)gx - ipx, (double)gy - ipy);
            S.last_x = px; S.last_y = py;
            S.bits = (S.bits & ~RW_LAST_GOAL) | RW_LAST_POS | ((uint32_t)(g + 1) << 8);
            if (S.pc_node >= 0 && g == 0) {   // the record's goal id is "switch"
                S.c_node = S.pc_node; S.c_dist = S.pc_dist; S.c_hop = S.pc_hop;
                S.bits |= RW_CDIST;
            } else {   // find_ninja_node on the integer position, then the level cache's tables of the LITERAL goal id
                const ReachNear NI = reach_near(T, ipx, ipy);
                const int start = reach_pick(T, NI, -1, 0);
                if (start >= 0) {   // (both goals exist on every level the mode accepts; no node: everything stays as it was)
                    const ReachNode q = reach_rec(T, NI, start);
                    S.c_node = start;
                    if (q.dist(g) != INFINITY) { S.c_dist = q.dist(g); S.bits |= RW_CDIST; }
                    S.c_hop = q.hop(g);
                }
            }
        }
        const double potential = (1.0 * objective) * scaled_weight;   // PBRS_SWITCH_DISTANCE_SCALE = PBRS_EXIT_DISTANCE_SCALE = 1.0
        o.potential = potential;
        if (S.bits & RW_PREV_POS) {   // :516-521
            const double dx = px - S.prev_x, dy = py - S.prev_y;
            S.path_len += sqrt(dx * dx + dy * dy);
        }
        S.prev_x = px; S.prev_y = py; S.bits |= RW_PREV_POS;
        if (!(S.bits & RW_OPTIMAL)) { S.optimal = RL.combined; S.bits |= RW_OPTIMAL; }   // :540-541
        if (S.bits & RW_PREV_POT) o.pbrs = P.pbrs_gamma * potential - S.prev_potential;   // :548-585
        S.prev_potential = potential; S.bits |= RW_PREV_POT;
        reward += o.pbrs;   // (the sequential waypoint bonus of :662-667 is 0.0 with waypoints off)
        if (wp_on) reward += wp_bonus;         // waypoints on: what npp_waypoint.hpp computed for this step (:667)
        {   // distance_to_goal: the fallback of :689-715, get_distance from the integer position with its own cache key
            const ReachNear NI = reach_near(T, ipx, ipy);
            bool miss = false;
            // (the switch's query never reads this dictionary: no entry carries its cache key.  A null `stamp` is "no dictionary")
            ReachMiss Mq{g ? M2->stamp : nullptr, M2->raw, S.epoch2};
            const double d = reach_goal_distance(T, NI, ipx, ipy, g, g ? 12.0 : 6.0, &Mq, false, &miss);
            o.approach = reward_approach_bonus(d);
        }
        reward += o.approach;
        o.reward = reward * REWARD_SCALE;
    }
    S.bits = (S.bits & ~RW_PREV_SWITCH) | (sw ? RW_PREV_SWITCH : 0u);
    if (ended) {   // the env's reset: calculator state, cache key, and the observation of the reset state (the next step's prev_obs)
        reward_restart(S);
        reward_observe(T, S, px, py, sw_now, M);
        S.bits = (S.bits & ~RW_PREV_SWITCH) | (sw_now ? RW_PREV_SWITCH : 0u);
    }
    return o;
}

}  // namespace npp
