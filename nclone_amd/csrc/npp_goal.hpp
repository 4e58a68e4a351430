// npp_goal.hpp -- the goal curriculum (include/npp_amd.h, npp_set_goal_curriculum): the reference's IntermediateGoalManager
// (gym_environment/reward_calculation/intermediate_goal_manager.py) and GoalCurriculumConfig (reward_config.py:953-983).  The exit
// switch and the exit door slide along the level's optimal path in stages; a (level, stage) pair is a VARIANT LEVEL -- the same tiles,
// mines and spawn with the two entities elsewhere (npp_level.hpp: compile_level_variant) -- so every consumer of a level serves it.
// Here: the stage table (host, fp64, no contraction) and the bookkeeping rule shared by the device kernels (npp_goal.hip), the
// host-only entry point (npp_reach.cpp: npp_goal_apply_host) and restated in tests/goal_ref.py.  No HIP header: the host sources also
// build with plain g++.
#pragma once
#include <cmath>
#include <cstdint>
#include <vector>

#include "npp_state.hpp"   // NPP_HD

namespace npp {

// ---- stage table (host) ----------------------------------------------------------------------------------------------------
// paths in tile-data space, as the manager keeps them (node x, y; world = node + 24)
struct GoalPath {
    std::vector<int> x, y;
    size_t size() const { return x.size(); }
};

struct GoalStages {
    GoalPath path[2];              // spawn -> switch, switch -> exit (build_paths_for_level, :158-336)
    bool combined = false;         // both paths were found: _combined_path is not empty
    double d_switch = 0.0, d_exit = 0.0, d_combined = 0.0;
    int num_stages = 0;            // 0: the level has no stages and stays on its base level
    double orig[4] = {0, 0, 0, 0}; // original switch x, y, door x, y
    std::vector<double> pos;       // [max(num_stages, 1)][4]: the two getters at every stage (row 0 of a level without stages: stage 0)
};

// _compute_path_distance (:338-358)
inline double goal_path_distance(const GoalPath &p) {
    if (p.size() < 2) return 0.0;
    double total = 0.0;
    for (size_t i = 1; i < p.size(); i++) {
        const double dx = (double)(p.x[i] - p.x[i - 1]), dy = (double)(p.y[i] - p.y[i - 1]);
        total += std::sqrt(dx * dx + dy * dy);
    }
    return total;
}

// _sample_position_at_distance (:484-546)
inline void goal_sample(const GoalPath &p, double target, double &ox, double &oy) {
    const size_t n = p.size();
    if (n < 2) {
        if (n == 1) { ox = (double)p.x[0] + 24.0; oy = (double)p.y[0] + 24.0; }
        else { ox = 0.0; oy = 0.0; }
        return;
    }
    std::vector<double> cum(n, 0.0);
    for (size_t i = 1; i < n; i++) {
        const double dx = (double)(p.x[i] - p.x[i - 1]), dy = (double)(p.y[i] - p.y[i - 1]);
        cum[i] = cum[i - 1] + std::sqrt(dx * dx + dy * dy);
    }
    const double total = cum[n - 1];
    target = std::fmax(0.0, std::fmin(target, total));
    if (target <= 0) { ox = (double)p.x[0] + 24.0; oy = (double)p.y[0] + 24.0; return; }
    if (target >= total) { ox = (double)p.x[n - 1] + 24.0; oy = (double)p.y[n - 1] + 24.0; return; }
    size_t hi = 0;   // bisect_right: the first index with cum > target
    while (hi < n && !(cum[hi] > target)) hi++;
    long seg = (long)hi - 1;
    if (seg < 0) seg = 0;
    if (seg > (long)n - 2) seg = (long)n - 2;
    const double len = cum[seg + 1] - cum[seg];
    const double t = len > 0 ? (target - cum[seg]) / len : 0.0;
    ox = ((double)p.x[seg] + t * (double)(p.x[seg + 1] - p.x[seg])) + 24.0;
    oy = ((double)p.y[seg] + t * (double)(p.y[seg + 1] - p.y[seg])) + 24.0;
}

// get_curriculum_switch_position (:570-638) / get_curriculum_exit_position (:640-696) at `stage`
inline void goal_positions(const GoalStages &G, double interval, int stage, double out[4]) {
    if (G.path[0].size() == 0) { out[0] = G.orig[0]; out[1] = G.orig[1]; }
    else goal_sample(G.path[0], std::fmin((double)(stage + 1) * interval, G.d_switch), out[0], out[1]);
    if (!G.combined) { out[2] = G.orig[2]; out[3] = G.orig[3]; return; }
    const double d = std::fmin((double)(stage + 2) * interval, G.d_combined);
    if (d <= G.d_switch) goal_sample(G.path[0], d, out[2], out[3]);
    else goal_sample(G.path[1], d - G.d_switch, out[2], out[3]);
}

// what build_paths_for_level leaves behind once the two paths are known (:296-315), and the getters at every stage
inline void goal_finish_stages(GoalStages &G, double interval) {
    if (G.combined) {
        G.d_switch = goal_path_distance(G.path[0]);
        G.d_exit = goal_path_distance(G.path[1]);
        G.d_combined = G.d_switch + G.d_exit;
        // _compute_num_stages (:427-440)
        if (G.d_combined <= 0) G.num_stages = 2;
        else {
            const long q = (long)(G.d_combined / interval) + 1;
            G.num_stages = (int)(q < 2 ? 2 : q);
        }
    }
    const int rows = G.num_stages > 0 ? G.num_stages : 1;
    G.pos.assign((size_t)rows * 4, 0.0);
    for (int s = 0; s < rows; s++) goal_positions(G, interval, s, G.pos.data() + 4 * (size_t)s);
}

struct CompiledLevel;
struct ReachBuilt;
// npp_reach.cpp, on the searches of DESIGN.md section 23: the manager's two paths from the ORIGINAL positions and the stage table.
// false: interval is not a positive finite number, or the level would have more than GOAL_MAX_STAGES stages
constexpr int GOAL_MAX_STAGES = 1024;
bool goal_stage_table(const CompiledLevel &level, const ReachBuilt &R, double interval, GoalStages &out);

// ---- bookkeeping rule (device + host) --------------------------------------------------------------------------------------
// Per base level, i32 planes [GL_N][n_base]; the ring of the last `window` outcomes as bits, u32[n_base][ring_words].
enum GoalLevelWord {
    GL_STAGE = 0, GL_PENDING /* -1 = none */, GL_NUM_STAGES, GL_VARIANT0 /* level id of stage 0; stage s = + s */, GL_FILL, GL_HEAD /* next slot */,
    GL_WINS, GL_ADVANCES, GL_APPENDED, GL_STALE, GL_N
};
// Per env, i32 planes [GE_N][n]: the counters of update_from_episode (:1014-1038), the switch latch of the running episode, and the
// level the env played when its episode ended (what the assignment compares with)
enum GoalEnvWord { GE_EPISODES = 0, GE_SWITCHES, GE_COMPLETIONS, GE_SEEN, GE_PREV, GE_N };
constexpr int GOAL_MAX_WINDOW = 8192;
constexpr int GOAL_F_WON = 1, GOAL_F_SWITCH = 4;   // NPP_F_WON, NPP_F_SWITCH

struct GoalState {
    int32_t *lv;          // [GL_N][n_base]
    uint32_t *ring;       // [n_base][ring_words]
    int32_t *env;         // [GE_N][n]
    const int32_t *base_of;    // [n_levels] base level of a level (itself for a base level)
    const int32_t *stage_of;   // [n_levels] stage of a variant, -1 for a base level
    int n_base, n, ring_words, window, need, auto_advance;
};
NPP_HD inline int32_t &goal_lv(const GoalState &g, int word, int level) { return g.lv[(size_t)word * g.n_base + level]; }
NPP_HD inline int32_t &goal_env(const GoalState &g, int word, int env) { return g.env[(size_t)word * g.n + env]; }

// the smallest w with (double)w / (double)window >= threshold (window + 1: no count reaches it)
inline int goal_need(int window, double threshold) {
    for (int w = 0; w <= window; w++)
        if ((double)w / (double)window >= threshold) return w;
    return window + 1;
}

// Rule 1, the env's half: one step row.  `ended` = the row ended the episode and outcomes are counted.  The switch latch takes the
// flag of rows that did NOT end the episode (under auto-reset the ending row's bit describes the state after the reset); a win
// implies the switch.  Returns nothing: the level's half reads the flags again.  goal_env_restart is the env's half of an explicit
// restart (npp_reset, npp_draw_levels: nothing is counted): the abandoned episode's latch goes with it.
NPP_HD inline void goal_env_row(const GoalState &g, int env, int flags, bool ended, int level_now) {
    if (ended) {
        const bool won = (flags & GOAL_F_WON) != 0;
        goal_env(g, GE_EPISODES, env) = (int32_t)((uint32_t)goal_env(g, GE_EPISODES, env) + 1u);
        if (won || goal_env(g, GE_SEEN, env)) goal_env(g, GE_SWITCHES, env) = (int32_t)((uint32_t)goal_env(g, GE_SWITCHES, env) + 1u);
        if (won) goal_env(g, GE_COMPLETIONS, env) = (int32_t)((uint32_t)goal_env(g, GE_COMPLETIONS, env) + 1u);
        goal_env(g, GE_SEEN, env) = 0;
        goal_env(g, GE_PREV, env) = level_now;
    } else if ((flags & GOAL_F_SWITCH) && !goal_env(g, GE_SEEN, env)) {
        goal_env(g, GE_SEEN, env) = 1;
    }
}

NPP_HD inline void goal_env_restart(const GoalState &g, int env, int level_now) {
    goal_env(g, GE_SEEN, env) = 0;
    goal_env(g, GE_PREV, env) = level_now;
}

// Rule 1, the level's half: an episode of `level` (a base level with stages), played at `stage`, ended with `won`
NPP_HD inline void goal_append(const GoalState &g, int level, int stage, bool won) {
    if (stage != goal_lv(g, GL_STAGE, level)) {   // played at a stale stage: not appended
        goal_lv(g, GL_STALE, level)++;
        return;
    }
    uint32_t *ring = g.ring + (size_t)level * g.ring_words;
    const int head = goal_lv(g, GL_HEAD, level);
    const uint32_t bit = 1u << (head & 31);
    if (goal_lv(g, GL_FILL, level) == g.window) goal_lv(g, GL_WINS, level) -= (ring[head >> 5] & bit) ? 1 : 0;   // the oldest leaves
    else goal_lv(g, GL_FILL, level)++;
    if (won) { ring[head >> 5] |= bit; goal_lv(g, GL_WINS, level)++; }
    else ring[head >> 5] &= ~bit;
    goal_lv(g, GL_HEAD, level) = head + 1 == g.window ? 0 : head + 1;
    goal_lv(g, GL_APPENDED, level)++;
}

// Rules 2 and 3 for one base level: the advance (`count` = outcomes were counted in this call), then a host-set pending stage
NPP_HD inline void goal_finish(const GoalState &g, int level, bool count) {
    const int ns = goal_lv(g, GL_NUM_STAGES, level);
    if (count && g.auto_advance && goal_lv(g, GL_FILL, level) == g.window && goal_lv(g, GL_WINS, level) >= g.need &&
        goal_lv(g, GL_STAGE, level) < ns - 1) {
        goal_lv(g, GL_STAGE, level)++;
        goal_lv(g, GL_ADVANCES, level)++;
        goal_lv(g, GL_FILL, level) = 0; goal_lv(g, GL_HEAD, level) = 0; goal_lv(g, GL_WINS, level) = 0;
    }
    const int p = goal_lv(g, GL_PENDING, level);
    if (p >= 0) {
        goal_lv(g, GL_STAGE, level) = ns > 0 ? (p < ns - 1 ? p : ns - 1) : 0;
        goal_lv(g, GL_PENDING, level) = -1;
    }
}

// Rule 3, the env's half: the level an env starts its next episode on, given the level it holds now (a variant, or the base level
// the pool just drew)
NPP_HD inline int goal_level_for(const GoalState &g, int level_now) {
    const int b = g.base_of[level_now];
    return goal_lv(g, GL_NUM_STAGES, b) > 0 ? goal_lv(g, GL_VARIANT0, b) + goal_lv(g, GL_STAGE, b) : b;
}

}  // namespace npp
