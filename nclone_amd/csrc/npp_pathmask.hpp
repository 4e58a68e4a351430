// npp_pathmask.hpp -- path-direction action masking: the detector the reference's env runs at every observation and the mask stage
// it feeds.  One function, compiled for the host (npp_path_direction_host, the CPU parity test against tests/golden/pathmask.npz)
// and for the device (npp_pathmask.hip), so both run the same arithmetic, as reach_features does.
//
// Restates BaseEnvironment._detect_straight_path_direction (gym_environment/base_environment.py:3109-3253), which
// _get_action_mask_with_path_update (:3075-3107) calls for every observation, and the last stage of Ninja.get_valid_action_mask
// (ninja.py:743-800) that consumes its result in masking mode "hard".  What the detector goes through on the way:
//   * find_ninja_node(ninja_pos, adjacency, spatial_hash, subcell_lookup, ninja_radius=10.0) (pathfinding_utils.py:1331-1496) with
//     no goal node: the env's spatial hash has no `query`, so the call is the linear scan -- reach_near() + reach_pick(T, N, -1, 0);
//   * LevelBasedPathDistanceCache.get_multi_hop_direction(node, goal_id) (path_distance_cache.py:162-185) with the LITERAL goal ids
//     "switch" / "exit": table 0 / table 1 of ReachHdr::off_mh.  (Not ReachHdr::exit_gid: that goal-id inference belongs to
//     get_distance.)
// The graph is the one built at the spawn; graph updates inside an episode are not modelled, as for the reachability features.
#pragma once
#include "npp_reach_features.hpp"

namespace npp {

enum PathDir { PATH_NONE = 0, PATH_LEFT = 1, PATH_RIGHT = 2, PATH_DOWN = 3 };

// the mask stage (ninja.py:766-800): bit a of a keep-mask = action a (NOOP, LEFT, RIGHT, JUMP, JUMP+LEFT, JUMP+RIGHT) survives
constexpr unsigned PATH_KEEP_NONE = 0x3f;    // nothing removed
constexpr unsigned PATH_KEEP_LEFT = 0x03;    // NOOP, LEFT
constexpr unsigned PATH_KEEP_RIGHT = 0x05;   // NOOP, RIGHT
constexpr unsigned PATH_KEEP_DOWN = 0x07;    // the three jump actions removed
// the table of the four, one byte per direction (a shift instead of an indexed array: nothing to address on the device)
constexpr unsigned PATH_KEEP = PATH_KEEP_NONE | (PATH_KEEP_LEFT << 8) | (PATH_KEEP_RIGHT << 16) | (PATH_KEEP_DOWN << 24);
NPP_HD inline unsigned path_keep_mask(int direction) { return (PATH_KEEP >> (8 * (direction & 3))) & 0x3fu; }

// physics_constants.py:397-402
constexpr double STRAIGHT_PATH_HORIZONTAL_THRESHOLD = 0.8, STRAIGHT_PATH_VERTICAL_THRESHOLD = 0.1, STRAIGHT_PATH_DOWNWARD_THRESHOLD = 0.3,
                 STRAIGHT_PATH_MIN_DISTANCE = 12.0;

// 0 none, 1 left, 2 right, 3 down.  *from_graph = 1 when the direction was classified from the graph's multi-hop direction: the
// reference's `_deterministic_mask_applied_count += 1`.
NPP_HD inline __attribute__((always_inline)) int reach_path_direction(const ReachTabs &T, double px, double py, int switch_activated, int *from_graph) {
    const ReachHdr &H = *T.H;
    // the node gather first: its loads depend on the position only, so they are in flight while the goal distance is computed (the
    // near-goal branch below then drops them; the reference does no look-up there, and none has a side effect)
    const ReachNear N = reach_near(T, px, py);
    const int node = reach_pick(T, N, -1, 0);
    const int g = switch_activated ? 1 : 0;   // the goal: the exit door once the exit switch is activated, else the exit switch
    const double dx_goal = (double)(g ? H.goal_x[1] : H.goal_x[0]) - px, dy_goal = (double)(g ? H.goal_y[1] : H.goal_y[0]) - py;
    const double distance_to_goal = sqrt(dx_goal * dx_goal + dy_goal * dy_goal);   // (...) ** 0.5
    *from_graph = 0;
    if (distance_to_goal < STRAIGHT_PATH_MIN_DISTANCE) {   // line-of-sight hint; dx == 0 goes "right", but only under the inequality
        if (fabs(dx_goal) > fabs(dy_goal) * 2.0) return dx_goal < 0.0 ? PATH_LEFT : PATH_RIGHT;
        return PATH_NONE;
    }
    if (node < 0) return PATH_NONE;
    double dx, dy;
    if (g == 0) {   // goal "switch": the record's own entry
        const ReachNode q = reach_rec(T, N, node);
        dx = q.mh0x; dy = q.mh0y;
    } else {        // goal "exit": one more look-up, table 1 of off_mh
        const double *m = T.mh(1) + 2 * (long)node;
        dx = m[0]; dy = m[1];
    }
    if (dx != dx) return PATH_NONE;   // not cached: at the goal, or no path
    const bool is_horizontal = fabs(dy) < STRAIGHT_PATH_VERTICAL_THRESHOLD && fabs(dx) > STRAIGHT_PATH_HORIZONTAL_THRESHOLD;
    const bool is_downward = dy > STRAIGHT_PATH_DOWNWARD_THRESHOLD;
    if (is_horizontal) { *from_graph = 1; return dx < 0.0 ? PATH_LEFT : PATH_RIGHT; }
    if (is_downward) { *from_graph = 1; return PATH_DOWN; }
    return PATH_NONE;
}

}  // namespace npp
