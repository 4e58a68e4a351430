/*
 * npp_amd.h -- C ABI of the MI355X batched N++ environment stepper.
 *
 * The reference (Tetramputechture/nclone) is pure Python and has no FFI seam; the seam it
 * does have is the object protocol of NPlayHeadless (nclone/nplay_headless.py:28) under the
 * Gymnasium surface of NppEnvironment (nclone/gym_environment/base_environment.py:483 step,
 * npp_environment.py:504 reset).  Each entry point below names the reference interface it
 * replaces for N environments at once.  INTEGRATION.md shows the ctypes stub a maintainer of
 * the reference would add.
 *
 * Conventions
 *   - plain C types only; every function returns an int status (0 = NPP_OK);
 *     npp_last_error(h) returns a human-readable message for the last failure on h
 *     (h may be NULL for errors raised by npp_create).
 *   - "d_" parameters are DEVICE-ACCESSIBLE pointers (hipMalloc'ed or hipHostMalloc'ed pinned
 *     host memory); everything else is ordinary host memory.
 *   - calls are asynchronous and ordered on the handle's HIP stream; npp_sync blocks.
 *   - one host thread per handle.  One handle per GPU (one process per GPU for multi-GPU).
 *   - all arithmetic of the physics path is IEEE fp64 without fused contraction, as in the
 *     reference (CPython floats).
 */
#ifndef NPP_AMD_H
#define NPP_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct npp_handle_s *npp_handle;

enum {
    NPP_OK = 0,
    NPP_ERR_INVALID = 1,     /* bad argument */
    NPP_ERR_HIP = 2,         /* HIP runtime failure (message has the hipError string) */
    NPP_ERR_UNSUPPORTED = 3, /* level uses entity types outside the accelerated path */
    NPP_ERR_STATE = 4        /* call order (e.g. step before levels were loaded) */
};

/* npp_create flags */
enum {
    NPP_FLAG_AUTORESET = 1u << 0,         /* reset an env in-kernel when it terminates/truncates
                                             (vector-env semantics; obs returned is the reset obs) */
    NPP_FLAG_ALLOW_UNSUPPORTED = 1u << 1, /* load levels with unsupported entity types, ignoring
                                             those entities (they are skipped, never simulated) */
    NPP_FLAG_FRAME_CENTERED = 1u << 2,    /* player_frame cropped around (x, y) as intended; default (0) reproduces
                                             the reference's axis-swapped crop (observation_processor.py:219-231) */
    NPP_FLAG_FAST_RESET = 1u << 3         /* every reset after the first one of a level assignment has the semantics of
                                             Simulator.fast_reset (nsim.py:78-140), which NppEnvironment.reset uses for
                                             same-level resets (npp_environment.py:541-557): entities are reset in place,
                                             so (a) the per-cell entity lists are rebuilt in entity_dic order (type key,
                                             then creation order) instead of map order, and (b) entities whose class has
                                             no reset_state() (drones, thwumps, bounce blocks, death balls, shove thwumps,
                                             regular doors, boost pads) keep position and state, only `active` is set.
                                             Default (0): every reset is Simulator.reset (nsim.py:62-76). */
};

/* out_flags bits written by npp_step */
enum {
    NPP_F_WON = 1u << 0,        /* ninja.has_won()  (ninja.py:1396)  */
    NPP_F_DEAD = 1u << 1,       /* ninja.has_died() (ninja.py:1399)  */
    NPP_F_SWITCH = 1u << 2,     /* exit_switch_activated() (nplay_headless.py:566) */
    NPP_F_TRUNCATED = 1u << 3,  /* sim.frame >= limit (truncation_checker.py:46-77) */
    NPP_F_CAUSE_MINE = 1u << 4, /* ninja.death_cause == "mine" */
    NPP_F_CAUSE_IMPACT = 1u << 5/* ninja.death_cause == "terminal_impact" */
};

#define NPP_GAME_STATE_DIM 41   /* gym_environment/constants.py:25 */
#define NPP_ACTION_DIM 6        /* base_environment.py:150 Discrete(6) */
#define NPP_ENTITY_POS_DIM 6    /* observation_processor.py:340-361 */
#define NPP_SPATIAL_CONTEXT_DIM 112 /* gym_environment/constants.py SPATIAL_CONTEXT_DIM */
#define NPP_MINIMAL_OBS_DIM 40  /* gym_environment/constants.py MINIMAL_OBSERVATION_DIM */
#define NPP_FRAME_W 84          /* gym_environment/constants.py:12-13 */
#define NPP_FRAME_H 84
#define NPP_DUMP_F64 12
#define NPP_DUMP_I32 32

/* Output block of npp_step.  Any pointer may be NULL (that output is skipped). */
typedef struct {
    float *d_game_state;      /* [N,41] f32: get_ninja_state() (nplay_headless.py:735-924) + time_remaining
                                 (base_environment.py:2811-2829), cast like observation_processor.py:284-302 */
    int8_t *d_action_mask;    /* [N,6]  i8 : ninja.get_valid_action_mask() (ninja.py:628-839) */
    float *d_entity_pos;      /* [N,6]  f32: [ninja, exit switch, exit door] / (1056, 600) */
    uint8_t *d_flags;         /* [N]    u8 : NPP_F_* of the state the step ended in (before auto-reset) */
    float *d_reward;          /* [N]    f32: sparse terminal reward only */
    uint16_t *d_frames;       /* [N]    u16: ticks executed this step (info["frame_skip_stats"]) */
    float *d_terminal_state;  /* [N,41] f32: game_state of the terminal state for envs that were
                                 auto-reset this step (rows of other envs are left untouched) */
    float *d_spatial_context; /* [N,112] f32: 8x8 local tile categories + 8 nearest mines x 6 features
                                 (gym_environment/spatial_context.py:113-176,309-508 as called from
                                 npp_environment.py:2318-2360, incl. its >= 12 px position cache) */
    double *d_positions;      /* [N,6]  f64: player_x, player_y, switch_x, switch_y, exit_door_x, exit_door_y in pixels:
                                 the pass-through scalars of the raw observation (base_environment.py _get_observation ->
                                 observation_processor.py:374-399), unrounded */
    uint16_t *d_work;         /* [N]    u16: depenetration iterations this env ran in this step (collide_vs_tiles,
                                 ninja.py:303-364) -- a profiling aid: the launch lasts as long as its busiest env */
} npp_step_out;

/* Simulator()+NPlayHeadless() for n_envs environments on GPU device_id. */
int npp_create(int n_envs, int device_id, unsigned flags, npp_handle *out);
int npp_destroy(npp_handle h);
const char *npp_last_error(npp_handle h);

/* Use an existing hipStream_t (e.g. torch's current stream) for all launches of h. NULL = default stream. */
int npp_set_stream(npp_handle h, void *hip_stream);
int npp_sync(npp_handle h);

/* NPlayHeadless.load_map_from_map_data (nplay_headless.py:195) -> Simulator.load (nsim.py:51) for a SET of
 * levels.  blob holds the raw map_data values of all levels back to back as doubles (generated levels carry
 * fractional entity coordinates); level i is blob[offsets[i] .. offsets[i+1]).
 * The host compiles every level (tiles -> ordered per-cell segment lists, entities -> per-cell tables) and
 * uploads the tables.  Replaces any previously loaded set and resets every env to level 0. */
int npp_load_levels(npp_handle h, const double *blob, const int64_t *offsets, int n_levels);

/* Which level each env plays (EnvMapLoader.load_map choice, env_map_loader.py:111-208).  env_ids == NULL
 * means envs 0..n-1.  The listed envs are reset (Simulator.reset, nsim.py:62). */
int npp_assign_levels(npp_handle h, const int32_t *env_ids, const int32_t *level_ids, int n);

/* Reset the envs whose mask byte is non-zero (NULL = all).  Without NPP_FLAG_FAST_RESET: Simulator.reset (nsim.py:62-76).
 * With it: Simulator.reset for an env's first reset after npp_load_levels / npp_assign_levels, Simulator.fast_reset
 * (nsim.py:78-140) afterwards -- the choice NppEnvironment.reset makes (npp_environment.py:541-557). */
int npp_reset(npp_handle h, const uint8_t *env_mask);
/* The same with an explicit choice: mode 0 = as npp_reset, 1 = Simulator.reset, 2 = Simulator.fast_reset
 * (NPlayHeadless.reset / fast_reset, nplay_headless.py). */
int npp_reset_ex(npp_handle h, const uint8_t *env_mask, int mode);

/* Truncation limit in frames (truncation_checker.py:21-29); limits == NULL sets `all` for every env. */
int npp_set_truncation_limit(npp_handle h, const int32_t *limits, int32_t all);
/* The reference env's DYNAMIC limit (npp_environment.py:1238-1256, base_environment.py:1078-1100 ->
 * truncation_calculator.py:19-57): per level int(clip(sqrt(reachable surface area) * 20 * 25, 1200, 10000)), the surface area
 * being the node count the reachability graph's flood fill finds from the spawn (npp_reach.cpp, pinned by the reference's own
 * values in tests/golden/reach.npz).  enable != 0: every env takes its level's limit now and again at every npp_load_levels /
 * npp_assign_levels (for the envs assigned); it drives both the truncation flag and game_state[40] (time_remaining).  A later
 * npp_set_truncation_limit overrides it until the next assignment.  Known deviation: the reference holds the 10 000-frame
 * fallback until its first reward calculation after a level load, i.e. for the first step's observation. */
int npp_set_dynamic_truncation(npp_handle h, int enable);
/* Host-only: that limit and the surface area for one level. */
int npp_level_truncation_limit(const double *map, int64_t n, int32_t *limit, int32_t *surface_area);

/* NppEnvironment.step for all envs (base_environment.py:483-755): d_actions[N] in 0..5
 * (_actions_to_execute, :366-402), up to frame_skip ticks with early stop on win/death (:535-609),
 * truncation check (:613), observation (:627,680).
 * d_reward: the sparse terminal constants only (+20 win, -3 death, +10 exit switch) -- reward parity, sparse mode: none; pbrs mode:
 * section 20 of DESIGN.md (npp_set_reward_mode / npp_step_reward below: the reference's PBRS calculator,
 * reward_calculation/main_reward_calculator.py:225, from a launch of its own behind this one, which overwrites d_reward). */
int npp_step(npp_handle h, const uint8_t *d_actions, int frame_skip, const npp_step_out *out);

/* Several Gymnasium steps in ONE launch, for action sequences that do not depend on the observations in between: batched
 * checkpoint replay (the reference's ActionReplayer.replay_to_checkpoint, action_replayer.py, replays one env at a time),
 * rollouts of a fixed plan.  d_actions: u8[n_steps][n_envs].  d_flags / d_reward / d_frames of `out` receive
 * [n_steps][n_envs] values (one row per step); the observations are those after the last step; with auto-reset an env that
 * terminates mid-sequence restarts on the spot (no terminal observation in this mode).  Wavefronts advance through their
 * steps independently, so the launch costs the sum of average step times instead of the sum of worst-case step times. */
int npp_step_many(npp_handle h, const uint8_t *d_actions, int n_steps, int frame_skip, const npp_step_out *out);

/* NPlayHeadless.tick(h, j) (nplay_headless.py:322) for all envs, n_ticks times, driven by replay input
 * bytes d_inputs[n_ticks][N] (bit0 jump, bit1 right, bit2 left: replay/replay_executor.py:61-84).
 * No early stop, no truncation, no auto-reset: the caller polls state like tools/test_replay_playback.py. */
int npp_tick(npp_handle h, const uint8_t *d_inputs, int n_ticks);

/* Observation of the current state without stepping (NppEnvironment._get_observation, used by reset()). */
int npp_observe(npp_handle h, const npp_step_out *out);

/* player_frame (84x84 u8) around each ninja, rasterised on device (nsim_renderer.py:71-134 +
 * observation_processor.py:207-282 crop incl. its axis swap).  d_out is [N,84,84]. */
int npp_render_player_frame(npp_handle h, uint8_t *d_out);
/* Goal-curriculum repositioning (gym_environment/reward_calculation/intermediate_goal_manager.py:698 apply_to_simulator): move
 * the exit switch (kind 0) or the exit door (kind 1) of ONE env to pixel position (x, y).  Like there, the entity's grid
 * cell follows (a switch that changes cell is appended to the new cell's list; the door joins its new cell's list when its
 * switch is hit) and the position survives resets until it is set again; NaN clears it.  Call between episodes.  Envs with
 * a moved entity run in the zoo kernels (merged neighbourhood walk). */
int npp_set_entity_pos(npp_handle h, int env, int kind, double x, double y);

/* switch_states observation (gym_environment/npp_environment.py:1782-1847): f32[n_envs][25] = up to 5 locked doors x
 * [switch x / 1056, switch y / 600, door x / 1056, door y / 600, collected]; the reference's door position falls back to the
 * switch position (its segment has no `p1`), reproduced.  Pinned by the reference's own two methods run on live entities
 * (tests/golden/obs.npz, make_golden_obs.py). */
int npp_switch_states(npp_handle h, float *d_out);

/* reachability_features (f32[n_envs][38]) and mine_sdf_features (f32[n_envs][3]) of the current state of every env: what
 * ReachabilityMixin._get_reachability_features (gym_environment/mixins/reachability_mixin.py:72-222) and
 * MineSignedDistanceField.get_features_at_position (graph/reachability/mine_proximity_cache.py:476) return, including the
 * reference's cache rule -- the 38 floats are recomputed only when (ninja cell, exit_switch_activated) differs from the key of
 * the env's previous call, so call it once per observation (after npp_step / npp_reset), as the reference does.  The
 * per-level tables (sub-node graph, entity mask, flood fill, geometric Dijkstra from both goals, mine SDF) are built on the
 * host at the first call.  Levels whose exit door lies 12-24 px from its switch send every exit-door query of the reference through
 * its cache-miss branch (physics A*, path_distance_calculator.py:744-845, 1218-1485): restated since round 3 -- per-level A* table
 * on the host, the calculator's per-episode (start cell, goal cell) dictionary per env on the device (13 KB per env, allocated only
 * when such a level is loaded; emptied when the env's episode counter moves, on npp_restore and on npp_assign_levels).
 * Either output may be NULL.  d_status (i32[n_envs], may be NULL): bit 0 set where the reference would have taken that branch
 * for a query the tables do not cover (no node with a cached distance under the ninja on a level without the A* table) -- those
 * rows carry the "unreachable" values.  NPP_ERR_UNSUPPORTED: a loaded level has several exit switches (the reference then also
 * leaves the level cache for the switch and runs a second search that is not restated), or an entity was moved with
 * npp_set_entity_pos.  Not meaningful between the steps of npp_step_many (the cache rule needs every observation).
 * mine_sdf_features: the VALUES are the reference's (MineSignedDistanceField); WHEN the reference's observation holds them (its
 * reward calculator builds / clears that SDF) is not modelled -- parity of that life cycle is unpinned. */
int npp_reachability(npp_handle h, float *d_features, float *d_mine_sdf, int32_t *d_status);
/* ... and, when d_switch_states (f32[n_envs][25]) is not NULL, npp_switch_states's output from the same launch (an idle lane of
 * every env's lane group writes it: the full observation Dict needs one kernel less). */
int npp_reachability_ex(npp_handle h, float *d_features, float *d_mine_sdf, int32_t *d_status, float *d_switch_states);

/* The reference's MINIMAL observation mode (gym_environment/config.py:17-20 `observation_mode`; space npp_environment.py:211-231,
 * content :2232-2270): minimal_observation f32[n_envs][40] = compute_minimal_observation (observation_processor.py:505-567):
 *    0-11  xspeed / MAX_HOR_SPEED, yspeed / MAX_HOR_SPEED, one-hot of min(state, 4), airborn and walled as +-1, wall_normal if
 *          walled else 0, floor_normalized_x / y
 *   12-19  reachability_features[13:15], [15:17], [8:10], [12], [24]
 *   20-35  the first 4 of the 8 nearest mines of spatial_context[64:], features 0, 1, 2, 5 of each 6
 *   36-39  jump_buffer / 5, floor_buffer / 5, wall_buffer / 5, launch_pad_buffer / 4, or -1 where the buffer is negative
 * every quotient in f64 and rounded once to f32, as the reference's assignment into its float32 array does.
 * npp_set_minimal_observation(h, enable): the mode's switch (off by default).  The mine columns are the step kernel's
 *   spatial_context rows, so while the mode is on every npp_step / npp_step_many / npp_observe writes them: into the caller's
 *   d_spatial_context, or, when the npp_step_out has none, into a buffer of the handle (448 bytes per env, allocated by the first such
 *   launch, freed by npp_destroy).  Nothing else changes; with the mode off nothing new runs.  The handle remembers WHERE the last
 *   such launch wrote the rows and npp_minimal_observation reads there: a caller's d_spatial_context must stay allocated until the
 *   next of these launches; a caller that frees or replaces the buffer first calls npp_set_minimal_observation(h, 1) again, which
 *   makes the handle forget the pointer (npp_minimal_observation is then NPP_ERR_STATE until the next launch).
 * npp_minimal_observation(h, d_out, d_status): the rows of the current state, from npp_reachability's launch -- it IS the
 *   observation's reachability call (same cache rule, same tables, same d_status), it additionally assembles the 40 floats, and it
 *   writes neither reachability_features nor mine_sdf_features.  Call it after the npp_step / npp_observe of the observation
 *   (NPP_ERR_STATE when there was none since the mode was switched on).  A call of npp_reachability[_ex] for the same observation,
 *   before or after, finds the key unchanged and both give the bits either gives alone.  The rows are a function of saved state
 *   only: npp_snapshot / npp_restore, resets, the level pool and the observation overlap (one launch per part) need nothing new.
 *   Refused like npp_reachability: NPP_ERR_UNSUPPORTED for levels with several exit switches and while an entity is repositioned with
 *   npp_set_entity_pos.  There is no terminal minimal observation (the reference defines none). */
int npp_set_minimal_observation(npp_handle h, int enable);
/* Host-only: the state encodings the device kernel runs (npp_minimal.hpp compiles for both) -- columns 0-11 and 36-39 of `count` rows
 * out f32[count][40] (the other columns are left alone) from state_a u32[count] (state word A; its bit layout: DESIGN.md section 3,
 * "packed state layout") and planes f64[count][4] = xspeed, yspeed, floor_normalized_x, floor_normalized_y. */
int npp_minimal_encode_host(const uint32_t *state_a, const double *planes, int count, float *out);
int npp_minimal_observation(npp_handle h, float *d_out /* [N,40] */, int32_t *d_status /* [N] or NULL */);

/* Path-direction action masking: the mask the reference's ENV returns.  Its observation does not carry
 * Ninja.get_valid_action_mask() as it stands: _get_action_mask_with_path_update (gym_environment/base_environment.py:3050,
 * 3075-3107) first runs _detect_straight_path_direction (:3109-3253) -- the ninja's graph node, the level cache's multi-hop
 * direction to the current goal (the exit switch, the exit door once the switch is activated), classified as left / right / down /
 * none -- and in masking mode "hard" (the default, nsim.py:48; the annealing schedule hard -> soft -> none of
 * reward_config.py:815-865) the last stage of get_valid_action_mask (ninja.py:743-800) removes what a straight path makes pointless:
 * left keeps NOOP and LEFT, right keeps NOOP and RIGHT, down removes the three jump actions.  d_action_mask of npp_step_out is that
 * function with the stage inert; these entry points add the stage, from the reachability tables of npp_reachability (built at the
 * first call, the graph of the spawn: graph updates inside an episode are not modelled) and the exact fp64 position, in a launch of
 * its own behind the step / observe / reset launch that produced the observation.  The rule is one function, npp_pathmask.hpp,
 * compiled for the device and for npp_path_direction_host.  Off by default: nothing is allocated or launched, every output is as
 * before.
 * npp_set_action_masking(h, mode): 0 off, 1 hard, 2 soft; may change between any two steps.  The first non-zero mode allocates the
 *   counters (17 bytes per env); mode 0 frees nothing and launches nothing.  < 0 or > 2: NPP_ERR_INVALID.
 * npp_path_action_mask(h, d_action_mask, d_direction, d_status): the launch, on the handle's stream, after joining an observation
 *   overlap.  Call it once per observation, after the npp_step / npp_observe / npp_reset that produced it.  d_direction (i8[n_envs],
 *   may be NULL): 0 none, 1 left, 2 right, 3 down.  Hard mode: the six bytes of every env in d_action_mask (i8[n_envs][6], the
 *   step's output) are filtered in place (NULL: NPP_ERR_INVALID); soft mode: d_action_mask is not touched (may be NULL) -- the
 *   direction is what a trainer's logit bias needs.  d_status (i32[n_envs], may be NULL): 1 where the direction was classified from
 *   the graph (the reference's `_deterministic_mask_applied_count += 1`), 0 where it is none or the near-goal line-of-sight hint.
 *   NPP_ERR_STATE in mode 0 and without levels; NULL handle: NPP_ERR_INVALID; NPP_ERR_UNSUPPORTED exactly where npp_reachability is
 *   (several exit switches; an entity repositioned with npp_set_entity_pos) -- the mask is then left unfiltered.
 * Counters, per env (the project's own definition; the reference also counts its terminal observation, which an auto-resetting
 *   device env never sees: parity of the two info numbers is unpinned): `observed` = calls of npp_path_action_mask since the env's last
 *   reset, `applied` = those with d_status 1.  When the npp_step before the call ended the env's episode and auto-reset it (its flags
 *   byte; without NPP_FLAG_AUTORESET never), both are latched into last_observed / last_applied and restart at this observation;
 *   npp_reset restarts the live ones, and so does switching the mode from 0 to 1 or 2 (observations went by uncounted).  They count
 *   CALLS: a second call for the same state (a caller that observes again between two steps, as NppVecEnvironment.restart does
 *   for the envs it leaves alone) counts again.  The handle remembers the flags row of the last npp_step: a caller's d_flags must stay allocated
 *   until this call (with d_flags NULL a row of the handle's is used).  After npp_step_many nothing is latched.  The counters are NOT
 *   part of archive / snapshot records: a restore leaves them as they are.
 * npp_path_mask_stats_view: device views u32[n_envs] of the four (any pointer may be NULL), valid until npp_destroy;
 *   NPP_ERR_STATE before the first non-zero mode. */
int npp_set_action_masking(npp_handle h, int mode);
int npp_path_action_mask(npp_handle h, int8_t *d_action_mask /* [N,6] in/out or NULL */, int8_t *d_direction /* [N] or NULL */,
                         int32_t *d_status /* [N] or NULL */);
int npp_path_mask_stats_view(npp_handle h, const uint32_t **d_observed, const uint32_t **d_applied, const uint32_t **d_last_observed,
                             const uint32_t **d_last_applied);
/* Host-only: the detector the device kernel runs (npp_pathmask.hpp compiles for both; base_environment.py:3109-3253 with
 * find_ninja_node, pathfinding_utils.py:1331-1496, and get_multi_hop_direction, path_distance_cache.py:162-185) on `count` positions
 * (f64[count][2]) of one level with switch_activated u8[count].  direction_out i8[count]: 0 none, 1 left, 2 right, 3 down;
 * from_graph_out u8[count] (may be NULL): npp_path_action_mask's d_status; status (one i32, may be NULL): bit 1 = level unsupported
 * (npp_reachability refuses it). */
int npp_path_direction_host(const double *map, int64_t n, const double *pos, const uint8_t *switch_activated, int count,
                            int8_t *direction_out, uint8_t *from_graph_out, int32_t *status);

/* Reward mode "pbrs": the step reward of the reference's RewardCalculator.calculate_reward
 * (gym_environment/reward_calculation/main_reward_calculator.py:225-904) as base_environment.step calls it (:644-657) with
 * RewardConfig(enable_path_waypoints=False), no goal curriculum, no momentum waypoints and a calculator reset() at every episode
 * start: terminal rewards (death with the switch milestone credited, win with the path-efficiency bonus), switch milestone, time
 * penalty x frames, distance milestones, gamma * Phi(s') - Phi(s) on the reference's potential WITH its position cache, the
 * completion-approach bonus, all times 0.1.  The rule is one function, npp_reward.hpp, compiled for the device (npp_reward.hip) and
 * for npp_reward_host; DESIGN.md 20 has the rule, the reference's quirks it reproduces, the per-env state and what the fixture
 * (tests/golden/reward.npz) pins.  The sequential path waypoints of a fresh RewardConfig() are an option of the mode
 * (npp_set_reward_waypoints below).  Out of scope: the goal curriculum, demo-waypoint merging, the bonuses calculate_reward has
 * disabled (turn approach, exit direction, velocity alignment, momentum waypoints), RewardConfig's schedules (its properties
 * as functions of the success rate: set the numbers with npp_set_reward_params), the TensorBoard diagnostics.  Known deviation: a step
 * that ends by TRUNCATION under NPP_FLAG_AUTORESET gets time penalty + switch milestone only (the reference evaluates the final
 * position, which the in-kernel reset has overwritten).
 * Off by default: nothing is allocated or launched, and d_reward of npp_step keeps its sparse constants bit for bit.
 * npp_set_reward_mode(h, mode, params): 0 sparse, 1 pbrs (params NULL = the defaults); other values: NPP_ERR_INVALID.  Switching on
 *   needs levels loaded (NPP_ERR_STATE), builds the tables of npp_reachability and each level's constants, allocates the per-env state
 *   (132 bytes per env, + 13 KB per env when a level takes the reference's miss branch) and restarts the reward state of every env
 *   on its current state.  NPP_ERR_UNSUPPORTED where npp_reachability refuses a level, and where the reference itself raises
 *   ("Combined geometric path distance is infinite") or would leave the restated paths; the mode then stays off.  npp_load_levels
 *   switches the mode off.
 * npp_set_reward_params(h, params): new numbers from the next npp_step_reward on (NULL: the defaults).
 * npp_step_reward(h, d_reward, d_components, d_status): the launch, on the handle's stream, after joining an observation overlap.  Call
 *   it once per npp_step, after it (NPP_ERR_STATE otherwise, in mode 0, and while an entity is repositioned with npp_set_entity_pos it
 *   is NPP_ERR_UNSUPPORTED).  d_reward f32[n_envs]: the fp64 reward rounded once.  d_components (f32[n_envs][6], may be NULL), unscaled:
 *   pbrs, distance milestone, switch milestone, approach bonus, terminal reward, potential.  d_status (i32[n_envs], may be NULL): which
 *   branch evaluated the potential: 0 full evaluation, 1 position-cache hit, 2 hit without next hop, 3 none (terminal step).  The
 *   handle remembers the flags and frames rows of the last npp_step (a caller's d_flags / d_frames must stay allocated until this call;
 *   rows of the handle's are used where the caller passed none).
 * Episode starts: the in-kernel auto-reset (from the step's flags byte), npp_reset, npp_assign_levels, the level pool's draw,
 *   npp_restore / npp_archive_restore and the test aids npp_set_ninja_state / npp_set_mover_state restart the reward state of the envs
 *   they touch ON THE STATE THEY LEAVE: calculator state emptied, cache key dropped, that state observed as the next step's prev_obs.
 *   Archive / snapshot records do NOT carry reward state.  npp_step_many is NPP_ERR_STATE while the mode is on: its inner steps have no
 *   observation.
 * The per-episode dictionary of the path calculator (levels whose exit door lies 12-24 px from its switch) is the handle's one, shared
 *   with npp_reachability: an entry is written once per (episode, cell), from the position of the first query, so the two launches
 *   agree whichever runs first PROVIDED both run at every observation when both are in use (NppVecEnvironment does). */
typedef struct NppRewardParams {
    double death_penalty, level_completion_reward, switch_activation_reward, time_penalty_per_step, pbrs_objective_weight, pbrs_gamma;
} NppRewardParams;
/* what a fresh RewardConfig() and PBRS_GAMMA give (recorded in tests/golden/reward.npz): -80, 200, 100, 0, 40, 0.99 */
void npp_reward_default_params(NppRewardParams *out);
int npp_set_reward_mode(npp_handle h, int mode, const NppRewardParams *params);
int npp_set_reward_params(npp_handle h, const NppRewardParams *params);
int npp_step_reward(npp_handle h, float *d_reward /* [N] */, float *d_components /* [N,6] or NULL */, int32_t *d_status /* [N] or NULL */);
/* Host-only: PBRSCalculator._compute_combined_path_distance (pbrs_potentials.py:897-1178) for one level: out[3] = spawn -> switch,
 * switch -> exit, their sum (pixels along the physics-optimal path on the base graph).  NPP_ERR_UNSUPPORTED (status 2, out = +inf where
 * the reference raises) for a level the mode refuses. */
int npp_reward_level_constants_host(const double *map, int64_t n, double *out, int32_t *status);
/* Host-only: the rollout twin of npp_step_reward on one level.  pos0: the position after the first reset; per step k pos[k] (the state the
 * env is in after the step: the reset state when flags[k] & end_bits), flags[k] (NPP_F_* of the state the step ended in), frames[k].
 * reward_out f64[count]; components_out f64[count][6] and kind_out u8[count] (d_status) may be NULL. */
int npp_reward_host(const double *map, int64_t n, const NppRewardParams *params, const double *pos0, const double *pos, const uint8_t *flags,
                    const uint16_t *frames, int count, int end_bits, double *reward_out, double *components_out, uint8_t *kind_out,
                    int32_t *status);

/* Reward mode "pbrs", sequential path waypoints: the bonus calculate_reward adds on every live step under a fresh RewardConfig()
 * (enable_path_waypoints=True, reward_config.py:48): `_calculate_sequential_waypoint_bonus` (main_reward_calculator.py:2313-2484) with
 * `get_waypoint_bonus` (reward_config.py:309-399), on the waypoints `extract_path_waypoints_for_level` (:1221-1398) places every
 * progress_spacing pixels along the two optimal paths of `_compute_original_paths` (spawn -> switch, switch -> exit; find_shortest_path
 * on the physics cost).  The rule is npp_waypoint.hpp, compiled for the device (npp_waypoint.hip, npp_waypoint_kernel, launched by
 * npp_step_reward in front of npp_reward_kernel) and for npp_reward_host_wp; DESIGN.md 23 has the table layout, the per-env state, the
 * reference's quirks and what tests/golden/waypoints.npz pins.  The farming penalty of the death branch is always 0 in the reference
 * (it reads a key its observation never has) and is not computed.  Off by default: nothing is allocated or launched.
 * npp_set_reward_waypoints(h, on, params): NPP_ERR_STATE unless reward mode 1 is on.  Switching on builds and uploads every loaded
 *   level's table (params NULL = the defaults; progress_spacing takes effect here only), allocates the per-env state (72 bytes per env:
 *   a 512-bit collected set, the next-expected index, the collected count) and restarts it.  NPP_ERR_UNSUPPORTED, naming the level, for
 *   more than 512 waypoints on a level and while an entity is repositioned with npp_set_entity_pos; NPP_ERR_INVALID for a non-finite
 *   number, a negative radius or one above 24 (the kernel walks the 3 x 3 cells of 24 px around the ninja), a spacing <= 0.  A level
 *   without waypoints is accepted: its bonus is always 0.  npp_load_levels and npp_set_reward_mode(h, 0, ...) switch it off.
 * npp_set_waypoint_params(h, params): radius and the two scales from the next launch on (NULL: the defaults; progress_spacing is ignored).
 * npp_step_reward_wp: npp_step_reward plus d_wp_bonus (f32[n_envs], the UNSCALED bonus of the step) and d_wp_info (i32[n_envs][3]: the
 *   collected sequence index or -1, the next expected index and the collected count after the step -- before the restart on a step that
 *   ended the episode).  Either may be NULL; both are left unwritten with waypoints off.  npp_step_reward is this call with both NULL.
 * Every episode start that restarts the reward state (above) restarts the waypoint state too; archive / snapshot records carry none.
 * npp_reward_waypoints(h, level, out_xy, out_phase, cap, count): host copy of a level's table in sequence order (world pixels; phase 0
 *   pre-switch, 1 post-switch); *count is the table's size, at most `cap` entries are written. */
typedef struct NppWaypointParams {
    double collection_radius, out_of_order_scale, progress_scale, progress_spacing;
} NppWaypointParams;
/* what a fresh RewardConfig() gives (recorded in tests/golden/waypoints.npz): 18, 0.3, 2.0, 12 */
void npp_waypoint_default_params(NppWaypointParams *out);
int npp_set_reward_waypoints(npp_handle h, int on, const NppWaypointParams *params);
int npp_set_waypoint_params(npp_handle h, const NppWaypointParams *params);
int npp_step_reward_wp(npp_handle h, float *d_reward /* [N] */, float *d_components /* [N,6] or NULL */, int32_t *d_status /* [N] or NULL */,
                       float *d_wp_bonus /* [N] or NULL */, int32_t *d_wp_info /* [N,3] or NULL */);
int npp_reward_waypoints(npp_handle h, int level, double *out_xy /* [cap][2] */, uint8_t *out_phase /* [cap] */, int cap, int32_t *count);
/* Host-only: one level's waypoint table (out_xy f64[cap][2], out_phase u8[cap], out_node_index i32[cap], *count its size), the two node
 * paths (path0 / path1 i32[path_cap][2] in tile-data pixels, path_len i32[2]) and the spawn, switch and exit node (nodes i32[3][2], -1 =
 * none).  Any output but count may be NULL.  NPP_ERR_UNSUPPORTED (status 2) for a level reward mode "pbrs" or the waypoints refuse. */
int npp_reward_waypoints_host(const double *map, int64_t n, double progress_spacing, int cap, double *out_xy, uint8_t *out_phase,
                              int32_t *out_node_index, int32_t *count, int path_cap, int32_t *path0, int32_t *path1, int32_t *path_len,
                              int32_t *nodes, int32_t *status);
/* Host-only: get_waypoint_bonus(index, total, in_sequence) under the two scales */
int npp_waypoint_bonus_host(int index, int total, int in_sequence, double progress_scale, double out_of_order_scale, double *out);
/* Host-only: npp_reward_host with the waypoints: wp NULL = off (then exactly npp_reward_host), else the numbers.  wp_bonus_out
 * f64[count] and wp_info_out i32[count][3] (as d_wp_bonus / d_wp_info, the bonus in fp64) may be NULL. */
int npp_reward_host_wp(const double *map, int64_t n, const NppRewardParams *params, const NppWaypointParams *wp, const double *pos0,
                       const double *pos, const uint8_t *flags, const uint16_t *frames, int count, int end_bits, double *reward_out,
                       double *components_out, uint8_t *kind_out, int32_t *status, double *wp_bonus_out, int32_t *wp_info_out);

/* The whole gray frame of envs [env0, env0 + count): what NPlayHeadless.render() returns in grayscale mode
 * (nplay_headless.py:144-156, nsim_renderer.py:71-134).  d_out: u8[count][600][1056]. */
int npp_render_frame(npp_handle h, int env0, int count, uint8_t *d_out);

/* global_view (observation_processor.py:304-328): the (600 x 1056) gray frame through cv2.resize(frame, (100, 176), INTER_AREA).
 * The reference's RENDERED_VIEW_WIDTH / HEIGHT are swapped (gym_environment/constants.py:18-19), so the frame is squashed to
 * 176 rows x 100 columns; reproduced as is (area-weighted mean of the source pixels).  d_out: u8[n_envs][176][100]. */
int npp_render_global_view(npp_handle h, uint8_t *d_out);

/* Parity hook: copies the simulator state of envs [env0, env0+count) to HOST buffers.
 * f64 [count][NPP_DUMP_F64]: xpos ypos xspeed yspeed floor_nx floor_ny ceil_nx ceil_ny xspeed_old yspeed_old
 *                            applied_gravity applied_drag
 * i32 [count][NPP_DUMP_I32]: see DESIGN.md ("state dump layout"). */
int npp_dump_state(npp_handle h, int env0, int count, double *f64_out, int32_t *i32_out);
/* Parity hook, a TEST AID: overwrites xpos, ypos, xspeed, yspeed of envs [env0, env0+count) from the HOST buffer
 * xyv f64 [count][4] and nothing else (every other plane and word of the env's state keeps its value).  Joins an open observation
 * overlap and synchronises, as the dump does.  NPP_ERR_INVALID for a non-finite value: then no env is touched.  After it an env's
 * action route and its archive meta rows no longer describe its state (tests/inject_states.py, DESIGN.md "injected states"). */
int npp_set_ninja_state(npp_handle h, int env0, int count, const double *xyv /* [count][4] x y vx vy */);
/* Parity hook, a TEST AID: for envs [env0, env0+count) and mover slot `slot` (the level's movers -- drones, bounce blocks, thwumps,
 * death balls, shove thwumps -- in entity_dic order) overwrites the record's four doubles from the HOST buffer xyab f64 [count][4]:
 * x, y and the speed of a bounce block / death ball or the target of a drone (thwumps and shove thwumps have neither: 0, 0).
 * field (i32 [count], or NULL to leave it alone) is the reference's own value of the 2-bit field: a thwump's state -1 / 0 / 1, a
 * drone's dir 0..3.  The record's cell and list-order number keep their values, like Entity.cell and the grid lists after an
 * attribute assignment in the reference: the next grid_move updates them.  NPP_ERR_INVALID for a non-finite value, a slot past
 * the movers of an env's level, a field the mover's kind does not have, or a non-zero third / fourth value for a thwump: then
 * nothing is written.  Joins and synchronises, as the dump does (tests/inject_zoo_states.py). */
int npp_set_mover_state(npp_handle h, int env0, int count, int slot, const double *xyab /* [count][4] */, const int32_t *field);
/* Parity hook, a TEST AID: one env's movers in slot order as rows of 5 doubles on the HOST: x, y, a, b and the field as above (a shove
 * thwump's state 0..3; 0 for bounce blocks and death balls).  Returns the count via *n_out. */
int npp_dump_movers(npp_handle h, int env, double *out /* [max_rows][5] */, int max_rows, int *n_out);
/* Host-only: npp_dump_state's own decode of one env's five packed state words (planes A..E, DESIGN.md "packed state layout") into
 * its i32 row.  Columns 13 and 27 are not in the words: 2 (no exit switch) and level 0. */
int npp_state_decode_host(const uint32_t words[5], int32_t *out /* NPP_DUMP_I32 */);

/* Parity hook: per-entity dynamic state of one env in level (map) order, movers left out (npp_dump_movers has them):
 * mines -> state 0/1/2, exit door -> switch_hit, regular door -> active + 2 * closed, boost pad -> active + 2 * touching,
 * others -> active.  Returns count via *n_out. */
int npp_dump_entities(npp_handle h, int env, int32_t *out, int max, int *n_out);

/* Parity hook: the compiled collision table of a level as rows of 8 int16
 * (cell x, cell y, kind, then x1,y1,x2,y2,oriented | cx,cy,hor,ver,convex), in query order. */
int npp_dump_level_segments(npp_handle h, int level, int16_t *out, int max_rows, int *n_out);

/* Host-only utilities (no GPU, no handle): run the level compiler on one level.  Used by the CPU test-suite to
 * check the compiler against the reference's ordered segment dump and entity tables.
 * segments: rows of 8 int16 as in npp_dump_level_segments.  entities: rows of 6 doubles in map order:
 * kind (1 mine, 2 gold, 3 exit door, 4 exit switch, 6 locked-door switch), x, y, cell x, cell y, initial 2-bit state. */
int npp_compile_level_segments(const double *map, int64_t n, int16_t *out, int max_rows, int *n_out,
                               uint32_t *unsupported_mask);
int npp_compile_level_entities(const double *map, int64_t n, double *out, int max_rows, int *n_out);

/* Build variant of the step kernel (a speed knob like npp_set_launch_geometry; results are bit-identical for every variant; no
 * counterpart in the reference).  The 16-lanes-per-env kernels of levels without moving entities exist in three builds -- 0: two
 * wavefronts per SIMD, two candidate slots per lane; 1: two wavefronts per SIMD, one slot (fastest on sparse geometry, slow where
 * creases gather more than 16 segments); 2: one wavefront per SIMD, two slots (fastest single chain) -- and npp_step times them
 * against each other on the handle's own workload (HIP events, no synchronisation) after every npp_load_levels /
 * npp_assign_levels and keeps the fastest.  variant = -1 (default) selects that autotuner, 0..2 pin a build.
 * npp_get_step_variant: *variant = the build npp_step currently launches, *tuned = 1 once the autotuner has decided (or a build is
 * pinned). */
int npp_set_step_variant(npp_handle h, int variant);
int npp_get_step_variant(npp_handle h, int *variant, int *tuned);

/* Observation overlap (a speed knob for the full observation Dict; results are bit-identical with it on or off; no counterpart in the
 * reference).  A step launch ends with a tail of a few long environments that leaves most of the chip idle.  With cuts c1 < c2 < ...
 * (percentages, at most three) npp_step cuts its heavy-first workgroup order at those points and launches every piece ("part") as a
 * kernel of its own, the most expensive first: the last piece (the cheap end) on the handle's stream, the others on HIP streams the
 * handle owns (chosen at set-up so that their kernels are seen to run beside the handle's stream: that call synchronises).  Until the next join npp_render_player_frame, npp_render_global_view, npp_reachability and npp_switch_states launch
 * one kernel per part, each behind the part it reads: the observations of the cheap environments are produced while the expensive
 * ones are still stepping.  npp_join makes the handle's stream wait for the others -- call it before anything else consumes the
 * step's or the observation kernels' outputs on the handle's stream; every other entry point (npp_sync, npp_step, npp_reset,
 * npp_snapshot ...) joins by itself.  npp_set_obs_overlap(h, percent) = one cut; percent = 0 / n_cuts = 0 (default) switch it off. */
int npp_set_obs_overlap(npp_handle h, int percent);
int npp_set_obs_overlap_parts(npp_handle h, const int *cuts, int n_cuts);
int npp_join(npp_handle h);

/* Host-only: the per-level reachability tables of one level, stage by stage (CPU tests compare them with the reference's,
 * tests/golden/reach.npz).  Node id = i * 46 + j for the sub-node at tile-data pixel (6 + 12 i, 6 + 12 j), 84 x 46 = 3864 ids.
 * info i32[16]: supported, len(adjacency), goal node of exit_switch_0 / exit_door_0 in the level cache, the two goal nodes
 * get_distance resolves, switch x, y, door x, y (int), goal id inferred for the door position (0 = "switch"), mines, has
 * SDF, surface area (nodes).  base_in / base_adj / phys: tile-only graph (node present, edge bits N E S W NE SE SW NW,
 * grounded | walled << 1).  in / adj: final adjacency.  dist f64[2][3864], hop i16[2][3864], mh f64[2][3864][2]: level
 * cache per goal.  sdf f32[50][88], grad f32[50][88][2].  scalars f64[8]: area scale, feature 0, feature 3, features 25-28.
 * Any pointer may be NULL. */
int npp_reach_compile(const double *map, int64_t n, int32_t *info, uint8_t *base_in, uint8_t *base_adj, uint8_t *phys, uint8_t *in,
                      uint8_t *adj, double *dist, int16_t *hop, double *mh, float *sdf, float *grad, double *scalars);
/* Host-only: the feature function the device kernel runs (npp_reach_features.hpp compiles for both), on `count` positions
 * (f64[count][2]) of one level; mines i32[count][2] = (total, deadly) toggle mines (NULL: all safe).  out f32[count][38],
 * sdf_out f32[count][3] (may be NULL), status i32[count] (may be NULL; bit 0 as in npp_reachability, bit 1 = level unsupported). */
int npp_reach_features_host(const double *map, int64_t n, const double *pos, const int32_t *mines, int count, float *out, float *sdf_out,
                            int32_t *status);
/* Host-only: the tables behind the cache-miss branch of CachedPathDistanceCalculator.get_distance
 * (graph/reachability/path_distance_calculator.py:1218-1485, physics A* :744-845), built for the exit door of levels whose door lies
 * within 24 px (but not 12) of its switch -- there the reference's goal-id inference sends EVERY exit-door query down that branch.
 * info i32[20]: miss branch active, number of goal nodes, switch and door share a 24-px cell, supported, then the goal node ids
 * (-1 padded).  cgoal u8[3864]: index of the goal node find_goal_node_closest_to_start picks for a temp start node (255 = node
 * not in the adjacency).  astar f64[16][3864]: _calculate_distance(start node, goal node) (NaN = pair not tabulated).
 * mine_mult f64[3864]: MineProximityCostCache multiplier per node (1 = none).  Any pointer may be NULL. */
int npp_reach_compile_miss(const double *map, int64_t n, int32_t *info, uint8_t *cgoal, double *astar, double *mine_mult);
/* Host-only: npp_reach_features_host along a ROLLOUT -- the `count` positions are consecutive feature recomputations of one env,
 * new_episode u8[count] marks the first recomputation after an episode reset (the path calculator's per-episode
 * (start cell, goal cell) dictionary is emptied there, reachability_mixin.py:67-70); what the device keeps per env.  raw_out f64[count]
 * (may be NULL): the dictionary's entry for the ninja's cell after each query (the raw A* cost; NaN = no entry). */
int npp_reach_rollout_host(const double *map, int64_t n, const double *pos, const int32_t *mines, const uint8_t *new_episode, int count,
                           float *out, int32_t *status, double *raw_out);

/* Host-only: the zoo tables the level compiler derives from map_data.  edges_out: int32[2][89*51] grid-edge counters at
 * load (horizontal then vertical, key = x * 51 + y; tile edges of tile_segment_factory.py:283-302 plus closed doors,
 * entity_door_base.py:78-89).  movers_out: rows of 4 doubles (Entity.type, x, y, creation order) in entity_dic order. */
int npp_compile_level_zoo(const double *map, int64_t n, int32_t *edges_out, double *movers_out, int max_movers, int *n_movers);

/* Test / debug aid for levels with moving entities: per env 6 doubles summed over the entities in the reference's
 * entity_dic order (keys ascending, creation order inside a key): sum x, sum y, sum xspeed, sum yspeed (bounce blocks and
 * death balls), sum of state codes (3*closed + 5*(state mod 7) + 11*dir + 13*touching + 17*activated), number of active
 * entities -- the row tests/golden/make_golden_zoo.py records from the reference after every tick. */
int npp_entity_checksum(npp_handle h, int env0, int count, double *out);

/* Go-Explore style checkpoints (state_checkpoint.py / action_replayer.py in the reference restore a state by
 * reset + replaying the action sequence and validating |dpos| < 0.01 px).  Here a checkpoint is a raw copy of the
 * state of ALL envs kept on the device (one slot per handle; inside, one record per env in the checkpoint archive's layout,
 * below, moved by the archive's kernel): npp_snapshot stores it, npp_restore puts it back for
 * the envs whose mask byte is non-zero (NULL = all).  The env -> level assignment must not have changed in between (draws of the
 * level pool are part of the state: the snapshot holds every env's level, draw count and truncation limit, and once a pool has been
 * on since npp_load_levels npp_restore puts them back together with the state). */
int npp_snapshot(npp_handle h);
int npp_restore(npp_handle h, const uint8_t *env_mask);

/* Checkpoint archive: restore any env from any slot.  The reference's Go-Explore checkpoints (state_checkpoint.py,
 * action_replayer.py, base_environment.py:1769-1789 _reset_to_checkpoint) are found by one worker and restarted from by any worker
 * on the same level, many times; npp_snapshot's single slot lets env e go back only to what env e itself was.  The archive holds
 * n_slots records of ONE env's state each -- everything npp_restore carries for an env: the double and word planes, the entity
 * words, the spatial-context cache row, the zoo block, the reachability key + cache row (or a "none" marker when the record was
 * stored before the first npp_reachability), the truncation limit, the level and the level pool's draw count (which only
 * npp_restore puts back) -- as one contiguous record whose size follows from the loaded level set (npp_archive_record_bytes).
 * npp_archive_create(h, n_slots): allocates it (empty); 0 frees it; < 0 is NPP_ERR_INVALID; needs levels loaded; a failed
 *   allocation is NPP_ERR_HIP and leaves the previous archive in place.  npp_load_levels drops the archive.
 * npp_archive_store / npp_archive_restore(h, d_envs, d_slots, count, d_status): d_envs / d_slots are DEVICE arrays i32[count],
 *   d_status a device array i32[count] or NULL.  Enqueued on the handle's stream after joining an observation overlap; no
 *   synchronisation and no host copy of the lists, so a training loop builds them on the same stream.  Entry i copies env
 *   d_envs[i] to slot d_slots[i] (store) or the slot to the env (restore); its status is decided on the device:
 *     0 done   1 skipped (env < 0 or slot < 0: padding of a fixed-length list)   2 level mismatch (restore: the slot's level is not
 *     the level the env plays; the env is not touched)   3 slot empty (restore)   4 env or slot out of range (nothing read or written)
 *   Every access stays in bounds whatever the lists hold.  The same env twice in one restore list, or the same slot twice in one
 *   store list, is a caller error (the result is a mixture of the two); one slot restored into many envs is the normal case.
 *   A restored env is in the reference's "reset + replay" condition exactly as after npp_restore: the per-episode reachability
 *   dictionary is emptied, the cached reachability vector is the slot's (or absent), and the env keeps the slot's frame count and
 *   truncation limit, so its truncation budget continues from the checkpoint (the reference's fresh budget after a replay,
 *   truncation_checker.py:53-58, is not modelled).
 *   NPP_ERR_STATE, with the cause in the message: no archive; the level pool is on; an entity is repositioned with
 *   npp_set_entity_pos -- once levels move on the device or an entity is moved the host cannot know what a record's tables belong
 *   to; for the same reason npp_set_level_pool and a repositioning npp_set_entity_pos are refused while an archive exists.
 *   npp_assign_levels keeps the archive: records carry their level and restore checks it on the device.
 * npp_archive_meta_view: device arrays f64[n_slots][4] = x, y, xspeed, yspeed and i32[n_slots][6] = stored (0 / 1), level, frame,
 *   cell_x, cell_y, switch_activated, written by the store kernel from the state it copies with npp_dump_state's decode (frame =
 *   i32 column 22, switch_activated = column 13 != 1); the cell is floor(x / 24), floor(y / 24), the reference's 24 px
 *   discretisation (state_checkpoint.py:26, replay/demo_checkpoint_seeder.py:284-287).  Valid while the archive lives, so a
 *   selection rule can run on them on the handle's stream. */
int npp_archive_create(npp_handle h, int n_slots);
int npp_archive_store(npp_handle h, const int32_t *d_envs, const int32_t *d_slots, int count, int32_t *d_status);
int npp_archive_restore(npp_handle h, const int32_t *d_envs, const int32_t *d_slots, int count, int32_t *d_status);
int npp_archive_meta_view(npp_handle h, const double **d_f64 /* [n_slots][4] */, const int32_t **d_i32 /* [n_slots][6] */);
int npp_archive_num_slots(npp_handle h);
int npp_archive_record_bytes(npp_handle h);   /* 0 without an archive */

/* Cell index over the checkpoint archive: Go-Explore's "best state per cell" and its count-weighted pick, decided on the device.
 * The reference ecosystem's rule (replay/demo_checkpoint_seeder.py): one checkpoint per cell (int(x // 24), int(y // 24)), cells
 * kept apart by switch_activated, the highest cumulative reward wins, strictly (:283-287, :427-435); no checkpoint nearer than
 * 72 px to the exit door once the switch is on (:30, :118-153); selection by visit count (:1-13).  The archive manager itself
 * lives in the trainer, so the bits below are this library's own definition (csrc/npp_cells.hpp).
 *   key       k = level * 2200 + (sw * 25 + cy) * 44 + cx, cx = (int)floor(x / 24.0), cy = (int)floor(y / 24.0), sw = the exit
 *             switch's state != 1 (npp_dump_state column 13 != 1): the meta row's own expressions.
 *   eligible  mask byte non-zero; ninja state (column 0) 0..5; 0 <= cx < 44, 0 <= cy < 25; the score is not NaN; and NOT (sw == 1,
 *             the level has an exit door, sqrt(dx * dx + dy * dy) < 72.0 with dx = x - door_x, dy = y - door_y) -- f64, no FMA.
 *   score     d_score[e], larger is better; NULL: -(float)frame (fewest frames to reach the cell).  Compared as ordered bits
 *             ob = b ^ ((b >> 31) ? 0xffffffff : 0x80000000): -0.0 below +0.0, the infinities ordinary values.
 *   winner    of a key in one explore call: the largest ob, ties to the lowest env; it replaces the incumbent only when strictly
 *             larger.  The winners of keys without a slot take slots n_used, n_used + 1, ... in ascending env order; one whose
 *             slot would be >= n_slots stays empty (status 7) and leaves only its visit count.
 *   counts    visits[k] += 1 per eligible env of every explore call (losers too); chosen[k] += 1 per env a select call sends to k.
 *   weight    w(k) = (uint32_t)floor(1048576.0 / sqrt((double)(visits[k] + chosen[k] + 1))) for a key that holds a slot, else 0;
 *             64-bit sums; the counts of before the select call.
 *   draw      env e in select call number c (0 after creation, +1 per call): u = mix(mix((e << 32) | c) ^ seed) with the level
 *             pool's splitmix64 round, T = the weight sum of the env's level, t = (u * T) >> 64; the first key of that level, in
 *             ascending order, whose inclusive prefix sum is > t; its slot.  T == 0: -1.
 * npp_archive_cells_create(h, enable, seed): enable != 0 needs an archive (NPP_ERR_STATE without); allocates the tables for the
 *   loaded level set, EMPTIES the archive (every slot's `stored` becomes 0) and owns all its slots from then on; a failed allocation
 *   is NPP_ERR_HIP and leaves the previous state in place.  enable == 0 frees the tables and leaves the records as they are.
 *   npp_archive_create (any argument) and npp_load_levels drop the index; npp_assign_levels keeps it.
 * npp_archive_explore(h, d_score, d_mask, d_status): d_score device f32[n] or NULL, d_mask device u8[n] or NULL (all envs), d_status
 *   device i32[n] or NULL.  Three launches on the handle's stream (propose, assign, the archive's store kernel) after joining an
 *   observation overlap; no synchronisation, no host copy.  Status: 0 stored (won a new or a better cell), 1 skipped (mask), 5 not
 *   eligible, 6 lost (the incumbent or another env of this call is at least as good), 7 archive full.
 * npp_archive_select(h, d_mask, d_slots): d_slots device i32[n] receives the drawn slot, -1 for a mask byte 0 or an env whose level
 *   holds no cell; feed it to npp_archive_restore.  Two launches (prefix sums per level, pick); all picks of one call see the
 *   same weights.
 * With an index, npp_archive_store is refused (NPP_ERR_STATE: the cell index owns the slots); npp_archive_restore, npp_snapshot
 *   and npp_restore work as before.  Explore and select are refused without an index and for the causes npp_archive_store names.
 * npp_archive_cells_view: device arrays cell_slot i32[K] (-1 = none), cell_score f32[K], visits / chosen u32[K], K = n_levels *
 *   2200 in key order; slot_key i32[n_slots] (-1 = unused); n_used i32[1].  Valid while the index lives.
 * npp_archive_cell_keys_host / npp_archive_cell_pick_host: the same rule without a GPU or a handle, for tests: the keys (-1 = not
 *   eligible by state, cell or exit filter) of `count` rows xy f64[count][2], state / switch_state i32[count] on `level` compiled
 *   from `map`; the slots that envs[i] draw from ONE level's 2200-entry tables in select call number `call`. */
int npp_archive_cells_create(npp_handle h, int enable, uint64_t seed);
int npp_archive_explore(npp_handle h, const float *d_score, const uint8_t *d_mask, int32_t *d_status);
int npp_archive_select(npp_handle h, const uint8_t *d_mask, int32_t *d_slots);
int npp_archive_cells_view(npp_handle h, const int32_t **d_cell_slot, const float **d_cell_score, const uint32_t **d_visits,
                           const uint32_t **d_chosen, const int32_t **d_slot_key, const int32_t **d_n_used);
int npp_archive_cell_keys_host(const double *map, int64_t n, int level, const double *xy, const int32_t *state, const int32_t *switch_state,
                               int count, int32_t *keys_out);
int npp_archive_cell_pick_host(const int32_t *cell_slot, const uint32_t *visits, const uint32_t *chosen, uint64_t seed, uint32_t call,
                               const int32_t *envs, int count, int32_t *slots_out);

/* Action routes: the list of actions that led every env from its spawn to where it is, kept on the device.  In the reference a
 * checkpoint IS its route: StateCheckpoint.action_sequence (state_checkpoint.py) is replayed from the spawn by ActionReplayer, and
 * the env keeps the running list -- base_environment.py:186 creates `_action_sequence`, :517 appends per step, :1677 clears at
 * reset, :2114 appends during a checkpoint replay; get_current_action_sequence() / get_action_sequence_length() serve it
 * (:2332-2349).  Off by default: nothing is allocated, nothing is launched, records keep their size.  The rule
 * (csrc/npp_route.hpp):
 *   buffers   u8[n_envs][2][cap], one action (0..5) per byte: the route being written and the route of the episode that ended last
 *   header    i32[n_envs][16]: words 0-5 the CURRENT route, 6-11 the FINISHED route, 12 which buffer holds the current one, 13-15 0
 *   a route   len | bits (1 = an action was dropped at len == cap, 2 = not replayable from this record) | frame_skip (0 while empty)
 *             | frames executed | flags byte of the last executed step | the level at the first append (-1 while empty);
 *             empty = len == 0 and bits == 0
 *   step row  (npp_step; npp_step_many: its n_steps rows in order) with x frames executed: x > 0 appends the action (an env that is
 *             terminal and not auto-reset executes 0 frames and appends nothing); then, with NPP_FLAG_AUTORESET and a flags byte with
 *             WON, DEAD or TRUNCATED, a FLIP: the current route becomes the finished one (no bytes move) and an empty one starts.
 *             A flip of an empty route changes nothing.  The append is a launch of its own behind the step (per part of a split
 *             step, on the part's stream); it reads the step's flags / frames rows -- rows of the handle when npp_step_out has none.
 *   resets    npp_reset / npp_reset_ex (masked envs), npp_assign_levels (listed envs), npp_draw_levels and the level pool's redraw
 *             (envs that changed level) flip; npp_load_levels empties both routes of every env; npp_tick sets bit 2 everywhere.
 *   records   while routes are on, every archive / snapshot record carries the env's current route (8 header words, then the
 *             bytes), and npp_archive_restore / npp_restore replace the env's CURRENT route with the record's (the finished route
 *             stays); npp_archive_record_bytes grows by 32 + cap.  Store and restore move the first len bytes rounded up to 16.
 * npp_set_routes(h, capacity): > 0 is rounded up to a multiple of 16 and allocates zeroed buffers and empty headers; 0 frees them;
 *   < 0 is NPP_ERR_INVALID.  NPP_ERR_STATE while a checkpoint archive exists (its records' layout depends on it: call it before
 *   npp_archive_create).  An existing snapshot is invalidated (npp_restore: NPP_ERR_STATE until the next npp_snapshot).  A failed
 *   allocation is NPP_ERR_HIP and leaves the previous state in place.
 * npp_route_view: device views of the buffers and headers, valid until the next npp_set_routes, rewritten in stream order.
 * npp_archive_route_view: slot s keeps its route header at d_records + s * stride_words + hdr_offset_words and its bytes 8 words
 *   later -- a selection rule can read route lengths (the reference's find_checkpoint_with_min_replay_cost) and an export can copy
 *   single routes without a kernel.  NPP_ERR_STATE without an archive or without routes.
 * npp_route_apply_host: the same rule without a GPU or a handle, for tests, on ONE env: hdr i32[16], actions u8[2][capacity]
 *   (capacity a multiple of 16), updated in place by `count` events of 8 words each: {0, action, flags, frames, frame_skip, level}
 *   a step row; {1} a reset; {2} raw ticks; {3, six header words, byte offset into restore_bytes} a restore from that route. */
int npp_set_routes(npp_handle h, int capacity);
int npp_route_view(npp_handle h, const uint8_t **d_actions, const int32_t **d_hdr, int *capacity);
int npp_archive_route_view(npp_handle h, const uint32_t **d_records, int64_t *hdr_offset_words, int64_t *stride_words);
int npp_route_apply_host(int32_t *hdr, uint8_t *actions, int capacity, int autoreset, const int32_t *events, int count,
                         const uint8_t *restore_bytes);

/* Episode statistics: what a trainer reads at every episode end, kept on the device.  The reference puts it into `info`
 * (base_environment.py:1163-1242): "r" = current_ep_reward (created at :156, += reward at :676, zeroed at npp_environment.py:587
 * and :688), "l" = sim.frame, "is_success" / "switch_activated" / "switch_activation_frame" (:546-552), "level_id",
 * "from_checkpoint", and episode_pbrs_metrics' pbrs_total and terminal_reward (main_reward_calculator.py:2825-2914).  Off by
 * default: nothing is allocated, nothing is launched.  The rule (csrc/npp_episode.hpp):
 *   record    per env NPP_EP_NI i32 words and NPP_EP_ND doubles, as planes i32[NPP_EP_NI][n_envs] / f64[NPP_EP_ND][n_envs]: the
 *             CURRENT episode (words NPP_EP_STEPS .. NPP_EP_BITS, doubles NPP_EP_RET, NPP_EP_COMP + 0..5), the FINISHED episode (the
 *             same at + NPP_EP_FIN / + NPP_EP_DFIN), the flags byte of its ending step (NPP_EP_FIN_FLAGS) and the u32 count of
 *             episodes the env finished (NPP_EP_N_FINISHED).  switch_step: the 1-based step at which NPP_F_SWITCH was first seen, 0 =
 *             never; switch_frames: the episode's frames after that step.  bits: 1 closed (ended without auto-reset), 2 begun by a
 *             restore, 4 npp_tick ran inside it.
 *   step row  flags f, frames x, reward r, optionally six components: nothing when x == 0 or the episode is closed; otherwise the
 *             episode takes the env's level if this is its first row, steps += 1, frames += x, ret += (double)r, comp[k] +=
 *             (double)c[k], the switch latch; and with WON, DEAD or TRUNCATED in f the episode is copied to FINISHED, n_finished += 1,
 *             its deltas go to the table, and the current episode restarts empty (NPP_FLAG_AUTORESET) or is closed (without: a
 *             truncated env keeps stepping and is not counted twice).
 *   table     u64[n_levels][16], columns NPP_EPC_*: episodes | won | dead | truncated | dead by mine | dead by impact | switch
 *             activated | steps | frames | frames of won episodes | return_fix = the two's-complement sum of
 *             floor(clamp(ret, +-2^42) * 2^20 + 0.5) | restored | abandoned | 0 0 0.  An episode begun by a restore adds 1 to `restored`
 *             and nothing else.  Integer atomics only: the table does not depend on the order in which envs end.
 *   events    RESET -- npp_reset / npp_reset_ex (masked envs), npp_assign_levels (listed envs), npp_draw_levels (envs that changed
 *             level): a current episode with steps that is neither closed nor begun by a restore adds 1 to `abandoned` of its
 *             level, then the current episode is empty on the env's level.  RESTORE -- npp_restore (masked envs),
 *             npp_archive_restore (entries of status 0): the same, and the new episode carries bit 2.  npp_tick sets bit 4.
 *             npp_demo_play and npp_archive_seed empty every current episode without counting.  FINISHED and n_finished stay.
 *             npp_load_levels switches the feature off (the table has a row per level).  With the level pool on, npp_step has
 *             already drawn the next level when the ending row is accumulated: the ended episode is charged to the level it was
 *             played on and the new one starts on the drawn level.
 * npp_set_episode_stats(h, enable): allocates the planes and the table for the loaded levels (NPP_ERR_STATE without), zeroes them
 *   and sets both levels of every record to -1; 0 frees them.  A failed allocation is NPP_ERR_HIP and leaves the previous state.
 * npp_episode_accumulate: n_steps rows [n_steps][n_envs] of flags, frames and reward, and, when not NULL, components
 *   f32[n_steps][n_envs][6] (8-byte aligned; NULL: the component doubles are neither read nor written).  Call it once per npp_step /
 *   npp_step_many, after npp_step_reward when the reward comes from there.  Every row is passed in: the handle remembers no
 *   pointer.  It joins a split step (npp_set_obs_overlap) first.  d_ended (u8[n_envs] or NULL): 1 where this call finished an episode.
 * npp_episode_restart: the RESET (from_restore == 0) or RESTORE event for the envs of a device mask (NULL = all), for callers
 *   that start episodes by other means.
 * npp_episode_view: the plane bases and the table, valid until the next npp_set_episode_stats / npp_load_levels, rewritten in
 *   stream order.  npp_episode_table_reset zeroes the table.
 * Each of these is NPP_ERR_INVALID on a NULL handle and NPP_ERR_STATE while the feature is off.
 * npp_episode_apply_host: the same rule without a GPU or a handle, for tests, on ONE env: rec_i32[NPP_EP_NI], rec_f64[NPP_EP_ND] and
 *   table u64[n_levels][16] (NULL with n_levels == 0) are updated in place by `count` events of 8 words each: {0, flags, frames,
 *   level_now, has_components} a step row whose reward and six components are rows[8 * i + 0 .. 6]; {1, level_now} RESET;
 *   {2, level_now} RESTORE; {3} npp_tick; {4} INIT; {5, level_now} the players' clearing.  *ended (may be NULL): 1 when a row
 *   finished an episode.  NPP_ERR_INVALID for a NULL record, flags outside 0..255, frames outside 0..65535 or an unknown kind. */
enum {
    NPP_EP_STEPS = 0, NPP_EP_FRAMES = 1, NPP_EP_SWITCH_STEP = 2, NPP_EP_SWITCH_FRAMES = 3, NPP_EP_LEVEL = 4, NPP_EP_BITS = 5,
    NPP_EP_FIN = 6, NPP_EP_FIN_FLAGS = 12, NPP_EP_N_FINISHED = 13, NPP_EP_NI = 14,
    NPP_EP_RET = 0, NPP_EP_COMP = 1, NPP_EP_DFIN = 7, NPP_EP_ND = 14
};
enum {
    NPP_EPC_EPISODES = 0, NPP_EPC_WON, NPP_EPC_DEAD, NPP_EPC_TRUNCATED, NPP_EPC_DEAD_MINE, NPP_EPC_DEAD_IMPACT, NPP_EPC_SWITCH,
    NPP_EPC_STEPS, NPP_EPC_FRAMES, NPP_EPC_WON_FRAMES, NPP_EPC_RETURN_FIX, NPP_EPC_RESTORED, NPP_EPC_ABANDONED, NPP_EP_COLS = 16
};
int npp_set_episode_stats(npp_handle h, int enable);
int npp_episode_accumulate(npp_handle h, const uint8_t *d_flags, const uint16_t *d_frames, const float *d_reward,
                           const float *d_components /* or NULL */, int n_steps, uint8_t *d_ended /* [N] or NULL */);
int npp_episode_restart(npp_handle h, const uint8_t *d_mask /* NULL = all */, int from_restore);
int npp_episode_view(npp_handle h, const int32_t **d_i32, const double **d_f64, const uint64_t **d_table);
int npp_episode_table_reset(npp_handle h);
int npp_episode_apply_host(int32_t *rec_i32, double *rec_f64, uint64_t *table, int n_levels, int autoreset, const int32_t *events,
                           const float *rows, int count, uint8_t *ended);

/* Launch geometry: lanes_per_env wavefront lanes cooperate on one environment (power of two, 1..64; 0 = choose from
 * n_envs so that the grid fills the chip), waves_per_block wavefronts share one LDS copy of a level (1..4, 0 = auto).
 * Results are bit-identical for every geometry; only speed changes. */
int npp_set_launch_geometry(npp_handle h, int lanes_per_env, int waves_per_block);
int npp_get_launch_geometry(npp_handle h, int *lanes_per_env, int *waves_per_block);

/* Host-only (no GPU, no handle): the per-env "zoo block" (doors' edge counters + moving entities) a level SET needs.
 * The block is sized over ALL levels of the set -- the reset kernel initialises the doors / movers of every level, not
 * only of those with moving entities -- and npp_load_levels refuses a plan that does not cover one of its levels. */
int npp_plan_zoo_block(const double *blob, const int64_t *offsets, int n_levels, int *doors, int *movers, int *words);

/* Frame stacking (the reference's FrameStackWrapper, nclone/gym_environment/frame_stack_wrapper.py; device rings in
 * npp_stack.hip).  Replaces the wrapper's deques (frame_stack_wrapper.py:123-129) with one ring per stacked key and env:
 * 2 K slots, the entry at ring position q stored in slots q and q + K, so every window of K entries is contiguous.
 * npp_set_frame_stack: visual_k / state_k entries of player_frame / game_state (1..12, the range checked at
 *   frame_stack_wrapper.py:116-121; 0 = that key is not stacked), padding 0 "zero" or 1 "repeat" (frame_stack_wrapper.py:183-188).
 *   (Re)allocates zeroed rings; invalid arguments return NPP_ERR_INVALID.  Synchronises the handle's stream.
 * npp_frame_stack_render: player_frame of every env straight into the ring slots of the entry the next push completes
 *   (npp_render_player_frame with a ring stride; the observation overlap applies the same way).
 * npp_frame_stack_push: completes one entry -- the observation() append of frame_stack_wrapper.py:334-338 -- from d_game_state
 *   [N,41] (and the frame rendered before), and re-pads every env that was reset: reset_all, or (d_flags[e] & reset_bits) != 0
 *   (the in-kernel auto-reset).  Re-padding writes the K - 1 older entries of the window (reset() / _reset_to_checkpoint_from_wrapper,
 *   frame_stack_wrapper.py:190-264).  d_terminal_stack [N,state_k,41] (may be NULL; needs state stacking and d_terminal_state):
 *   per env the stack it shows after this push, except that a reset env gets the last K - 1 entries of its previous window
 *   followed by d_terminal_state[e].  Launch it after npp_join: it reads the outputs of the observation kernels.
 * npp_frame_stack_view: which 0 = player_frame ring (u8 elements), 1 = game_state ring (f32 elements): *base, and the element
 *   offset of env 0's oldest entry and the element stride between envs of the current window (its K entries of 7056 or 41
 *   elements are contiguous, oldest first).  Valid until the next push. */
int npp_set_frame_stack(npp_handle h, int visual_k, int state_k, int padding);
int npp_frame_stack_render(npp_handle h);
int npp_frame_stack_push(npp_handle h, const float *d_game_state, const float *d_terminal_state, const uint8_t *d_flags,
                         int reset_bits, int reset_all, float *d_terminal_stack);
int npp_frame_stack_view(npp_handle h, int which, void **base, int64_t *offset, int64_t *batch_stride);

/* Level pool: a new level for every episode (EnvMapLoader.load_map, env_map_loader.py:111-208, which draws a category by weight
 * (_select_category, :210-234; set_curriculum_weights, :312) and a map inside it; npp_environment.py:516-557 fast-resets only when
 * the same map comes up again).  The pool is the loaded level set plus one weight per level.
 * npp_set_level_pool: weights f64[n_levels] (n_levels == npp_num_levels), all finite and >= 0, not all zero; weights == NULL turns the
 *   pool off (the default: every env keeps its level, byte-identical to a handle that never had a pool).  May be called again between
 *   steps (curriculum updates): the next draw uses the new weights.  NaN, negative or infinite weights, an all-zero vector and a wrong
 *   length return NPP_ERR_INVALID.  A call with the pool's current seed keeps the per-env draw counts (a curriculum update); turning
 *   the pool on or changing the seed restarts them at 0.  Refused while an entity is repositioned
 *   (npp_set_entity_pos), which is refused in turn while the pool is on.  npp_load_levels turns the pool off.
 * With the pool on, npp_step with NPP_FLAG_AUTORESET draws for every env whose flags show won, dead or truncated, after the step
 *   kernel (and after joining an observation overlap): an env that drew ANOTHER level is assigned it exactly as by npp_assign_levels
 *   (Simulator.reset with fresh entities, reachability cache row and per-episode dictionary dropped, dynamic truncation limit of the
 *   new level) and its observation rows of `out` (game_state, action_mask, entity_pos, spatial_context, positions) are rewritten with
 *   the new level's spawn observation; flags, reward, frames and terminal_state keep describing the episode that ended.  An env that
 *   drew its own level keeps the step kernel's auto-reset (fast_reset under NPP_FLAG_FAST_RESET).  Observation kernels called after
 *   npp_step see the new levels.  npp_step_many and npp_tick never draw (their in-kernel resets stay on the current level).
 * npp_draw_levels: every env whose mask byte is non-zero (NULL = all) draws now, with the same consequences for envs that change
 *   level; the others are not touched (NppVecEnvironment.reset draws this way before its reset).  NPP_ERR_STATE without a pool.
 * The draw of env e with per-env draw count c (u32, starts at 0, +1 per draw; independent of the 13-bit episode counter):
 *     mix(z)  = z += 0x9E3779B97F4A7C15; z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9; z = (z ^ z >> 27) * 0x94D049BB133111EB; z ^ z >> 31
 *     u       = mix(mix(((uint64_t)e << 32) | c) ^ seed)                      (splitmix64 rounds, arithmetic mod 2^64)
 *     t       = (double)(u >> 11) * 2^-53 * cdf[n - 1]                        (cdf[l] = w[0] + ... + w[l], summed in f64 in index order)
 *     level   = the number of l with cdf[l] <= t, or the last level of non-zero weight if that is n
 *   so level l comes up with probability w[l] / sum(w), weight-0 levels never, and the draw depends on nothing but (seed, e, c):
 *   not on launch geometry, build variant, observation overlap or stream.  The reference's own draws (Python `random`) are not
 *   reproduced.  The draw counts and levels are part of npp_snapshot / npp_restore.
 * npp_get_env_levels: i32[n_envs], the level every env plays now (synchronises).
 * npp_env_level_view: *d_levels = the device array i32[n_envs] behind it (valid while the handle lives; the draws rewrite it in
 *   stream order, so a consumer on the handle's stream sees the levels of the step it follows).
 * npp_level_pool_draw_host (host-only): the same draw for `count` (env, count) pairs, with the same weight checks. */
int npp_set_level_pool(npp_handle h, const double *weights, int n_levels, uint64_t seed);
int npp_draw_levels(npp_handle h, const uint8_t *env_mask);
int npp_get_env_levels(npp_handle h, int32_t *host_out);
int npp_env_level_view(npp_handle h, const int32_t **d_levels);
int npp_level_pool_draw_host(const double *weights, int n_levels, uint64_t seed, const int32_t *envs, const uint32_t *counts, int count,
                             int32_t *out);

/* Evaluation sweep: a fixed list of levels, each played an exact number of times, one outcome per episode (the reference's eval_mode:
 * EnvMapLoader walks its test suite in order, env_map_loader.py:138-162; create_evaluation_env).  A third assignment policy beside the
 * level pool's draw and the goal curriculum's variant: take the next job from a list.  The rule (csrc/npp_sweep.hpp):
 *   jobs      i32[n_jobs] level ids in the caller's order; job j is ONE episode on level jobs[j].
 *   state     counters i32[3] = next (jobs handed out), done (jobs finished), n_jobs; env_job i32[n_envs], the job an env plays, -1 =
 *             idle; one result row per job as planes i32[NPP_SWEEP_RI][n_jobs] -- the six words of the finished episode
 *             (NPP_EP_STEPS .. NPP_EP_BITS), the flags byte of its ending step (NPP_SWEEP_R_FLAGS), the env that played it
 *             (NPP_SWEEP_R_ENV, -1 until then) and status (NPP_SWEEP_R_STATUS: 0 pending, 1 done) -- and f64[NPP_SWEEP_RD][n_jobs], the
 *             return and the six component sums.
 *   start     env e < min(n_envs, n_jobs) takes job e, is put on level jobs[e] and reset as by npp_assign_levels; the other envs are
 *             idle and keep their level; next = min(n_envs, n_jobs).
 *   step      after every npp_step, in the place of the pool's draw: the envs whose flags show won, dead or truncated AND that hold a
 *             job, taken in env order, get ranks 0, 1, ...; the env of rank r takes job j = next + r (next as before the step): with
 *             j < n_jobs it is assigned level jobs[j] exactly as the pool assigns a drawn level (reset, observation rows rewritten
 *             and the level's dynamic truncation limit when the level is another one; the step kernel's auto-reset stands when it
 *             is the same), otherwise it goes idle: it plays on where it is and nothing it does is recorded.  next += the number
 *             of ranked envs, so next runs past n_jobs by the envs that found the queue dry.  One workgroup ranks the row without
 *             atomics: the same bits in every run.  npp_step_many, npp_tick and npp_reset never assign.
 *   collect   npp_episode_accumulate with n_steps == 1 copies, for every env whose job ended in the step, the finished half of its
 *             episode record into the job's row and adds 1 to done.  The contract is ONE npp_episode_accumulate behind EVERY npp_step
 *             while a sweep runs; the sweep is over when done == n_jobs.
 * npp_sweep_start(h, jobs, n_jobs): NPP_ERR_STATE, each with its own text: n_jobs <= 0; episode statistics off; a handle without
 *   NPP_FLAG_AUTORESET; the level pool on; the goal curriculum on; a checkpoint archive exists; an entity repositioned with
 *   npp_set_entity_pos.  NPP_ERR_INVALID for a job outside the loaded levels.  A start while a sweep runs begins a new one.
 * While a sweep runs, NPP_ERR_STATE: npp_set_level_pool, npp_set_goal_curriculum, npp_archive_create, npp_demo_create / npp_demo_play,
 *   npp_archive_seed, npp_assign_levels, a repositioning npp_set_entity_pos, npp_snapshot and npp_restore (a restored env's job would be
 *   undefined).  What holds with the level pool on holds here: no LDS level staging, the zoo kernels run when any env or any job level
 *   has zoo entities, the step-variant autotuner decides once, npp_get_env_levels reads back.
 * npp_sweep_stop(h): the sweep ends, every env keeps the level it plays, and the handle steps with the bytes of one that never had a
 *   sweep.  npp_load_levels and npp_set_episode_stats(h, 0) end it as well.  Without a sweep nothing is allocated or launched.
 * npp_sweep_view: device pointers (any may be NULL), valid until the next npp_sweep_start / npp_load_levels and rewritten in stream
 *   order; they outlive npp_sweep_stop.  NPP_ERR_STATE before the first start.
 * npp_sweep_assign_host (host-only, for tests): one `step` of the rule on host arrays -- counters i32[3] in / out; level_trunc i32[n_levels]
 *   or NULL (then trunc is not touched).  NPP_ERR_INVALID for a negative size, a missing array, an env_job outside -1 .. n_jobs - 1. */
enum { NPP_SWEEP_R_FLAGS = 6, NPP_SWEEP_R_ENV = 7, NPP_SWEEP_R_STATUS = 8, NPP_SWEEP_RI = 9, NPP_SWEEP_RD = 7 };
int npp_sweep_start(npp_handle h, const int32_t *jobs, int n_jobs);
int npp_sweep_stop(npp_handle h);
int npp_sweep_view(npp_handle h, const int32_t **d_env_job, const int32_t **d_results_i32, const double **d_results_f64,
                   const int32_t **d_counters /* next | done | n_jobs */, int *n_jobs);
int npp_sweep_assign_host(const uint8_t *flags, int end_bits, int n_envs, const int32_t *jobs, int n_jobs, int32_t *counters, int32_t *env_job,
                          int32_t *prev_job, int32_t *env_level, int32_t *trunc, const int32_t *level_trunc, int n_levels, uint8_t *changed);

/* Graph observations for the GCN encoder: graph_node_feats, graph_edge_index, graph_node_mask, graph_edge_mask of the reference's
 * training Dict (OBSERVATION_SPACE_README.md; gym_environment/npp_environment.py:245-271).  The reference builds the graph at every
 * reset from the freshly loaded level (mixins/graph_mixin.py:96-109, 340-376) and keeps it for the episode, so it is a constant per
 * level: the masked, flood-filled `adjacency` of GraphBuilder.build_graph (the one npp_reachability restates) converted by
 * create_graph_data (graph/edge_building.py:124-272) with the node features of graph/feature_builder.py:67-197, entities in their
 * spawn state.  Nodes: the endpoints of edges in (x, y) order, at most 2500 (one node at (0, 0) when there is no edge); edges in the
 * adjacency's dict order, those touching a truncated node skipped, at most 20000.  Unlike npp_reachability, levels with several exits
 * are served.
 * npp_graph_observation: rows of env e -- d_node_feats f32[N][2500][6], d_edge_index u16[N][2][20000], d_node_mask u8[N][2500],
 *   d_edge_mask u8[N][20000], zero padded -- hold the graph of the level env e plays.  The handle keeps, per env, the level its rows
 *   hold (-1 = none) and rewrites, whole, only the rows of envs whose current level (npp_env_level_view) differs; a call on an
 *   unchanged batch is one small launch.  A call with another buffer set than the last, or with flags bit 0, rewrites every row.
 *   npp_load_levels forgets what the rows hold.  d_node_feats, d_edge_index and d_edge_mask must be 16-byte aligned.  Joins an
 *   observation overlap first (the result does not depend on it).  NPP_ERR_UNSUPPORTED while an entity is repositioned with
 *   npp_set_entity_pos (the reference rebuilds from the moved positions; not restated).  The per-level tables are built at the first
 *   call (host work, about 140 KB of HBM per level at most).
 * npp_graph_compile (host-only, no GPU, no handle): one level's rows -- feats f32[2500][6], edge_index u16[2][20000], zero padded --
 *   and counts i32[2] = (num_nodes, num_edges); any output may be NULL. */
int npp_graph_observation(npp_handle h, float *d_node_feats, uint16_t *d_edge_index, uint8_t *d_node_mask, uint8_t *d_edge_mask, int flags);
int npp_graph_compile(const double *map, int64_t n, float *feats, uint16_t *edge_index, int32_t *counts);

/* Frame augmentation of player_frame and global_view: what the reference's FrameStackWrapper.observation does to both keys at every
 * observation when AugmentationConfig.enable_augmentation is set, its default (gym_environment/config.py:64-87;
 * frame_stack_wrapper.py:343-377, 402-462 -> frame_augmentation.apply_augmentation; a stacked player_frame gets ONE transform for all
 * its frames, _apply_consistent_augmentation).  The four transforms, their order and their gates are the reference's pipeline
 * (frame_augmentation.py:56-103): translate (gate 0.8 p), horizontal flip (0.4 p), coarse dropout (0.5 p), brightness / contrast
 * (0.4 p).  PARITY WITH ALBUMENTATIONS' PIXELS IS UNPINNED, and the draws are a counter-based hash, not numpy's stream: what is pinned
 * is the integer definition of DESIGN.md 15 (nclone_amd/csrc/npp_augment.hpp; numpy model tests/frame_aug_ref.py), bit for bit.
 * One parameter set is AugParams, 14 int32 words: gate mask (bit 0 translate, 1 flip, 2 dropout, 3 brightness / contrast), sx, sy
 * (shift in 1/32 px), hole count, two holes of (h, w, y0, x0), a, b (v <- clamp((a v + b) >> 8, 0, 255)).
 * npp_set_frame_augmentation(h, enable, p, scale, seed): enable != 0 allocates (or keeps) the two destination buffers -- u8
 *   [n_envs][max(K, 1)][84][84] for player_frame, K the visual stack size of npp_set_frame_stack, and u8 [n_envs][176][100] for
 *   global_view -- and sets the augmentation call count to 0; enable == 0 frees them (the default: nothing allocated, nothing
 *   launched).  p outside [0, 1], a scale other than 0.7 (light), 1.0 (medium) or 1.3 (strong), or a handle without visual outputs --
 *   no player_frame rendered or stacked, or no global_view rendered yet -- return NPP_ERR_INVALID.  Synchronises the handle's stream.
 *   Call it again after npp_set_frame_stack changed K.
 * npp_frame_augment(h, host_params): one augmentation call for every env, on the handle's stream.  It reads player_frame from the
 *   frame ring's current window when the handle stacks it, else from where npp_render_player_frame last wrote, and global_view from
 *   where npp_render_global_view last wrote (both must still be allocated, 16-byte aligned), and never writes them: the ring keeps
 *   clean frames, which come back in later stacks under other draws.  Call it after npp_join and after npp_frame_stack_push (the
 *   padding of reset envs must be in the ring).  host_params == NULL: env e draws its parameters for target t (0 player_frame, 1
 *   global_view) from (seed, e, call count c, t):
 *     base = mix(mix(((uint64_t)e << 32) | c) ^ seed ^ (t * 0xD1B54A32D192ED03)), word j = mix(base + j)     (mix: npp_set_level_pool)
 *     words: 0 translate gate, 1 sx, 2 sy, 3 flip gate, 4 dropout gate, 5 hole count, 6-9 / 10-13 holes, 14 b/c gate, 15 a, 16 b;
 *     a gate passes when (word >> 11) * 2^-53 < probability; an integer in [lo, hi] is lo + (((word >> 32) * (hi - lo + 1)) >> 32)
 *   otherwise host_params is int32 [n_envs][2][14], AugParams per env and target, used in place of the draw (rejected with
 *   NPP_ERR_INVALID when a hole leaves the image or a value leaves the arithmetic's range).  Either way the call count advances by
 *   one; npp_snapshot / npp_restore leave it alone (observation noise, not simulation state).
 * npp_frame_augment_view(h, which, base, bytes): which 0 = the player_frame destination, 1 = global_view's; valid until the next
 *   npp_set_frame_augmentation, rewritten by the next npp_frame_augment.  NPP_ERR_STATE while the feature is off.
 * npp_frame_augment_params_host (host-only): the draw for `count` (env, call count, target) triples, out int32 [count][14].
 * npp_frame_augment_apply_host (host-only): the per-pixel function the kernel compiles on `count` frames u8 [count][height][width]
 *   with params int32 [count][14]. */
int npp_set_frame_augmentation(npp_handle h, int enable, double p, double scale, uint64_t seed);
int npp_frame_augment(npp_handle h, const int32_t *host_params);
int npp_frame_augment_view(npp_handle h, int which, void **base, int64_t *bytes);
int npp_frame_augment_params_host(uint64_t seed, double p, double scale, const int32_t *envs, const uint32_t *counts, const int32_t *targets,
                                  int count, int32_t *out);
int npp_frame_augment_apply_host(const uint8_t *frames, int count, int height, int width, const int32_t *params, uint8_t *out);

/* Demonstration transitions from recorded replays, played as one batch: what the reference's ReplayExecutor.execute_replay
 * (replay/replay_executor.py:304-462) and DemonstrationBuffer (replay/demonstration_buffer.py:72-209) produce one replay at a time in
 * Python, for R replays over the handle's n_envs envs.  For a replay with input bytes in[0 .. L) and frame skip fs:
 *   load     a level assignment plus Simulator.reset (NPlayHeadless.load_map_from_map_data); every byte is one NPlayHeadless.tick with
 *            decode_input_to_controls' controls -- npp_tick's semantics: NO stop at a win or a death
 *   rows     a transition AFTER tick f whenever (f + 1) % fs == 0: rows = min(L / fs, max_transitions); the trailing L % fs ticks yield
 *            nothing, ticks behind the cap are unobservable and are not promised to run
 *   columns  frame = f; action = map_input_to_action(in[f]) (bytes 6, 7 and above -> 0); done = 1 on the replay's last row
 *   game_state[0:40] = get_ninja_state() after tick f; game_state[40] = the EXECUTOR's time value max(0, (L - (f + 1)) / L), an fp64
 *            division rounded once to f32 (replay_executor.py:537-544) -- not the env's truncation value
 *   action_mask  all ones (:595); with NPP_DEMO_MASK_ENV the mask npp_observe produces
 *   reachability_features, spatial_context, switch_states, mine_sdf_features: DELIBERATELY the rows npp_observe / npp_reachability_ex
 *            give for the state (the env's definitions, pinned against the reference's env), not the executor's private variants
 * The dataset is replay-major in the CALLER's order and time-ordered inside a replay: replay r owns rows row_base[r] .. + rows[r].
 * npp_demo_plan_host (host only): rows i32[n], row_base i64[n], the schedule order i32[n] (the replays with rows > 0 by descending
 *   rows, ties by index; -1 padded; round q plays entries q * n_envs .. one per env), round_ticks i32[n] (max rows of the round x fs;
 *   0 padded), counts i32[2] = scheduled replays, rounds; *rows_total.  Any output may be NULL.  NPP_ERR_INVALID for frame_skip < 1, a
 *   negative length, n_envs < 1, max_transitions < 0: nothing is written.
 * npp_demo_create: uploads the ragged byte table (HOST inputs u8[offsets[n]], offsets i64[n + 1] from 0) and the plan for the handle's
 *   n_envs.  levels[r] names a level of the loaded set (the caller de-duplicates maps); out of range: NPP_ERR_INVALID.  key_flags:
 *   NPP_DEMO_* planes to fill.  NPP_ERR_STATE while action routes, reward mode "pbrs", action masking, frame stacks, the level pool or
 *   the observation overlap are on (the player ticks outside their bookkeeping); NPP_ERR_UNSUPPORTED with the reachability keys where
 *   npp_reachability refuses a level.  Replaces a previous object.  npp_demo_destroy frees it; npp_load_levels drops it.
 * npp_demo_play: plays every round and fills `out` (DEVICE pointers, one plane [rows_total][dim] per key of key_flags; the per-row
 *   columns may be NULL).  Per round: npp_assign_levels (envs without a replay get the level of the round's first replay and zero
 *   inputs) and a full reset -- the assignment synchronises as it always does --, then per period, on the handle's stream and without
 *   synchronisation or host read-back: the feed kernel (ragged table -> [fs][n_envs] input rows), npp_tick, npp_observe,
 *   npp_reachability_ex when its keys are on, and the collect kernel, which writes row row_base[r] + p of every plane for every env
 *   whose replay has a row in period p and NOTHING for the others.  Rows of `out` that belong to no transition do not exist; the
 *   call leaves the handle on the last round's levels.  d_flags: NPP_F_WON | NPP_F_DEAD | NPP_F_SWITCH of the row's state;
 *   d_status: npp_reachability's status word (0 without its keys). */
enum {
    NPP_DEMO_GAME_STATE = 1u << 0, NPP_DEMO_ACTION_MASK = 1u << 1, NPP_DEMO_ENTITY_POSITIONS = 1u << 2, NPP_DEMO_SPATIAL_CONTEXT = 1u << 3,
    NPP_DEMO_REACHABILITY = 1u << 4, NPP_DEMO_MINE_SDF = 1u << 5, NPP_DEMO_SWITCH_STATES = 1u << 6, NPP_DEMO_POSITIONS = 1u << 7,
    NPP_DEMO_MASK_ENV = 1u << 16
};
typedef struct NppDemoOut {
    float *d_game_state;            /* [rows,41]  */
    int8_t *d_action_mask;          /* [rows,6]   */
    float *d_entity_positions;      /* [rows,6]   */
    float *d_spatial_context;       /* [rows,112] */
    float *d_reachability_features; /* [rows,38]  */
    float *d_mine_sdf_features;     /* [rows,3]   */
    float *d_switch_states;         /* [rows,25]  */
    double *d_positions;            /* [rows,6] f64: player, exit switch, exit door in pixels */
    uint8_t *d_action;              /* [rows] 0..5 */
    int32_t *d_frame;               /* [rows] */
    uint8_t *d_done;                /* [rows] */
    int32_t *d_replay;              /* [rows] the caller's replay index */
    int32_t *d_level;               /* [rows] levels[replay] */
    uint8_t *d_flags;               /* [rows] */
    int32_t *d_status;              /* [rows] */
} NppDemoOut;
int npp_demo_plan_host(const int64_t *lengths, int n_replays, int frame_skip, int64_t max_transitions, int n_envs, int32_t *rows,
                       int64_t *row_base, int32_t *order, int32_t *round_ticks, int32_t *counts, int64_t *rows_total);
int npp_demo_create(npp_handle h, const uint8_t *inputs, const int64_t *offsets, const int32_t *levels, int n_replays, int frame_skip,
                    int64_t max_transitions, unsigned key_flags);
int npp_demo_destroy(npp_handle h);
int npp_demo_rows(npp_handle h, int64_t *rows_total, int32_t *n_rounds, int64_t *ticks_total);
int npp_demo_play(npp_handle h, const NppDemoOut *out);

/* Seeding the cell index from recorded replays: what the reference's DemoCheckpointSeeder (replay/demo_checkpoint_seeder.py) does
 * before training starts -- it plays every matching .replay file tick by tick (_extract_positions_from_demo_simple, :667-809),
 * keeps one checkpoint per cell, the one with the highest score (extract_best_checkpoints), drops checkpoints nearer than 72 px to
 * the exit door once the switch is on (:30, :118-153), and hands (cell, action_sequence, score) to the archive -- on the handle
 * that owns the index, with the handle's envs as players.  Meant for the start of training.  The rule is this
 * library's own definition; for a replay r with input bytes in[0 .. L) on level levels[r] of the loaded set:
 *   play       as npp_demo_play with frame skip 1: per round npp_assign_levels plus a full reset, one NPlayHeadless.tick per byte
 *              with decode_input_to_controls' controls, NO stop at a win or a death; the schedule is npp_demo_plan_host's with
 *              frame_skip = 1 and max_transitions = max L: longest first, ties by index, round q plays entries q * n_envs .. one per env
 *   candidate  the state after tick f (0 <= f < L) of an env that holds a replay in this round; idle envs and ticks past a replay's
 *              end never are (a mask byte the feed kernel writes, not an accident of the state).  One npp_archive_explore per tick,
 *              in tick order, over the candidates: eligibility, key, winner, ties and slot allocation are exactly explore's.  An
 *              incumbent therefore wins a tie against every later tick, round or replay; inside one tick the lowest env wins
 *   deviation  the reference appends the tick on which the ninja died before it breaks (:798-802; the cumulative-reward path
 *              :310-312).  Here ninja states 6 to 9 are not eligible, as everywhere in the index: a dead state is no checkpoint.
 *              The winning tick is removed on both sides by the 72 px filter.  Ticks behind the reference's break run here and
 *              are never eligible (the ninja stays won or dead)
 *   score      score_mode 0 "progress": (float)((double)f / (double)L), the seeder's frame_idx / max(1, total_frames) (:777-779);
 *              1 "frames": the index's own NULL score -(float)frame (frame = f + 1), the scale of npp_archive_explore(d_score =
 *              NULL) during training; 2 "table": d_scores[offsets[r] + f], a DEVICE f32 array ragged like the inputs (any return the
 *              trainer computed itself); NaN = not eligible, as in explore
 *   counts     seeding changes neither visits nor chosen: it adds cells, not visits.  n_used, cell_slot, cell_score, slot_key and
 *              the records change as under explore
 *   routes     with action routes on (npp_set_routes), the record of a candidate after tick f carries the route
 *              map_input_to_action(in[0 .. f]) (bytes 6, 7 and above -> 0; the table npp_demo_play's `action` column uses):
 *              frame_skip 1, frames f + 1, the level, the flags of the state.  Route bit 2 ("not replayable") is set from the first
 *              byte b whose action's controls differ from decode_input_to_controls(b) -- b == 7, or b >= 8 with (b & 7) not in
 *              {0, 6} -- and only then: npp_tick's blanket bit 2 does not reach these records.  Bit 1 when f + 1 exceeds the
 *              capacity, as for a step.  Without routes nothing route-related is launched
 *   afterwards the handle stays on the last round's levels, like npp_demo_play; every env's current and finished route is empty
 * npp_archive_seed: HOST inputs u8[offsets[n]], offsets i64[n + 1] from 0, levels i32[n]; d_scores DEVICE (mode 2 only); d_counts
 *   DEVICE i32[n_replays][4] or NULL, zeroed by the call: candidates, eligible, stored (explore status 0), archive full (status 7) per
 *   replay -- integer atomic adds whose return value is not used.  Per tick, on the handle's stream and without synchronisation
 *   or host read-back inside a round: the feed kernel (input byte, action, candidate mask, score, route-mismatch latch per env),
 *   the tick, the route append when routes are on, propose (without the visit count), assign, store.  The assignment of every round
 *   synchronises as it always does, and the call synchronises once at its end, before its tables are freed.
 *   NPP_ERR_STATE without a cell index, for the causes npp_archive_explore names, and for the causes npp_demo_create names EXCEPT
 *   action routes.  NPP_ERR_INVALID for a level id out of range, offsets[0] != 0, a negative length, an unknown score_mode, mode 2
 *   without d_scores.  A refused call changes nothing: complete or not at all, as npp_demo_create is.
 * npp_archive_seed_rows_host (host only, for tests): the per-tick rows of the rule for ONE replay -- actions u8[len], route_bits
 *   u8[len] (2 from the first mismatching byte on; bit 1 depends on a capacity and is not included), scores f32[len] for score_mode
 *   0 or 1 (another mode: NPP_ERR_INVALID).  Any output may be NULL. */
int npp_archive_seed(npp_handle h, const uint8_t *inputs, const int64_t *offsets, const int32_t *levels, int n_replays, int score_mode,
                     const float *d_scores, int32_t *d_counts);
int npp_archive_seed_rows_host(const uint8_t *in, int64_t len, int score_mode, uint8_t *actions, uint8_t *route_bits, float *scores);

/* Goal curriculum: the exit switch and the exit door slide along the level's optimal path in stages (IntermediateGoalManager,
 * gym_environment/reward_calculation/intermediate_goal_manager.py; GoalCurriculumConfig, reward_config.py:953-983; the env side at
 * npp_environment.py:703-1000 and base_environment.py:404-481).  DESIGN.md 25 has the scope, the reference's quirks and the rule.
 * A (level, stage) pair is a VARIANT LEVEL: the level compiled with the two positions overridden, appended to the handle's level set
 * behind the base levels, so the step, the observations of the entity tables, the pool, the archive and the episode table serve it
 * and no kernel of the step changes.
 * NppGoalCurriculumParams: stage_distance_interval (pixels, > 0), advancement_threshold (completion rate in [0, 1]), rolling_window
 *   (outcomes per level, 1..8192), auto_advance (the device advances a level's stage; 0 = only npp_goal_set_stage does).
 * npp_set_goal_curriculum(h, enable, params): enable != 0 builds the stage table of every loaded level (build_paths_for_level,
 *   :158-336, and the two getters, :570-696, from the ORIGINAL positions), compiles the variants (apply_to_simulator, :698-1012,
 *   carried statically in the cell lists) and RELOADS the level set as base levels + variants: like npp_load_levels it switches the
 *   level pool, the archive, the reward mode, episode statistics, the demonstration player and snapshots off, so call it first.
 *   Every env restarts on the stage-0 variant of the base level it played.  enable == 0 reloads the base levels alone.
 *   npp_load_levels switches the mode off.  NPP_ERR_STATE without levels; NPP_ERR_INVALID for numbers outside the ranges above or a
 *   level with more than 1024 stages.  While the mode is on, level ids an entry point TAKES (npp_assign_levels, npp_set_level_pool's
 *   weights) are base ids; level ids it REPORTS (npp_get_env_levels, the episode table, archive records) are ids of the whole set,
 *   and npp_goal_tables maps them back.  A level without both paths has no stages and stays on its base level.
 * The rule, once per npp_step under NPP_FLAG_AUTORESET, behind the step kernel (two launches, npp_goal.hip): (1) every env whose
 *   episode ended counts into its own three counters (update_from_episode, :1014-1038) and, when it played its level's CURRENT stage,
 *   appends its `won` bit to the level's ring, in env-index order; (2) with auto_advance a level whose ring is full with at least
 *   `need` wins (the smallest w with (double)w / window >= threshold) and that is not at its last stage advances by one and clears its
 *   ring; (3) a pending stage (npp_goal_set_stage) replaces the stage, and every env that ended is put on the variant of its level's
 *   stage -- with the level pool on, of the level the pool drew -- exactly as the pool assigns a level.  npp_reset and
 *   npp_draw_levels run (3) alone for the envs they restart; npp_assign_levels takes base ids and maps them.
 * npp_goal_set_stage(h, level, stage): level -1 = all base levels; deferred to the env's next episode start as in the reference
 *   (set_curriculum_stage, base_environment.py:404-481), clamped to num_stages - 1.
 * npp_goal_view: device views, valid until the mode is switched: level words i32[NPP_GOAL_LEVEL_WORDS][n_base] (stage, pending,
 *   num_stages, first variant id, ring fill, ring head, wins, advances, appended, stale), ring u32[n_base][ring_words], env words
 *   i32[NPP_GOAL_ENV_WORDS][n_envs] (episode_count, switch_activation_count, completion_count, switch latch, level at the last end).
 * npp_goal_tables (host): base_of i32[n_levels], stage_of i32[n_levels] (-1 = a base level); either may be NULL; *n_base.
 * npp_goal_stage_positions(h, level, ...): num_stages, the three distances, the original positions f64[4] and per stage the switch
 *   and door position f64[cap][4] of a base level.
 * Served on variants and pinned against the reference there: npp_reachability[_ex], npp_minimal_observation,
 *   npp_path_action_mask, reward mode "pbrs" without the waypoints (a variant's level constants take the manager's fractional
 *   positions, pbrs_potentials.py:952-955).  npp_graph_observation is NPP_ERR_UNSUPPORTED while the mode is on: nothing pins the
 *   graph rows of a moved level.
 * Refused while the mode is on (NPP_ERR_STATE, each with its own text): npp_set_reward_waypoints (the reference recomputes the paths
 *   to the moved goals, main_reward_calculator.py:1254-1297), npp_demo_create and npp_archive_seed (the replays belong to the base
 *   levels), npp_step_many (its inner steps have no episode boundary the rule could see).
 * Host-only: npp_goal_stages_host -- the stage table of one level; npp_goal_apply_host -- one application of the rule on host
 *   arrays laid out as the views (drawn: the pool's draw per env or NULL; count 0 = step (3) alone);
 *   npp_compile_level_segments_goal / _entities_goal -- the dumps of a variant (goal_xy f64[4] switch x, y, door x, y; NULL = the
 *   level itself); order i32[rows][4] = CSR slot, list-order number after Simulator.reset, after fast_reset, place in the fast walk. */
typedef struct NppGoalCurriculumParams {
    double stage_distance_interval;
    double advancement_threshold;
    int32_t rolling_window;
    int32_t auto_advance;
} NppGoalCurriculumParams;
#define NPP_GOAL_LEVEL_WORDS 10
#define NPP_GOAL_ENV_WORDS 5
void npp_goal_default_params(NppGoalCurriculumParams *out);
int npp_set_goal_curriculum(npp_handle h, int enable, const NppGoalCurriculumParams *params);
int npp_goal_set_stage(npp_handle h, int level, int stage);
int npp_goal_view(npp_handle h, const int32_t **d_level_words, const uint32_t **d_ring, const int32_t **d_env_words, int *n_base,
                  int *ring_words, int *need);
int npp_goal_tables(npp_handle h, int32_t *base_of, int32_t *stage_of, int *n_base);
int npp_goal_stage_positions(npp_handle h, int level, int32_t *num_stages, double *dist, double *orig, int stage_cap, double *pos);
int npp_goal_stages_host(const double *map, int64_t n, double interval, int32_t *num_stages, double *dist /* [3] */, double *orig /* [4] */,
                         int stage_cap, double *pos /* [stage_cap][4] */, int path_cap, int32_t *path0, int32_t *path1, int32_t *path_len);
int npp_goal_apply_host(int32_t *level_words, uint32_t *ring, int32_t *env_words, const int32_t *base_of, const int32_t *stage_of, int n_base,
                        int n_levels, int n_envs, int window, int need, int auto_advance, const uint8_t *flags, int end_bits, int count,
                        int32_t *env_level, const int32_t *drawn, uint8_t *changed);
/* Host-only: npp_reach_rollout_host, npp_path_direction_host, npp_reward_level_constants_host and npp_reward_host_wp on a variant (goal_xy f64[4] as above; NULL = the level itself). */
int npp_reward_level_constants_goal_host(const double *map, int64_t n, const double *goal_xy, double *out, int32_t *status);
int npp_reward_goal_host(const double *map, int64_t n, const double *goal_xy, const NppRewardParams *params, const NppWaypointParams *wp,
                         const double *pos0, const double *pos, const uint8_t *flags, const uint16_t *frames, int count, int end_bits,
                         double *reward_out, double *components_out, uint8_t *kind_out, int32_t *status, double *wp_bonus_out,
                         int32_t *wp_info_out);   /* wp must be NULL with goal_xy */
int npp_reach_rollout_goal_host(const double *map, int64_t n, const double *goal_xy, const double *pos, const int32_t *mines,
                                const uint8_t *new_episode, int count, float *out, int32_t *status, double *raw_out);
int npp_path_direction_goal_host(const double *map, int64_t n, const double *goal_xy, const double *pos, const uint8_t *switch_activated,
                                 int count, int8_t *direction_out, uint8_t *from_graph_out, int32_t *status);
int npp_compile_level_segments_goal(const double *map, int64_t n, const double *goal_xy, int16_t *out, int max_rows, int *n_out,
                                    uint32_t *unsupported_mask);
int npp_compile_level_entities_goal(const double *map, int64_t n, const double *goal_xy, double *out, int max_rows, int *n_out, int32_t *order);

int npp_num_envs(npp_handle h);
int npp_num_levels(npp_handle h);

#ifdef __cplusplus
}
#endif
#endif /* NPP_AMD_H */
