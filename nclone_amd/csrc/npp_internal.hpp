// npp_internal.hpp -- structures shared between the C ABI (npp_capi.cpp) and the HIP kernels (npp_kernels.hip).
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>

#include "npp_goal.hpp"
#include "npp_state.hpp"
#include "npp_zoo_layout.hpp"

namespace npp {

// ---- SoA ninja state: f64 plane k of env e lives at d_f64[k * n_envs + e] (coalesced per wave) -------------------
enum F64Plane { F_X = 0, F_Y, F_VX, F_VY, F_VXO, F_VYO, F_FNX, F_FNY, F_CNX, F_CNY, F_SCX, F_SCY, NF64 };  // F_SC*: position of the cached mine overlay
// u32 planes U_A .. U_E: npp_state.hpp has the planes and their bit layout

// Per-level header (device copy); offsets are bytes into the level blob.
// The "hot" region [off_hot, off_hot + hot_bytes) = seg_start | ent_start | cell_bounds | segs is what a
// workgroup stages into LDS when all of its envs play this level.
struct LevelHdr {
    uint32_t off_hot;
    uint32_t hot_bytes;   // multiple of 16
    uint32_t off_ent_x;   // f64[n_ent]
    uint32_t off_ent_y;   // f64[n_ent]
    uint32_t off_ent_meta;  // u32[n_ent]
    uint32_t off_init_words;  // u32[n_words]
    uint32_t off_tiles;   // u8[1100]
    uint32_t off_raster;  // u16[n_ent + n_mov] draw order (npp_level.hpp: raster_order); read by write_spatial_context only --
                          // the rasteriser walks off_draw_recs
    uint32_t off_doors;   // f64[5 * n_door]
    uint32_t n_door;
    uint32_t n_seg;
    uint32_t n_ent;
    uint32_t n_words;
    uint32_t n_think;
    int32_t obs_switch;
    int32_t obs_door;
    uint32_t fits_lds;
    // entity zoo (all zero / unused when has_zoo == 0)
    uint32_t has_zoo;
    uint32_t off_ent_seq;   // u16[n_ent]
    uint32_t off_ent_cell;  // u16[n_ent]
    uint32_t off_mov_meta;  // u32[n_mov]
    uint32_t off_mov_x0;    // f64[n_mov]
    uint32_t off_mov_y0;    // f64[n_mov]
    uint32_t off_edges;     // u32[2 * EDGE_WORDS]
    uint32_t off_door_tab;  // u32[2 * n_zdoor]
    uint32_t n_mov;
    uint32_t n_zdoor;
    uint32_t n_created;
    uint32_t n_balls;
    uint32_t ball_first;    // mover slot of the first death ball
    uint32_t off_ent_rank;  // u16[n_ent] list-order number after a fast reset (entity_dic rank)
    uint32_t off_mov_rank;  // u16[n_mov]
    uint32_t off_ent_perm;  // u16[n_ent] CSR walk order after a fast reset
    uint32_t off_ent_ident; // u16[n_ent] identity walk order
    uint32_t off_keep_words;  // u32[n_words] state bits a fast reset keeps
    uint32_t off_draw_recs;   // uint4[n_ent + n_mov] drawables in draw order (npp_level.hpp: draw_recs); 16-byte aligned
    double db_count;
    int32_t locked_slots[5];   // CSR slots of the first five locked doors (entity_dic[6] order), -1 = none
    int32_t pad_;
    double spawn_x, spawn_y;
    double sw_x, sw_y, door_x, door_y;
};

// offsets inside the hot region (bytes)
constexpr uint32_t HOT_SEG_START = 0;      // u16[1101] (2202 -> padded 2208)
constexpr uint32_t HOT_ENT_START = 2208;   // u16[1101]
constexpr uint32_t HOT_BOUNDS = 4416;      // u8[1100] (-> padded 1104)
constexpr uint32_t HOT_SEGS = 5520;        // u16[n_seg]

struct StepOut {
    float *game_state;
    int8_t *action_mask;
    float *entity_pos;
    uint8_t *flags;
    float *reward;
    uint16_t *frames;
    float *terminal_state;
    float *spatial_context;
    double *positions;
    uint16_t *work;
};

struct KernelArgs {
    double *f64;          // [NF64][n]
    uint32_t *u32;        // [NU32][n]
    uint32_t *ent_bits;   // [n_words_max][n]
    float *sc_cache;      // [n][48] cached mine overlay of spatial_context
    const int32_t *env_level;   // [n]
    const int32_t *trunc_limit; // [n]
    const LevelHdr *hdr;  // [n_levels]
    const unsigned char *blob;
    const uint8_t *tile_canvas;   // u8 [n_levels][600][1056]: tile-layer coverage counts (render kernels only; built lazily)
    const uint8_t *inputs;  // actions [n] (mode 0) or replay bytes [n_ticks][n] (mode 1)
    const uint8_t *reset_mask;  // reset kernel only; NULL = all
    const uint8_t *obs_mask;    // observe launches (n_ticks == 0) only: the envs whose rows are written (a device mask); NULL = all.
                                // Workgroups without a masked env return at once; the rows of the other envs are left alone
    int n;
    int n_ticks;          // frame_skip (mode 0) or tick count (mode 1); 0 = observe only
    int n_steps;          // mode 0: Gymnasium steps per launch (npp_step_many); 0 / 1 = one
    int mode;             // 0 gym step, 1 raw ticks
    int autoreset;
    int n_words_max;
    int lanes_per_env;    // G
    int waves_per_block;  // WPB
    uint32_t lds_hot_cap; // bytes reserved for a staged level
    int lds_level;        // 1: every workgroup is level-uniform and its level fits lds_hot_cap -> stage it in LDS
    // entity zoo: per-env block of zoo_words 8-byte words at zoo[env * zoo_words] (layout: ZOO_* below)
    double *zoo;
    int zoo_words;
    int zoo_doors;        // door slots per env (max over levels)
    int zoo_movers;       // mover slots per env (max over levels)
    int zoo_active;       // 1: some env currently plays a level with zoo entities -> the zoo step kernel runs
    int reset_fresh;      // reset kernel: 1 = this reset is the first creation after a (re)assignment of levels
    int fast_reset;       // reset kernel: this reset is a Simulator.fast_reset; step kernels: auto-resets are fast resets
    int reset_auto;       // reset kernel, with fast_reset: envs without a Simulator.reset since their level assignment (S_FRESH,
                          // npp_state.hpp) get a full reset instead -- the reference env's first reset() (npp_environment.py:518-557)
    // npp_step only (null elsewhere): heavy-first launch order of the workgroups -- wg_order[blockIdx.x] is the block of envs this
    // workgroup steps, wg_cost[block] the shader clocks its last launch took (launch_cost_order rebuilds the order from the costs)
    const uint32_t *wg_order;
    uint32_t *wg_cost;
    int wg_first, wg_count;   // split launch: this launch covers entries [wg_first, wg_first + wg_count) of the order; wg_count == 0 =
                              // the whole grid
    // observation overlap (npp_set_obs_overlap): the step is launched in parts -- the workgroups expected to run long on streams of
    // their own -- and `phase` (u8[n], written by npp_phase_kernel before the parts are launched) says which part steps an env; the
    // observation kernels are then launched once per part, each instance on its part's stream, skipping the envs of the other
    // parts (phase == NULL: no filter).  The step kernel itself does not look at it.
    uint8_t *phase;
    int phase_id;
    int variant;          // build variant of the G = 16 plain step kernels (npp_kernels.hip: VariantK); 0 everywhere else
    StepOut out;
};

constexpr int WAVE = 64;

constexpr int EDGE_WORDS_D = 142;   // == npp::EDGE_WORDS (npp_level.hpp)

// Launch geometry: G lanes cooperate on one environment (G in {1,2,4,8,16,32,64}); a wavefront holds 64/G envs; a
// workgroup holds WPB wavefronts that share one LDS copy of a level when all their envs play the same level.
// dynamic LDS layout: [hot_cap][ent words: n_words_max * envs_per_block * 4][obs staging: envs_per_block * 41 * 4][pad to 8]
//                     [spill rows: envs_per_block * LDS_SPILL_BYTES][zoo blocks + grid edges]
// spill row of an env (round 3): what the step kernel parks in LDS instead of scratch memory -- the eight ninja doubles that are
// dead during the collision loops (64 B) and the DepenIO / DepenIOZ block handed to the out-of-line depenetration fallback
constexpr int LDS_SPILL_BYTES = 208;   // 8 doubles | 8 ints | DepenIOZ (104 B, from byte 96)
__host__ __device__ inline size_t lds_spill_offset(uint32_t hot_cap, int n_words_max, int envs_per_block) {
    const size_t b = (size_t)hot_cap + (size_t)n_words_max * envs_per_block * 4 + (size_t)envs_per_block * 41 * 4;
    return (b + 7) & ~(size_t)7;
}
__host__ __device__ inline size_t lds_zoo_offset(uint32_t hot_cap, int n_words_max, int envs_per_block) {
    return lds_spill_offset(hot_cap, n_words_max, envs_per_block) + (size_t)envs_per_block * LDS_SPILL_BYTES;
}
inline size_t lds_bytes(uint32_t hot_cap, int n_words_max, int envs_per_block, int zoo_words = 0) {
    size_t b = lds_zoo_offset(hot_cap, n_words_max, envs_per_block);
    // zoo kernels add, per env: the zoo block and a private copy of the level's grid-edge bitmaps
    if (zoo_words) b += (size_t)envs_per_block * ((size_t)zoo_words * 8 + 2 * EDGE_WORDS_D * 4);
    return b;
}

hipError_t launch_step(const KernelArgs &a, hipStream_t s);
hipError_t launch_reset(const KernelArgs &a, hipStream_t s);
// stride: bytes between the frames of consecutive envs; mirror: non-zero = each frame is also written `mirror` bytes further on
hipError_t launch_render(const KernelArgs &a, uint8_t *d_out, int centered, hipStream_t s, uint32_t stride = 84 * 84, uint32_t mirror = 0);
// npp_stack.hip: one frame-stack push (see npp_frame_stack_push in include/npp_amd.h)
struct StackArgs {
    int n;
    int visual_k, state_k;        // 0 = that ring is off
    int vhead, shead;             // ring position of the entry this push completes (its slots are head and head + K)
    int repeat;                   // padding: 0 zeros, 1 copies of the newest entry
    int reset_bits, reset_all;    // env e is re-padded when reset_all or (flags[e] & reset_bits)
    const uint8_t *flags;
    const float *game_state;      // [n][41] this step's entry
    const float *terminal_state;  // [n][41] (reset envs) the state at the terminal step
    uint8_t *frames;              // [n][2 visual_k][84 * 84]
    float *state;                 // [n][2 state_k][41]
    float *terminal_stack;        // [n][state_k][41] or null
};
hipError_t launch_stack_push(const StackArgs &a, hipStream_t s);
// npp_pool.hip: the level pool's draw (see npp_set_level_pool in include/npp_amd.h)
struct PoolArgs {
    int n;
    const uint8_t *flags;         // env e draws when flags[e] & bits
    int bits;
    const double *cdf;            // [n_levels] cumulative weights
    int n_levels, last;           // last: the last level of non-zero weight
    uint64_t seed;
    uint32_t *count;              // [n] draw counts
    int32_t *env_level;           // [n]
    int32_t *trunc;               // [n] truncation limits
    const int32_t *level_trunc;   // [n_levels] dynamic truncation limit per level; null = dynamic truncation off
    uint8_t *changed;             // [n] out: 1 = the env drew another level than it played (every other byte 0)
};
hipError_t launch_pool_draw(const PoolArgs &a, hipStream_t s);
// npp_goal.hip: the goal curriculum's bookkeeping (see npp_set_goal_curriculum in include/npp_amd.h; the rule: npp_goal.hpp)
struct GoalArgs {
    GoalState g;
    const uint8_t *flags;         // [n] env e's episode ended when flags[e] & bits
    int bits;
    int count;                    // 1: outcomes are counted (a step); 0: only the levels at the end and pending stages (explicit restarts)
    int32_t *env_level;           // [n]
    int32_t *trunc;               // [n] truncation limits
    const int32_t *level_trunc;   // [n_levels] or null, as PoolArgs
    uint8_t *changed;             // [n] out: 1 = the env starts its next episode on another level than it ended on
    int32_t *list;                // [2][n] scratch, the ended envs in env order: base level | stage * 2 + won (stage -1: a base level)
};
hipError_t launch_goal_update(const GoalArgs &a, hipStream_t s);
hipError_t launch_goal_assign(const GoalArgs &a, hipStream_t s);
// npp_sweep.hip: the evaluation sweep (see npp_sweep_start in include/npp_amd.h; the rule: npp_sweep.hpp)
struct SweepArgs {
    int n, n_jobs;
    const int32_t *jobs;          // [n_jobs] level ids
    int32_t *counters;            // [3] next | done | n_jobs
    int32_t *env_job, *prev_job;  // [n]
    // assign: the step's flags row and what the level pool's draw writes
    const uint8_t *flags;         // [n] env e's episode ended when flags[e] & bits
    int bits;
    int32_t *env_level;           // [n]
    int32_t *trunc;               // [n] truncation limits
    const int32_t *level_trunc;   // [n_levels] or null, as PoolArgs
    uint8_t *changed;             // [n] out: 1 = the env's next job is on another level than it played (every other byte 0)
    // collect: the episode records (EpisodeArgs) and the result planes
    const int32_t *ep_i32;        // [EP_NI][n]
    const double *ep_f64;         // [EP_ND][n]
    int32_t *res_i32;             // [SWEEP_RI][n_jobs]
    double *res_f64;              // [SWEEP_RD][n_jobs]
};
hipError_t launch_sweep_assign(const SweepArgs &a, hipStream_t s);
hipError_t launch_sweep_collect(const SweepArgs &a, hipStream_t s);
// npp_augment.hip: one augmentation call (see npp_frame_augment in include/npp_amd.h; the draw and the pixels: npp_augment.hpp)
struct AugArgs {
    int n, k;                     // k: player_frame entries per env (the visual stack size, or 1)
    const uint8_t *pf_src;        // env e's k entries are contiguous from pf_src + e * pf_stride (frame ring window / output block)
    size_t pf_stride;
    const uint8_t *gv_src;        // [n][176 * 100]
    uint8_t *pf_dst, *gv_dst;     // [n][k][84 * 84], [n][176 * 100]
    const int32_t *params;        // [n][2][AUG_WORDS] used in place of the draw; null = draw
    uint64_t seed;
    uint32_t count;               // the handle's augmentation call count
    double p;
    int s10;                      // intensity scale * 10
};
hipError_t launch_frame_augment(const AugArgs &a, hipStream_t s);
// npp_cells.hip: the cell index over the checkpoint archive (see npp_archive_cells_create in include/npp_amd.h; the rule:
// npp_cells.hpp).  K = n_levels * NPP_CELLS_PER_LEVEL keys.
struct CellArgs {
    int n, n_levels, n_slots;
    // the live state the key and the default score are read from
    const double *f64;            // [NF64][n]
    const uint32_t *u32;          // [NU32][n]
    const uint32_t *ent;          // [n_words_max][n]
    const int32_t *env_level;     // [n]
    const LevelHdr *hdr;          // [n_levels]
    // the caller's arrays
    const float *score;           // [n] or null = -(float)frame
    const uint8_t *mask;          // [n] or null = all envs
    int32_t *status;              // explore: [n] or null
    int32_t *slots_out;           // select: [n]
    // the tables
    unsigned long long *best;     // [K] high word = ordered score bits; low word 0xffffffff = incumbent, 0xfffffffe - env = proposal; 0 = empty
    int32_t *cell_slot;           // [K] -1 = the key has no slot
    float *cell_score;            // [K]
    uint32_t *visits, *chosen;    // [K]
    int32_t *slot_key;            // [n_slots]
    int32_t *n_used;              // [1]
    int32_t *env_key;             // [n] propose -> assign: the env's key, -1 = masked out or not eligible
    int32_t *slot_of_env;         // [n] assign -> store: the slot the env's state goes to, -1 = none
    unsigned long long *cdf;      // [K] select: inclusive prefix sums of the weights inside each level
    uint64_t seed;
    uint32_t call;                // select call number
    int no_count;                 // propose: 1 = leave visits alone (npp_archive_seed adds cells, not visits); 0 everywhere else
};
hipError_t launch_cells_propose(const CellArgs &a, hipStream_t s);
hipError_t launch_cells_assign(const CellArgs &a, hipStream_t s);
hipError_t launch_cells_cdf(const CellArgs &a, hipStream_t s);
hipError_t launch_cells_pick(const CellArgs &a, hipStream_t s);
// npp_route.hip: action routes (see npp_set_routes in include/npp_amd.h; the rule: npp_route.hpp)
struct RouteArgs {
    int n, cap;
    int32_t *hdr;                 // [n][ROUTE_HDR_WORDS]
    uint8_t *act;                 // [n][2][cap]
    // append: the rows of one step launch
    int n_steps, frame_skip, autoreset;
    const uint8_t *actions;       // [n_steps][n]
    const uint8_t *flags;         // [n_steps][n]
    const uint16_t *frames;       // [n_steps][n]
    const int32_t *env_level;     // [n]
    const uint8_t *phase;         // observation overlap: only the envs of part phase_id (null = all)
    int phase_id;
    // event: one of ROUTE_EV_* for the envs with a non-zero mask byte (null = all)
    const uint8_t *mask;
};
enum RouteEvent { ROUTE_EV_FLIP = 0, ROUTE_EV_TICK = 1, ROUTE_EV_INIT = 2 };
hipError_t launch_route_append(const RouteArgs &a, hipStream_t s);
hipError_t launch_route_event(const RouteArgs &a, int event, hipStream_t s);
// npp_episode.hip: episode statistics (see npp_set_episode_stats in include/npp_amd.h; the rule: npp_episode.hpp)
struct EpisodeArgs {
    int n, n_levels;
    int32_t *i32;                 // [EP_NI][n]
    double *f64;                  // [EP_ND][n]
    unsigned long long *table;    // [n_levels][EP_COLS]
    const int32_t *env_level;     // [n]
    // accumulate: the rows of one step launch
    int n_steps, autoreset;
    const uint8_t *flags;         // [n_steps][n]
    const uint16_t *frames;       // [n_steps][n]
    const float *reward;          // [n_steps][n]
    const float *comps;           // [n_steps][n][6] or null: the component planes are then neither loaded nor stored
    uint8_t *ended;               // [n] or null: 1 = the call finished an episode of the env
    // event: the envs, as RewardArgs selects them
    const uint8_t *mask;
    const int32_t *envs;
    const int32_t *env_status;
    int count;
};
hipError_t launch_episode(const EpisodeArgs &a, hipStream_t s);
hipError_t launch_episode_event(const EpisodeArgs &a, int event, hipStream_t s);
// npp_graph.hip: graph observation rows (see npp_graph_observation in include/npp_amd.h; tables: npp_graph.hpp)
struct GraphHdr;
struct GraphArgs {
    int n, n_levels;
    int all;                      // 1: rewrite every row
    const int32_t *env_level;     // [n] the level env e plays
    int32_t *row_level;           // [n] the level env e's rows hold, -1 = none; set to env_level[e] once they are written
    const GraphHdr *hdr;          // [n_levels]
    const unsigned char *blob;
    float *feats;                 // [n][2500][6]     (16-byte aligned)
    uint16_t *edges;              // [n][2][20000]    (16-byte aligned)
    uint8_t *node_mask;           // [n][2500]
    uint8_t *edge_mask;           // [n][20000]       (16-byte aligned)
};
hipError_t launch_graph_rows(const GraphArgs &a, hipStream_t s);
// max_records: the largest number of draw records (closed-door strokes + entities + movers) of a loaded level; sizes the LDS
// order / cost: u32[n] each -- the launch order of the envs (heaviest first) and the clocks every env's wavefront took; `reorder`
// rebuilds the order from the costs before the launch (null order = env order)
hipError_t launch_global_view(const KernelArgs &a, int max_records, const uint8_t *gv_p, const float *gv_h, const uint8_t *gv_v,
                              uint8_t *d_out, uint32_t *order, uint32_t *cost, int reorder, hipStream_t s);
// per-level static tables of global_view (the level right after a reset; needs the tile canvas): gv_p u8[n_levels][600][1056]
// (+ 16 bytes) picture, gv_h f32[n_levels][600][100] horizontal sums, gv_v u8[n_levels][176][100] view
hipError_t launch_gv_static(const KernelArgs &a, int n_levels, uint8_t *gv_p, float *gv_h, uint8_t *gv_v, hipStream_t s);
hipError_t launch_full_frame(const KernelArgs &a, int env0, int count, uint8_t *d_out, hipStream_t s);
hipError_t launch_switch_states(const KernelArgs &a, float *d_out, hipStream_t s);
// npp_reach_kernel.hip (tables: npp_reach.hpp)
struct ReachHdr;
// per-env arrays behind ReachMiss (npp_reach_features.hpp): allocated only when a loaded level takes the reference's miss branch
struct ReachMissDev {
    uint32_t *stamp;   // [n][REACH_CELLS]
    double *raw;       // [n][REACH_CELLS]
    uint32_t *epoch;   // [n] current epoch of the env's entries (stamp == epoch: live); 0 = never called
    uint32_t *last_episode;   // [n] episode counter (S_EPISODE, npp_state.hpp) seen at the last call
};
// min_out (f32[n][40], may be NULL): the minimal observation rows, assembled by the same launch; sc_rows (f32[n][112], needed with
// min_out): the spatial_context rows the step kernel wrote for this observation
hipError_t launch_reach(const KernelArgs &a, const ReachHdr *rh, const unsigned char *rblob, uint32_t *key, float *cache,
                        const ReachMissDev &md, float *out, float *sdf_out, int32_t *status, float *sw_out, float *min_out,
                        const float *sc_rows, hipStream_t s);
// envs selected by a.reset_mask (NULL = all) lose their cached vector and their miss dictionary (a new level)
hipError_t launch_reach_drop(const KernelArgs &a, uint32_t *key, const ReachMissDev &md, hipStream_t s);
// npp_pathmask.hip: path-direction action masking (see npp_set_action_masking in include/npp_amd.h; the rule: npp_pathmask.hpp)
struct PathMaskArgs {
    int n;
    const double *f64;            // [NF64][n]
    const uint32_t *ent_bits;     // [n_words_max][n]
    const int32_t *env_level;     // [n]
    const LevelHdr *hdr;          // [n_levels]
    const ReachHdr *rh;           // [n_levels] the reachability tables (npp_reach.hpp)
    const unsigned char *rblob;
    const uint8_t *flags;         // [n] flags row of the step that produced this observation; null = no step did
    int end_bits;                 // flags bits after which the step kernel auto-reset the env (0 without auto-reset)
    int8_t *mask;                 // [n][6] in / out, null = leave the mask alone (soft mode)
    int8_t *dir;                  // [n] or null
    int32_t *status;              // [n] or null: 1 = classified from the graph
    uint32_t *observed, *applied, *last_observed, *last_applied;   // [n] each
};
hipError_t launch_path_mask(const PathMaskArgs &a, hipStream_t s);
hipError_t launch_path_mask_restart(int n, const uint8_t *mask, uint32_t *observed, uint32_t *applied, hipStream_t s);
// npp_reward.hip: reward mode "pbrs" (see npp_set_reward_mode in include/npp_amd.h; the rule: npp_reward.hpp)
struct RewardLevel;
struct RewardArgs {
    int n;
    const double *f64;            // [NF64][n]
    const uint32_t *u32;          // [NU32][n]
    const uint32_t *ent_bits;     // [n_words_max][n]
    const int32_t *env_level;     // [n]
    const LevelHdr *hdr;          // [n_levels]
    const ReachHdr *rh;           // [n_levels] the reachability tables (npp_reach.hpp)
    const unsigned char *rblob;
    const RewardLevel *rl;        // [n_levels] the levels' constants
    double params[6];             // NppRewardParams
    double *sd;                   // [RW_ND][n] the per-env reward state (npp_reward.hpp RewardState), doubles
    uint32_t *si;                 // [RW_NI][n] ... words
    ReachMissDev md;              // the path calculator's per-episode dictionary, shared with npp_reachability (null pointers: none)
    uint32_t *stamp2;             // [n][REACH_CELLS] the fallback query's own dictionary, or null
    double *raw2;
    const uint8_t *flags;         // [n] flags row of the step
    const uint16_t *frames;       // [n] frames row of the step
    int end_bits;                 // flags bits after which the step kernel auto-reset the env (0 without auto-reset)
    const uint8_t *mask;          // restart: the envs (null = all) ...
    const int32_t *envs;          // ... or, when not null, a list of `count` envs, entry i skipped when env_status[i] != 0
    const int32_t *env_status;    //     (null = none skipped; an entry outside 0 .. n - 1 is skipped)
    int count;
    float *reward;                // [n]
    float *comps;                 // [n][6] or null
    int32_t *status;              // [n] or null
    const double *wp_bonus;       // [n] the step's waypoint bonus (npp_waypoint_kernel), or null: waypoints off
};
hipError_t launch_reward(const RewardArgs &a, hipStream_t s);
hipError_t launch_reward_restart(const RewardArgs &a, int init, hipStream_t s);
// npp_waypoint.hip: the sequential path waypoints of reward mode "pbrs" (see npp_set_reward_waypoints in include/npp_amd.h; the rule:
// npp_waypoint.hpp)
struct WaypointHdr;
struct WaypointArgs {
    int n;
    const double *f64;            // [NF64][n]
    const int32_t *env_level;     // [n]
    const WaypointHdr *wh;        // [n_levels] the levels' waypoint tables
    const unsigned char *wblob;
    double params[3];             // collection radius, out-of-order scale, progress scale
    uint32_t *state;              // [WP_NI][n] the per-env collected set, next expected index, collected count
    const uint8_t *flags;         // [n] flags row of the step
    int end_bits;                 // flags bits after which the step kernel auto-reset the env (0 without auto-reset)
    const uint8_t *mask;          // restart: the envs, as RewardArgs selects them
    const int32_t *envs;
    const int32_t *env_status;
    int count;
    double *bonus;                // [n] the step's unscaled bonus, read by npp_reward_kernel
    float *bonus_out;             // [n] or null
    int32_t *info_out;            // [n][3] or null
};
hipError_t launch_waypoint(const WaypointArgs &a, hipStream_t s);
hipError_t launch_waypoint_restart(const WaypointArgs &a, hipStream_t s);
// npp_demo.hip: demonstration transitions from recorded replays (see npp_demo_create in include/npp_amd.h; the plan: npp_demo.hpp)
struct DemoOut {   // NppDemoOut of include/npp_amd.h, field by field
    float *game_state;
    int8_t *action_mask;
    float *entity_positions, *spatial_context, *reachability_features, *mine_sdf_features, *switch_states;
    double *positions;
    uint8_t *action;
    int32_t *frame;
    uint8_t *done;
    int32_t *replay, *level;
    uint8_t *flags;
    int32_t *status;
};
struct DemoArgs {
    int n, fs, period;            // envs, frame skip, the period of the round (its ticks are period * fs ..)
    const int32_t *slot;          // [n] the replay env e plays in this round, -1 = none
    const uint8_t *inputs;        // the ragged input table
    const int64_t *offsets;       // [n_replays + 1]
    const int32_t *rows;          // [n_replays]
    const int64_t *row_base;      // [n_replays]
    const int32_t *rep_level;     // [n_replays]
    uint8_t *staging;             // feed: [fs][n] input rows of the period
    // collect: the player's observation rows, one per env (a plane that is off is null, and so is its destination)
    const float *gs, *epos, *sc, *reach, *sdf, *sw;
    const int8_t *mask;
    const uint8_t *flags;
    const double *pos;
    const int32_t *rstatus;       // npp_reachability's status row, or null
    int mask_ones;                // action_mask is the executor's all ones
    DemoOut out;
};
hipError_t launch_demo_feed(const DemoArgs &a, hipStream_t s);
hipError_t launch_demo_collect(const DemoArgs &a, hipStream_t s);
// npp_seed.hip: seeding the cell index from recorded replays (see npp_archive_seed in include/npp_amd.h; the rows: npp_seed.hpp)
struct SeedArgs {
    int n, tick;                  // envs; the tick f of the round the rows are for
    int score_mode;               // SeedScoreMode
    int feed;                     // feed kernel: 1 = write the rows of tick f, 0 = only count the tick before (behind a round's last tick)
    const int32_t *slot;          // [n] the replay env e plays in this round, -1 = none
    const uint8_t *inputs;        // the ragged input table
    const int64_t *offsets;       // [n_replays + 1]
    const float *scores;          // mode 2: ragged like the inputs
    // the rows of the coming tick, one entry per env
    uint8_t *staging;             // the input byte npp_tick's launch reads (0 for an idle env and past a replay's end)
    uint8_t *action;              // map_input_to_action of it
    uint8_t *mask;                // 1 = the state after this tick is a candidate
    float *score;
    uint8_t *latch;               // 1 from the first byte of the round whose action does not press the byte's controls
    // counters: the explore status of the tick before (null at a round's first tick) and where they go (null = none)
    const int32_t *status;        // [n]
    int32_t *counts;              // [n_replays][4] candidates | eligible | stored | full
    // route append (routes on): the state the flags are read from and the env's route
    const uint32_t *u32;          // [NU32][n]
    const uint32_t *ent;          // [n_words_max][n]
    const int32_t *env_level;     // [n]
    const LevelHdr *hdr;          // [n_levels]
    int32_t *route_hdr;           // [n][ROUTE_HDR_WORDS]
    uint8_t *route_act;           // [n][2][cap]
    int cap;
};
hipError_t launch_seed_feed(const SeedArgs &a, hipStream_t s);
hipError_t launch_seed_route(const SeedArgs &a, hipStream_t s);
hipError_t launch_phase_assign(const uint32_t *order, int blocks, int epb, int n, const int *edge, int parts, uint8_t *phase, hipStream_t s);
hipError_t launch_spin(long long ticks, hipStream_t s);   // a bounded idle wavefront (stream calibration)
// order <- the indices 0 .. n - 1 sorted by cost, heaviest first (128 logarithmic bins; any costs give a permutation)
hipError_t launch_cost_order(const uint32_t *cost, uint32_t *order, int n, hipStream_t s);
hipError_t launch_tile_tables(hipStream_t s);   // per-device tile gray tables of the player_frame kernel
hipError_t launch_tile_canvas(const LevelHdr *d_hdr, const unsigned char *d_blob, uint8_t *d_canvas, int n_levels, hipStream_t s);

}  // namespace npp
