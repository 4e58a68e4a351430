// npp_capi.cpp -- the C ABI declared in include/npp_amd.h: handle management, level upload, launches.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/npp_amd.h"
#include "npp_archive.hpp"
#include "npp_augment.hpp"
#include "npp_cells.hpp"
#include "npp_demo.hpp"
#include "npp_episode.hpp"
#include "npp_goal.hpp"
#include "npp_graph.hpp"
#include "npp_host.hpp"
#include "npp_internal.hpp"
#include "npp_level.hpp"
#include "npp_reach_build.hpp"
#include "npp_reward.hpp"
#include "npp_waypoint.hpp"
#include "npp_seed.hpp"
#include "npp_sweep.hpp"

using namespace npp;

namespace {

// Owners of the handle's device resources: released when they are dropped or reassigned, never by hand.  Kernel arguments stay
// plain pointers (.get()); the caller's stream is borrowed and never wrapped.
template <class T> class DevBuf {   // n elements of T in device memory
    T *p_ = nullptr;
    size_t n_ = 0;

  public:
    DevBuf() = default;
    DevBuf(DevBuf &&o) noexcept { *this = std::move(o); }
    DevBuf &operator=(DevBuf &&o) noexcept { reset(); std::swap(p_, o.p_); std::swap(n_, o.n_); return *this; }
    ~DevBuf() { reset(); }
    hipError_t alloc(size_t n, size_t pad = 0) {   // `pad` bytes past the end: for kernels that read rows as aligned dword groups
        reset();
        const hipError_t e = hipMalloc((void **)&p_, n * sizeof(T) + pad);
        if (e == hipSuccess) n_ = n; else p_ = nullptr;
        return e;
    }
    void reset() { if (p_) (void)hipFree(p_); p_ = nullptr; n_ = 0; }
    T *get() const { return p_; }
    size_t size() const { return n_; }
    size_t bytes() const { return n_ * sizeof(T); }
    explicit operator bool() const { return p_ != nullptr; }
};

template <class T, hipError_t (*Create)(T *, unsigned), hipError_t (*Destroy)(T)> class HipObject {   // a HIP event or stream
    T o_ = nullptr;

  public:
    HipObject() = default;
    HipObject(HipObject &&o) noexcept { *this = std::move(o); }
    HipObject &operator=(HipObject &&o) noexcept { reset(); std::swap(o_, o.o_); return *this; }
    ~HipObject() { reset(); }
    hipError_t create(unsigned flags) {
        reset();
        const hipError_t e = Create(&o_, flags);
        if (e != hipSuccess) o_ = nullptr;
        return e;
    }
    void reset() { if (o_) (void)Destroy(o_); o_ = nullptr; }
    T get() const { return o_; }
    explicit operator bool() const { return o_ != nullptr; }
};
using Event = HipObject<hipEvent_t, hipEventCreateWithFlags, hipEventDestroy>;
using Stream = HipObject<hipStream_t, hipStreamCreateWithFlags, hipStreamDestroy>;   // one the handle created

// live per-env state (npp_create)
struct EnvState {
    DevBuf<double> f64;             // [NF64][n]
    DevBuf<uint32_t> u32;           // [NU32][n]
    DevBuf<int32_t> level, trunc;   // level and truncation limit (host mirrors: npp_handle_s::env_level / trunc)
    DevBuf<uint8_t> mask;           // a caller's env mask, copied for a launch
    DevBuf<float> sc;               // [n][48] spatial-context cache
    DevBuf<uint32_t> count;         // level pool draw counts
};

// global_view's per-level tables: picture / horizontal sums / view of the level right after a reset
struct GvTables {
    DevBuf<float> h;
    DevBuf<uint8_t> v, p;
};

// reachability observation (npp_reachability): per-level tables + per-env cache
struct Reach {
    DevBuf<ReachHdr> hdr;
    DevBuf<unsigned char> blob;
    DevBuf<uint32_t> key;   // (ninja cell, exit_switch_activated) of the cached vector, 0 = none
    DevBuf<float> cache;    // [n][REACH_DIM + 1]
    // per-env dictionary of the miss branch (levels with ReachHdr::miss_exit only)
    DevBuf<uint32_t> stamp, epoch, last_episode;
    DevBuf<double> raw;
    ReachMissDev miss() const { return {stamp.get(), raw.get(), epoch.get(), last_episode.get()}; }
};

// graph observations (npp_graph_observation): per-level tables + what the caller's rows hold
struct GraphObs {
    DevBuf<GraphHdr> hdr;
    DevBuf<unsigned char> blob;
    DevBuf<int32_t> row_level;   // [n] the level env e's rows hold, -1 = none
    const void *rows[4] = {nullptr, nullptr, nullptr, nullptr};   // the buffer set row_level describes
};

// The loaded level set and everything derived from it: replaced whole by npp_load_levels
struct LevelSet {
    std::vector<CompiledLevel> levels;
    std::vector<std::vector<double>> maps;   // map_data of the base levels (the goal curriculum compiles its variants from them)
    int n_base = 0;                          // levels [0, n_base) were loaded by the caller; the rest are goal-curriculum variants
    std::vector<LevelHdr> hdrs;
    int n_words_max = 1;
    uint32_t hot_max = 0;   // largest staged-level size over the set
    int zoo_words = 0, zoo_doors = 0, zoo_movers = 0;
    DevBuf<unsigned char> blob;   // staged levels
    DevBuf<LevelHdr> hdr;
    DevBuf<uint32_t> ent;         // [n_words_max][n] entity words
    DevBuf<double> zoo;           // [n][zoo_words] per-env zoo blocks (at least the 8-word head)
    // built on first use
    DevBuf<uint8_t> canvas;       // tile-layer coverage canvas of every level (render paths)
    GvTables gv;
    Reach reach;
    GraphObs graph;
    std::vector<int32_t> level_trunc;   // [n_levels] dynamic truncation limit (empty = not computed)
    DevBuf<int32_t> d_level_trunc;      // the same on the device (level pool + dynamic truncation)
    DevBuf<double> pool_cdf;            // [n_levels] (level pool)
};

// The snapshot slot (npp_snapshot / npp_restore): one record per env in the checkpoint archive's layout (npp_archive.hpp), written
// and read by its kernels, record e for env e
struct Snapshot {
    ArchiveLayout lay;
    DevBuf<uint32_t> rec;           // [n][lay.words]
    std::vector<uint8_t> ovr;       // npp_handle_s::ovr at npp_snapshot (the records' zoo block heads carry the repositioning itself)
    unsigned long long gen = ~0ull;   // npp_handle_s::assign_gen at npp_snapshot
};

// heavy-first launch orders and the costs they are built from (sized by n: kept across npp_load_levels)
struct Orders {
    DevBuf<uint32_t> wg_order, wg_cost;   // npp_step: workgroup order and per-block costs
    int wg_blocks = 0;
    long step_launches = 0;
    DevBuf<uint32_t> pf_order, pf_cost;   // npp_render_player_frame: env order and per-env costs
    long pf_launches = 0;
    DevBuf<uint32_t> gv_order, gv_cost;   // global_view: env order and per-env costs
    long gv_launches = 0;
};

// autotuner of the step-kernel build variant (npp_kernels.hip: VariantK): windows of TUNE_WINDOW launches per variant, timed
// with one pair of HIP events each (never synchronised: the decision is taken once the last event has completed)
struct Tuner {
    int pin = -1;        // -1 = autotune
    int variant = 0;     // what npp_step launches now
    int state = 0;       // 0 = warm-up, 1 .. TUNE_ROUNDS * 3 = measuring windows, > that = waiting for events / decided
    int count = 0;       // launches inside the current state
    bool tuned = false;
    long since = 0;      // launches since the last decision
    std::vector<Event> ev;   // one (start, end) pair per measured launch: 2 * TUNE_WINDOW * windows
    // a new level set / assignment / geometry / stream: the warm-up also lets the heavy-first order settle
    void restart() { state = 0; count = 0; tuned = pin >= 0; variant = pin >= 0 ? pin : 0; }
};

// observation overlap (npp_set_obs_overlap / npp_set_obs_overlap_parts): npp_step cuts its heavy-first workgroup order at
// cut_pct[] percent and launches every piece ("part") as a kernel of its own -- part 0, the cheap tail of the order, on the
// caller's stream, the others on part_stream[] -- and while live_parts > 1 every observation entry point launches one kernel per
// part on the stream of the part it reads, so the observations of the cheap envs are produced while the expensive envs are still
// stepping.  join_streams() makes the caller's stream wait for the others.
struct Overlap {
    int n_cuts = 0;               // 0 = off
    int cut_pct[3] = {0, 0, 0};   // ascending, from the head (most expensive end) of the order
    int live_parts = 1;           // parts of the last npp_step still to be joined (1 = it was not split)
    bool phase_dirty = true;      // phase does not describe the current order / cuts
    DevBuf<uint8_t> phase;        // [n] which part steps the env (npp_phase_kernel, rewritten when the order or the cuts change)
    hipStream_t part_stream[4] = {nullptr, nullptr, nullptr, nullptr};   // part 0 = the cheap tail of the order, on the caller's stream
    // the streams behind part_stream[1..] and side[]: created by calibrate_streams(), which keeps only streams whose kernels were
    // SEEN to run beside the caller's and beside each other (HIP spreads a process's streams over four hardware queues; two streams
    // on one queue serialise, and which queue a new stream gets depends on every stream the process has created before)
    std::vector<Stream> owned;
    hipStream_t owned_for = nullptr;   // the caller's stream they were chosen against
    bool owned_valid = false;
    Event cal_ev[2];
    Event part_ev[4];   // join
    Event ov_ev[2];     // fork / tables on the caller's stream ready
    // ... and with two parts player_frame need not wait for the other observation kernels either: it runs on side[p], forked off
    // the stream that stepped part p.  Measured (doors, full Dict, two parts cut at 40 %): no side stream 471 us per step,
    // global_view aside 485, player_frame aside 436, both 555 -- HIP feeds a process through four hardware queues, so more
    // streams than that share queues and serialise again
    hipStream_t side[2] = {nullptr, nullptr};
    Event side_ev[2];   // fork, then reused for the join
    bool side_busy[2] = {false, false};
};

// frame stacking (npp_set_frame_stack / npp_frame_stack_push, npp_stack.hip): one ring of 2 K slots per env and stacked key
struct FrameStack {
    int vk = 0, sk = 0, repeat = 0;   // stack sizes (0 = off) and padding
    int vhead = 0, shead = 0;         // ring position of the newest entry
    DevBuf<uint8_t> frames;           // [n][2 vk][84 * 84]
    DevBuf<float> state;              // [n][2 sk][41]
};

// level pool (npp_set_level_pool, npp_pool.hip): with it on, the device changes env_level / trunc after a step, and the host
// mirrors are read back lazily (pull_levels) where a host path needs them
struct Pool {
    bool on = false;
    bool ever = false;    // a pool was on since npp_load_levels: levels change without npp_assign_levels, snapshots carry them
    bool dirty = false;   // the device may have drawn since env_level / trunc were read back
    uint64_t seed = 0;
    int last = 0;         // the last level of non-zero weight
    std::vector<double> w;
    DevBuf<uint8_t> flags;     // [n] step flags when the caller asked for none
    DevBuf<uint8_t> changed;   // [n] envs that drew another level (device reset / observe mask)
};

// goal curriculum (npp_set_goal_curriculum; the rule: npp_goal.hpp, the kernels: npp_goal.hip): with it on, the device changes
// env_level after a step as the level pool does, and shares the pool's changed mask and flags row
struct Goal {
    bool on = false;
    NppGoalCurriculumParams params{100.0, 0.80, 500, 1};
    int ring_words = 0, need = 0;
    std::vector<GoalStages> stages;            // [n_base]
    std::vector<int32_t> base_of, stage_of;    // [n_levels]
    std::vector<int32_t> variant0;             // [n_base]
    std::vector<double> all;                   // [n_levels] of 1.0: make_plan's "any level an env may play"
    DevBuf<int32_t> lv, env, d_base_of, d_stage_of, list;
    DevBuf<uint32_t> ring;
};

// evaluation sweep (npp_sweep_start; the rule: npp_sweep.hpp, the kernels: npp_sweep.hip): with it on, the device changes env_level /
// trunc after a step as the level pool does, and shares the pool's changed mask and flags row.  Allocated by npp_sweep_start; the
// result planes outlive npp_sweep_stop (npp_sweep_view) and go with the next start or level set.
struct Sweep {
    bool on = false;
    int n_jobs = 0;
    std::vector<double> w;                     // [n_levels] 1.0 for a level some job names: make_plan's "any level an env may play"
    DevBuf<int32_t> jobs, counters, env_job, prev_job, res_i32;
    DevBuf<double> res_f64;
};

// minimal observation (npp_set_minimal_observation / npp_minimal_observation): its mine columns are read from the spatial_context
// rows of the step kernel, so with the mode on every step / observe launch writes them -- into the caller's d_spatial_context, or
// into `sc` when the caller's npp_step_out has none
struct Minimal {
    bool on = false;
    DevBuf<float> sc;            // [n][112], allocated by the first launch that needs it
    const float *rows = nullptr; // where the last step / observe launch wrote the rows (the caller's buffer or `sc`)
};

// frame augmentation (npp_set_frame_augmentation / npp_frame_augment, npp_augment.hip): augmented copies of the player_frame
// window and of global_view in buffers of the handle; the sources are where the render entries last wrote
struct FrameAug {
    bool on = false;
    double p = 0.0;
    int s10 = 10;                // intensity scale * 10
    uint64_t seed = 0;
    uint32_t count = 0;          // augmentation calls since npp_set_frame_augmentation (observation noise: not in the snapshot)
    int k = 1;                   // player_frame entries per env of `pf` (the visual stack size it was allocated for, or 1)
    DevBuf<uint8_t> pf, gv;      // [n][k][84 * 84], [n][176 * 100]
    DevBuf<int32_t> params;      // [n][2][AUG_WORDS] a caller's parameters, allocated by the first call that brings some
    const uint8_t *pf_out = nullptr, *gv_out = nullptr;   // d_out of the last npp_render_player_frame / npp_render_global_view
};

// checkpoint archive (npp_archive_create, npp_archive.hip): n_slots records of one env's state each, plus a meta row per slot.
// Sized by the loaded level set, dropped with it.
struct Archive {
    int n_slots = 0;              // 0 = none
    ArchiveLayout lay;
    DevBuf<uint32_t> rec;         // [n_slots][lay.words]
    DevBuf<double> meta_f64;      // [n_slots][ARCHIVE_META_F64]
    DevBuf<int32_t> meta_i32;     // [n_slots][ARCHIVE_META_I32], word 0 = the slot holds a record
};

// cell index over the checkpoint archive (npp_archive_cells_create, npp_cells.hip): per-(level, switch, cell) tables; while it
// exists it owns every slot of the archive.  Sized by the loaded level set and the archive, dropped with either.
struct Cells {
    bool on = false;
    uint64_t seed = 0;
    uint32_t call = 0;                    // select calls since npp_archive_cells_create
    DevBuf<unsigned long long> best, cdf;   // [K], K = n_levels * NPP_CELLS_PER_LEVEL
    DevBuf<int32_t> cell_slot;            // [K]
    DevBuf<float> cell_score;             // [K]
    DevBuf<uint32_t> visits, chosen;      // [K]
    DevBuf<int32_t> slot_key;             // [n_slots]
    DevBuf<int32_t> n_used;               // [1]
    DevBuf<int32_t> env_key, slot_of_env, iota;   // [n]
};

// action routes (npp_set_routes, npp_route.hip): per env a header and two action buffers; the archive's and the snapshot's records
// carry the current route while this is on (record_layout)
struct Routes {
    int cap = 0;                  // bytes per buffer, a multiple of 16; 0 = off
    DevBuf<int32_t> hdr;          // [n][ROUTE_HDR_WORDS]
    DevBuf<uint8_t> act;          // [n][2][cap]
    // the step's flags / frames rows when the caller asked for none (as Pool::flags), grown to the longest npp_step_many seen
    DevBuf<uint8_t> flags;        // [rows][n]
    DevBuf<uint16_t> frames;      // [rows][n]
    int rows = 0;
};

// episode statistics (npp_set_episode_stats / npp_episode_accumulate, npp_episode.hip): per-env record planes and the per-level table.
// Allocated when switched on; dropped by npp_load_levels (the table has a row per level of the set).
struct Episode {
    bool on = false;
    int n_levels = 0;
    DevBuf<int32_t> i32;                 // [EP_NI][n]
    DevBuf<double> f64;                  // [EP_ND][n]
    DevBuf<unsigned long long> table;    // [n_levels][EP_COLS]
    DevBuf<int32_t> restore_status;      // status row of an npp_archive_restore whose caller asked for none (only restored envs restart)
    size_t restore_cap = 0;
};

// path-direction action masking (npp_set_action_masking / npp_path_action_mask, npp_pathmask.hip): the mode, the per-env counters
// and where the last step wrote its flags row.  Allocated by the first call that switches a mode on, kept for the handle's life.
struct PathMask {
    int mode = 0;                        // 0 off, 1 hard, 2 soft
    DevBuf<uint32_t> counters;           // [4][n] observed | applied | last_observed | last_applied
    DevBuf<uint8_t> flagbuf;             // [n] the step's flags row when the caller asked for none (as Pool::flags)
    const uint8_t *flags = nullptr;      // flags row of the last npp_step not yet consumed by npp_path_action_mask
    uint32_t *plane(int k, int n) const { return counters.get() + (size_t)k * n; }
};

// reward mode "pbrs" (npp_set_reward_mode / npp_step_reward, npp_reward.hip): the mode, the parameters, the levels' constants, the
// per-env state planes and where the last step wrote its flags and frames rows.  Allocated when the mode is switched on; dropped by
// npp_load_levels (the constants belong to the level set).
struct Reward {
    int mode = 0;                        // 0 sparse, 1 pbrs
    NppRewardParams params{};
    DevBuf<RewardLevel> levels;          // [n_levels]
    DevBuf<double> sd;                   // [RW_ND][n]
    DevBuf<uint32_t> si;                 // [RW_NI][n]
    DevBuf<uint32_t> stamp2;             // [n][REACH_CELLS] the fallback query's dictionary (levels with ReachHdr::miss_exit only)
    DevBuf<double> raw2;
    DevBuf<uint8_t> flagbuf;             // [n] the step's flags row when the caller asked for none
    DevBuf<uint16_t> framebuf;           // [n] likewise the frames row
    DevBuf<int32_t> restore_status;      // status row of an npp_archive_restore whose caller asked for none (only restored envs restart)
    size_t restore_cap = 0;
    const uint8_t *flags = nullptr;      // rows of the last npp_step not yet consumed by npp_step_reward
    const uint16_t *frames = nullptr;
    // the sequential path waypoints (npp_set_reward_waypoints, npp_waypoint.hip): allocated when they are switched on
    int wp_on = 0;
    NppWaypointParams wp_params{};
    DevBuf<WaypointHdr> wp_hdr;          // [n_levels]
    DevBuf<unsigned char> wp_blob;
    DevBuf<uint32_t> wp_state;           // [WP_NI][n]
    DevBuf<double> wp_bonus;             // [n] the step's bonus, from npp_waypoint_kernel to npp_reward_kernel
    std::vector<std::vector<uint32_t>> wp_rec;   // host copy of the levels' records (npp_reward_waypoints)
};

// demonstration player (npp_demo_create / npp_demo_play, npp_demo.hip): the ragged input table and the plan on the device, the
// staging rows npp_tick reads and one observation row per env for the existing observation launches to write.  Dropped by
// npp_load_levels (its level ids belong to the set).
struct Demo {
    bool on = false;
    int n_replays = 0, fs = 1;
    unsigned keys = 0;
    DemoPlan plan;
    std::vector<int32_t> levels;          // [n_replays]
    DevBuf<uint8_t> inputs;               // the ragged table
    DevBuf<int64_t> offsets, row_base;    // [n_replays + 1], [n_replays]
    DevBuf<int32_t> rows, rep_level;      // [n_replays]
    DevBuf<int32_t> slot;                 // [n_rounds][n] the replay of env e in round q, -1 = none
    DevBuf<uint8_t> staging;              // [fs][n]
    DevBuf<float> gs, epos, sc, reach, sdf, sw;   // the observation rows, one per env (allocated for the keys that are on)
    DevBuf<int8_t> mask;
    DevBuf<uint8_t> flags;
    DevBuf<double> pos;
    DevBuf<int32_t> rstatus;
};

// the launch plan (plan_geometry)
struct Plan {
    int g = 1, wpb = 1;         // lanes per env, wavefronts per workgroup
    uint32_t lds_hot_cap = 0;   // LDS bytes reserved for a staged level
    int zoo_active = 0;         // some env may play a level with zoo entities (or has one repositioned)
    int lds_level = 0;          // all workgroups level-uniform and staged levels fit
};

}  // namespace

struct npp_handle_s {
    int n = 0, device = 0;
    unsigned flags = 0;
    hipStream_t stream = nullptr;   // the caller's
    std::string err;
    std::vector<int32_t> env_level, trunc;   // host mirrors of env.level / env.trunc
    bool dyn_trunc = false;           // npp_set_dynamic_truncation: per-level limit from the reachable surface area
    std::vector<uint8_t> ovr;         // per env: ZOO_OVR_* flags set through npp_set_entity_pos
    int n_ovr = 0;
    unsigned long long assign_gen = 0;
    int lanes_per_env = 0, waves_per_block = 0;   // npp_set_launch_geometry (0 = choose)
    Plan plan;
    EnvState env;
    LevelSet ls;
    Snapshot snap;
    Orders ord;
    Tuner tune;
    Overlap ov;
    FrameStack fs;
    Pool pool;
    Minimal mini;
    FrameAug aug;
    Archive ar;
    Cells cells;
    Routes rt;
    PathMask pm;
    Reward rw;
    Demo demo;
    Episode ep;
    Goal goal;
    Sweep sweep;
};


namespace {

constexpr uint32_t LDS_BUDGET = 64 * 1024;  // per workgroup (160 KiB per CU: at least two workgroups per CU)

int fail(npp_handle h, int code, const std::string &msg) {
    if (h) h->err = msg; else host_error() = msg;
    return code;
}

#define HIP_TRY(h, expr)                                                                              \
    do {                                                                                              \
        hipError_t _e = (expr);                                                                       \
        if (_e != hipSuccess) return fail(h, NPP_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(_e)); \
    } while (0)

uint32_t align_up(uint32_t v, uint32_t a) { return (v + a - 1) / a * a; }

// observation overlap: the caller's stream waits for everything the other streams were given since the last split step
hipError_t join_streams(npp_handle h) {
    Overlap &ov = h->ov;
    hipError_t e = hipSuccess;
    for (int p = 0; p < 2; p++)
        if (ov.side_busy[p]) {
            ov.side_busy[p] = false;
            if (e == hipSuccess) e = hipEventRecord(ov.side_ev[p].get(), ov.side[p]);
            if (e == hipSuccess) e = hipStreamWaitEvent(h->stream, ov.side_ev[p].get(), 0);
        }
    for (int p = 0; p < ov.live_parts && ov.live_parts > 1; p++) {
        if (ov.part_stream[p] == h->stream) continue;
        if (e == hipSuccess) e = hipEventRecord(ov.part_ev[p].get(), ov.part_stream[p]);
        if (e == hipSuccess) e = hipStreamWaitEvent(h->stream, ov.part_ev[p].get(), 0);
    }
    ov.live_parts = 1;
    return e;
}
// the stream an observation kernel of part `part` is launched on: the part's own stream, or (player_frame, two parts only) a side
// stream forked off it here.  `tables`: the caller's stream holds work the kernel needs (order tables) -- other streams wait for that.
hipError_t obs_stream(npp_handle h, bool player_frame, int part, bool tables, hipStream_t *out) {
    Overlap &ov = h->ov;
    hipStream_t dst = ov.part_stream[part];
    hipError_t e = hipSuccess;
    if (player_frame && ov.n_cuts == 1 && ov.side[part] != nullptr) {
        if (!ov.side_busy[part]) {   // (a second call before the join just queues behind the first)
            e = hipEventRecord(ov.side_ev[part].get(), dst);
            if (e == hipSuccess) e = hipStreamWaitEvent(ov.side[part], ov.side_ev[part].get(), 0);
            ov.side_busy[part] = true;
        }
        dst = ov.side[part];
    }
    if (e == hipSuccess && tables && dst != h->stream) {
        e = hipEventRecord(ov.ov_ev[1].get(), h->stream);
        if (e == hipSuccess) e = hipStreamWaitEvent(dst, ov.ov_ev[1].get(), 0);
    }
    *out = dst;
    return e;
}

// Do kernels on streams a and b run side by side?  Two idle wavefronts of `ticks` each, one per stream: b's ends about when a's
// does, or a whole kernel later.  (Setup path: synchronises both streams.)
bool streams_overlap(npp_handle h, hipStream_t a, hipStream_t b, long long ticks, float single_ms) {
    if (hipStreamSynchronize(a) != hipSuccess || hipStreamSynchronize(b) != hipSuccess) return true;
    bool ok = hipEventRecord(h->ov.cal_ev[0].get(), a) == hipSuccess;
    ok = ok && launch_spin(ticks, a) == hipSuccess && launch_spin(ticks, b) == hipSuccess;
    ok = ok && hipEventRecord(h->ov.cal_ev[1].get(), b) == hipSuccess;
    ok = ok && hipStreamSynchronize(a) == hipSuccess && hipStreamSynchronize(b) == hipSuccess;
    float ms = 0.f;
    if (!ok || hipEventElapsedTime(&ms, h->ov.cal_ev[0].get(), h->ov.cal_ev[1].get()) != hipSuccess) return true;   // cannot tell: take the stream
    return ms < 1.6f * single_ms;
}

// `need` streams of the handle's own that overlap with the caller's stream and with each other (see Overlap::owned); when fewer
// can be found among 12 candidates the rest are streams that do not -- slower, never wrong.
int calibrate_streams(npp_handle h, int need) {
    Overlap &ov = h->ov;
    if (ov.owned_valid && ov.owned_for == h->stream && (int)ov.owned.size() >= need) return NPP_OK;
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    ov.owned.clear();
    if (!ov.cal_ev[0]) {
        HIP_TRY(h, ov.cal_ev[0].create(hipEventDefault));
        HIP_TRY(h, ov.cal_ev[1].create(hipEventDefault));
    }
    const long long ticks = 3000;   // 30 us of the 100 MHz wall clock
    float single_ms = 0.03f;
    {   // what one such kernel takes between two events on one stream (launch overhead included)
        launch_spin(ticks, h->stream);   // warm: the code object
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        HIP_TRY(h, hipEventRecord(ov.cal_ev[0].get(), h->stream));
        HIP_TRY(h, launch_spin(ticks, h->stream));
        HIP_TRY(h, hipEventRecord(ov.cal_ev[1].get(), h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, ov.cal_ev[0].get(), ov.cal_ev[1].get()) == hipSuccess && ms > 0.f) single_ms = ms;
    }
    std::vector<Stream> rejected;
    for (int c = 0; c < 12 && (int)ov.owned.size() < need; c++) {
        Stream st;
        HIP_TRY(h, st.create(hipStreamNonBlocking));
        bool ok = streams_overlap(h, h->stream, st.get(), ticks, single_ms);
        for (size_t i = 0; ok && i < ov.owned.size(); i++) ok = streams_overlap(h, ov.owned[i].get(), st.get(), ticks, single_ms);
        (ok ? ov.owned : rejected).push_back(std::move(st));   // a rejected stream stays alive until the search ends: it keeps its queue busy
    }
    while ((int)ov.owned.size() < need && !rejected.empty()) { ov.owned.push_back(std::move(rejected.back())); rejected.pop_back(); }
    rejected.clear();
    while ((int)ov.owned.size() < need) {
        Stream st;
        HIP_TRY(h, st.create(hipStreamNonBlocking));
        ov.owned.push_back(std::move(st));
    }
    ov.owned_for = h->stream;
    ov.owned_valid = true;
    // hand them out: the parts first, then (two parts only) the side streams
    int k = 0;
    // the cheap tail of the order rides on the caller's stream: that stream also carries the order-table kernels the other
    // streams wait for, and behind the most expensive part they would come a whole step late (measured: 520 us per step
    // instead of 440, doors, full Dict)
    for (int q = 0; q <= ov.n_cuts; q++) ov.part_stream[q] = q == 0 ? h->stream : ov.owned[k++].get();
    for (int q = 0; q < 2; q++) ov.side[q] = ov.n_cuts == 1 ? ov.owned[k++].get() : nullptr;
    return NPP_OK;
}
int streams_needed(npp_handle h) { return h->ov.n_cuts + (h->ov.n_cuts == 1 ? 2 : 0); }

// One observation kernel: as it is on the caller's stream (overlap off), or once per part of the last split step, the most
// expensive part first, each launch told which part's envs are its own.
template <class F> int obs_launch(npp_handle h, KernelArgs a, bool player_frame, bool tables, F &&launch) {
    if (h->ov.live_parts <= 1) {   // overlap off, or the last step was not split
        HIP_TRY(h, launch(a, h->stream));
        return NPP_OK;
    }
    hipStream_t st = h->stream;
    a.phase = h->ov.phase.get();
    for (int q = h->ov.live_parts - 1; q >= 0; q--) {
        HIP_TRY(h, obs_stream(h, player_frame, q, tables, &st));
        a.phase_id = q;
        HIP_TRY(h, launch(a, st));
    }
    return NPP_OK;
}

// Every entry point that launches, copies or allocates runs with the HANDLE's device current and puts the caller's device
// back afterwards: a caller whose current device differs (another handle, another framework) must neither receive our
// launch on its GPU nor find its own current device changed.
struct DeviceGuard {
    int prev = -1;
    hipError_t err = hipSuccess;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) err = hipSetDevice(dev); else prev = -1;
    }
    ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
    DeviceGuard(const DeviceGuard &) = delete;
    DeviceGuard &operator=(const DeviceGuard &) = delete;
};
#define ON_DEVICE(h)                                                                                          \
    DeviceGuard _dg((h)->device);                                                                             \
    if (_dg.err != hipSuccess) return fail(h, NPP_ERR_HIP, std::string("hipSetDevice: ") + hipGetErrorString(_dg.err))
// every entry point but the observation kernels themselves first joins the two streams of a split step (see npp_set_obs_overlap)
#define ON_DEVICE_JOINED(h)                                                                                   \
    ON_DEVICE(h);                                                                                             \
    HIP_TRY(h, join_streams(h))

// Launch geometry (DESIGN.md "lanes per environment"): G lanes cooperate on one env.  The chip has 256 CUs x 4 SIMDs;
// the path is a latency-bound fp64 dependency chain, so the grid is sized to put about two wavefronts on every SIMD
// (one hides the other's latency) and the spare lanes of each wavefront are spent on segment-level parallelism.
// The plan for n envs playing `level` of set L; `any_ovr`: some exit switch / door is repositioned; `pool`: the weights of the
// level pool when it is on.
Plan make_plan(const LevelSet &L, int n, const std::vector<int32_t> &level, int lanes_per_env, int waves_per_block, bool any_ovr,
               const std::vector<double> *pool) {
    Plan p;
    int g = lanes_per_env;
    if (g <= 0) {
        // measured on MI355X (tools/sweep_geometry.py, tools/big_batch_probe.py): 16 lanes per env up to 16 384 envs, 8 at
        // 32 768, 4 from 65 536 on (95.8 M env-steps/s there; 2 lanes per env is 2.5x slower at any size)
        g = 16;
        while (g > 4 && (long long)n * g / 64 > 4096) g >>= 1;
    }
    int gg = 1;
    while (gg * 2 <= g && gg < 64) gg *= 2;
    g = gg;
    int wpb = waves_per_block;
    if (wpb <= 0) wpb = 4;
    if (wpb > 4) wpb = 4;
    while (wpb > 1 && (64 / g) * wpb > n) wpb >>= 1;
    p.zoo_active = any_ovr ? 1 : 0;   // repositioned switches / doors are handled by the zoo kernel's merged walk
    if (!L.levels.empty())
        for (int e = 0; e < n && !p.zoo_active; e++) p.zoo_active = L.levels[level[e]].has_zoo ? 1 : 0;
    if (pool)   // (level pool) any level an env may draw
        for (size_t l = 0; l < pool->size() && !p.zoo_active; l++) p.zoo_active = (*pool)[l] > 0.0 && L.levels[l].has_zoo ? 1 : 0;
    const int zw = p.zoo_active ? L.zoo_words : 0;
    // LDS plan: staged level + entity words + observation staging (+ zoo blocks) must fit the per-workgroup budget
    for (;;) {
        int epb = (64 / g) * wpb;
        uint32_t fixed = (uint32_t)lds_bytes(0, L.n_words_max, epb, zw);
        if (fixed > LDS_BUDGET) {
            if (wpb > 1) { wpb >>= 1; continue; }
            if (g < 64) { g *= 2; continue; }   // zoo blocks are big: fewer envs per wavefront
        }
        uint32_t cap = L.hot_max;
        if (zw && fixed + cap > LDS_BUDGET && wpb > 1) { wpb >>= 1; continue; }   // zoo: staging the level beats a bigger workgroup
        if (fixed + cap > LDS_BUDGET) cap = fixed < LDS_BUDGET ? ((LDS_BUDGET - fixed) / 16) * 16 : 0;
        p.lds_hot_cap = cap;
        break;
    }
    p.g = g;
    p.wpb = wpb;
    // can every workgroup stage ONE level?  (the host owns the env -> level assignment)
    int epb = (64 / g) * wpb;
    int ok = !L.hdrs.empty() && !pool;   // (level pool: levels change on the device, workgroups no longer share one)
    for (int b0 = 0; b0 < n && ok; b0 += epb) {
        int lvl = level[b0];
        if (L.hdrs[lvl].hot_bytes > p.lds_hot_cap) ok = 0;
        for (int e = b0 + 1; e < b0 + epb && e < n && ok; e++)
            if (level[e] != lvl) ok = 0;
    }
    p.lds_level = ok;
    return p;
}

int pull_levels(npp_handle h);

void plan_geometry(npp_handle h, bool keep_tuning = false) {
    (void)pull_levels(h);   // (a failure leaves the mirror as it was and is reported by the next call that syncs)
    const Plan p = make_plan(h->ls, h->n, h->env_level, h->lanes_per_env, h->waves_per_block, h->n_ovr > 0,
                             h->pool.on ? &h->pool.w : (h->goal.on ? &h->goal.all : (h->sweep.on ? &h->sweep.w : nullptr)));
    // a new plan (level set, assignment, geometry, zoo kernels on / off) restarts npp_step's variant autotuner; a plan that comes
    // out the same (npp_restore of a snapshot with the same overrides) keeps the decision
    const bool same_plan = keep_tuning && p.g == h->plan.g && p.wpb == h->plan.wpb && p.zoo_active == h->plan.zoo_active;
    h->plan = p;
    if (!same_plan) h->tune.restart();
}

KernelArgs base_args(npp_handle h) {
    const LevelSet &L = h->ls;
    KernelArgs a;
    std::memset(&a, 0, sizeof(a));
    a.f64 = h->env.f64.get();
    a.u32 = h->env.u32.get();
    a.ent_bits = L.ent.get();
    a.sc_cache = h->env.sc.get();
    a.env_level = h->env.level.get();
    a.trunc_limit = h->env.trunc.get();
    a.hdr = L.hdr.get();
    a.blob = L.blob.get();
    a.tile_canvas = L.canvas.get();
    a.n = h->n;
    a.autoreset = (h->flags & NPP_FLAG_AUTORESET) ? 1 : 0;
    a.fast_reset = (h->flags & NPP_FLAG_FAST_RESET) ? 1 : 0;   // in-kernel auto-resets
    a.n_words_max = L.n_words_max;
    a.lds_hot_cap = h->plan.lds_hot_cap;
    a.lanes_per_env = h->plan.g;
    a.waves_per_block = h->plan.wpb;
    a.lds_level = h->plan.lds_level;
    a.zoo = L.zoo.get();
    a.zoo_words = L.zoo_words;
    a.zoo_doors = L.zoo_doors;
    a.zoo_movers = L.zoo_movers;
    a.zoo_active = h->plan.zoo_active;
    a.variant = (h->plan.g == 16 && !h->plan.zoo_active) ? h->tune.variant : 0;   // npp_step's autotuner (or the pinned build)
    return a;
}

void fill_out(KernelArgs &a, const npp_step_out *o) {
    if (!o) return;
    a.out.game_state = o->d_game_state;
    a.out.action_mask = o->d_action_mask;
    a.out.entity_pos = o->d_entity_pos;
    a.out.flags = o->d_flags;
    a.out.reward = o->d_reward;
    a.out.frames = o->d_frames;
    a.out.terminal_state = o->d_terminal_state;
    a.out.spatial_context = o->d_spatial_context;
    a.out.positions = o->d_positions;
    a.out.work = o->d_work;
}

// fill_out for the launches that produce an observation (step, step_many, observe, the level pool's masked observe): with the
// minimal observation on, a launch whose caller asked for no spatial_context writes the rows into the handle's own buffer
int fill_obs_out(npp_handle h, KernelArgs &a, const npp_step_out *o) {
    fill_out(a, o);
    Minimal &m = h->mini;
    if (!m.on) return NPP_OK;
    if (!a.out.spatial_context) {
        if (!m.sc) {
            HIP_TRY(h, m.sc.alloc((size_t)h->n * NPP_SPATIAL_CONTEXT_DIM));
            HIP_TRY(h, hipMemsetAsync(m.sc.get(), 0, m.sc.bytes(), h->stream));
        }
        a.out.spatial_context = m.sc.get();
    }
    m.rows = a.out.spatial_context;
    return NPP_OK;
}

// The render kernels read the tile layer from a per-level coverage canvas (npp_render.hip); it is built the first time a
// frame is asked for, so handles that never render pay neither the memory (633 600 B per level) nor the kernel.
int ensure_canvas(npp_handle h) {
    LevelSet &L = h->ls;
    if (L.canvas) return NPP_OK;
    HIP_TRY(h, L.canvas.alloc(L.levels.size() * 600 * 1056, 16));   // + 16: rows are read as aligned dword pairs
    HIP_TRY(h, launch_tile_tables(h->stream));   // idempotent: every handle of a device writes the same bytes
    HIP_TRY(h, launch_tile_canvas(L.hdr.get(), L.blob.get(), L.canvas.get(), (int)L.levels.size(), h->stream));
    return NPP_OK;
}

int ensure_gv(npp_handle h) {
    if (int rc = ensure_canvas(h)) return rc;
    if (h->ls.gv.h) return NPP_OK;
    const size_t nl = h->ls.levels.size();
    GvTables t;   // complete or not at all: a failure leaves nothing behind and the next call starts over
    HIP_TRY(h, t.v.alloc(nl * 176 * 100));
    HIP_TRY(h, t.p.alloc(nl * 600 * 1056, 16));   // + 16: row slices are read as four aligned dwords
    HIP_TRY(h, t.h.alloc(nl * 600 * 100));
    HIP_TRY(h, launch_gv_static(base_args(h), (int)nl, t.p.get(), t.h.get(), t.v.get(), h->stream));
    h->ls.gv = std::move(t);
    Orders &o = h->ord;
    if (!o.gv_order) {
        HIP_TRY(h, o.gv_order.alloc(h->n));
        HIP_TRY(h, o.gv_cost.alloc(h->n));
        HIP_TRY(h, hipMemsetAsync(o.gv_cost.get(), 0, o.gv_cost.bytes(), h->stream));
        o.gv_launches = 0;   // the first launch builds an order (any permutation) from the zero costs
    }
    return NPP_OK;
}

// The reachability tables (npp_reach.cpp) are built the first time the observation is asked for: ~1 ms of host work and
// ~260 KB of HBM per level, which handles that never ask for it do not pay.
// `keep` (may be null): receives every level's ReachBuilt when the tables are built by this call (left empty when they existed)
int ensure_reach(npp_handle h, std::vector<ReachBuilt> *keep = nullptr) {
    if (h->ls.reach.hdr) return NPP_OK;
    const size_t N = (size_t)h->n, nl = h->ls.levels.size();
    std::vector<ReachHdr> hdrs(nl);
    std::vector<unsigned char> blob;
    bool any_miss = false;
    std::vector<ReachBuilt> local(keep ? nl : 1);
    for (size_t i = 0; i < nl; i++) {
        ReachBuilt &R = local[keep ? i : 0];
        build_reach(h->ls.levels[i], R);
        if (!R.hdr.supported)
            return fail(h, NPP_ERR_UNSUPPORTED, "npp_reachability: level " + std::to_string(i) + ": " + R.note +
                                                    " (outside the restated part of the reference's reachability code, see DESIGN.md)");
        any_miss = any_miss || R.hdr.miss_exit;
        pack_reach(R, hdrs[i], blob);
    }
    Reach r;   // complete or not at all: a failed allocation / copy leaves nothing behind
    HIP_TRY(h, r.blob.alloc(blob.size(), 16));
    HIP_TRY(h, hipMemcpy(r.blob.get(), blob.data(), blob.size(), hipMemcpyHostToDevice));
    HIP_TRY(h, r.key.alloc(N));
    HIP_TRY(h, hipMemset(r.key.get(), 0, r.key.bytes()));
    HIP_TRY(h, r.cache.alloc((REACH_DIM + 1) * N));
    HIP_TRY(h, hipMemset(r.cache.get(), 0, r.cache.bytes()));
    if (any_miss) {   // 13.2 KB per env: 108 MB at 8192 envs
        HIP_TRY(h, r.stamp.alloc(REACH_CELLS * N));
        HIP_TRY(h, hipMemset(r.stamp.get(), 0, r.stamp.bytes()));
        HIP_TRY(h, r.raw.alloc(REACH_CELLS * N));
        HIP_TRY(h, r.epoch.alloc(N));
        HIP_TRY(h, hipMemset(r.epoch.get(), 0, r.epoch.bytes()));
        HIP_TRY(h, r.last_episode.alloc(N));
        HIP_TRY(h, hipMemset(r.last_episode.get(), 0xff, r.last_episode.bytes()));
    }
    HIP_TRY(h, r.hdr.alloc(nl));
    HIP_TRY(h, hipMemcpy(r.hdr.get(), hdrs.data(), r.hdr.bytes(), hipMemcpyHostToDevice));
    h->ls.reach = std::move(r);
    if (keep) *keep = std::move(local);
    return NPP_OK;
}

// The graph observation tables (npp_graph.cpp) likewise, at the first npp_graph_observation: at most ~140 KB of HBM per level
int ensure_graph(npp_handle h) {
    if (h->ls.graph.hdr) return NPP_OK;
    const size_t nl = h->ls.levels.size();
    std::vector<GraphHdr> hdrs(nl);
    std::vector<unsigned char> blob;
    for (size_t i = 0; i < nl; i++) {
        GraphBuilt G;
        build_graph_obs(h->ls.levels[i], G);
        pack_graph_obs(G, hdrs[i], blob);
    }
    GraphObs g;   // complete or not at all
    HIP_TRY(h, g.blob.alloc(blob.size()));
    HIP_TRY(h, hipMemcpy(g.blob.get(), blob.data(), blob.size(), hipMemcpyHostToDevice));
    HIP_TRY(h, g.row_level.alloc((size_t)h->n));
    HIP_TRY(h, hipMemset(g.row_level.get(), 0xff, g.row_level.bytes()));
    HIP_TRY(h, g.hdr.alloc(nl));
    HIP_TRY(h, hipMemcpy(g.hdr.get(), hdrs.data(), g.hdr.bytes(), hipMemcpyHostToDevice));
    h->ls.graph = std::move(g);
    return NPP_OK;
}

// level pool: read the device's env_level / trunc back into the host mirrors (synchronises; only after a draw)
int pull_levels(npp_handle h) {
    if (!h->pool.dirty) return NPP_OK;
    HIP_TRY(h, join_streams(h));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    HIP_TRY(h, hipMemcpy(h->env_level.data(), h->env.level.get(), h->env.level.bytes(), hipMemcpyDeviceToHost));
    HIP_TRY(h, hipMemcpy(h->trunc.data(), h->env.trunc.get(), h->env.trunc.bytes(), hipMemcpyDeviceToHost));
    h->pool.dirty = false;
    return NPP_OK;
}

void level_trunc_table(npp_handle h) {
    LevelSet &L = h->ls;
    if (L.level_trunc.size() == L.levels.size()) return;
    L.level_trunc.resize(L.levels.size());
    for (size_t i = 0; i < L.levels.size(); i++) {
        ReachBuilt R;
        build_reach(L.levels[i], R);
        L.level_trunc[i] = truncation_limit_for_area(R.spawn_area);
    }
}

// level pool + dynamic truncation: the per-level limits on the device, for the draw kernel
int upload_level_trunc(npp_handle h) {
    LevelSet &L = h->ls;
    level_trunc_table(h);
    if (!L.d_level_trunc) HIP_TRY(h, L.d_level_trunc.alloc(L.levels.size()));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    HIP_TRY(h, hipMemcpy(L.d_level_trunc.get(), L.level_trunc.data(), L.d_level_trunc.bytes(), hipMemcpyHostToDevice));
    return NPP_OK;
}

// envs selected by mask (NULL = all) take their level's dynamic limit
int apply_dynamic_truncation(npp_handle h, const uint8_t *mask) {
    if (int rc = pull_levels(h)) return rc;
    level_trunc_table(h);
    for (int e = 0; e < h->n; e++)
        if (!mask || mask[e]) h->trunc[e] = h->ls.level_trunc[h->env_level[e]];
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    HIP_TRY(h, hipMemcpy(h->env.trunc.get(), h->trunc.data(), h->env.trunc.bytes(), hipMemcpyHostToDevice));
    return NPP_OK;
}

// ---- action routes (npp_set_routes; the rule: npp_route.hpp, the kernels: npp_route.hip).  Nothing below launches or allocates
// while they are off.
RouteArgs route_args(npp_handle h) {
    RouteArgs r{};
    r.n = h->n;
    r.cap = h->rt.cap;
    r.hdr = h->rt.hdr.get();
    r.act = h->rt.act.get();
    r.env_level = h->env.level.get();
    r.autoreset = (h->flags & NPP_FLAG_AUTORESET) ? 1 : 0;
    return r;
}

// a reset (ROUTE_EV_FLIP), raw ticks (ROUTE_EV_TICK) or a new level set (ROUTE_EV_INIT) for the envs of a device mask (null = all),
// on the caller's stream; the caller has joined the streams
int route_event(npp_handle h, int event, const uint8_t *d_mask) {
    if (!h->rt.cap) return NPP_OK;
    RouteArgs r = route_args(h);
    r.mask = d_mask;
    HIP_TRY(h, launch_route_event(r, event, h->stream));
    return NPP_OK;
}

// The flags / frames rows the append reads: the caller's, or rows of the handle's own where `o` has none (as the level pool does
// with Pool::flags)
int route_rows(npp_handle h, npp_step_out &o, int n_steps) {
    Routes &R = h->rt;
    if (o.d_flags && o.d_frames) return NPP_OK;
    if (R.rows < n_steps) {
        DevBuf<uint8_t> f;
        DevBuf<uint16_t> x;
        if (f.alloc((size_t)n_steps * h->n) != hipSuccess || x.alloc((size_t)n_steps * h->n) != hipSuccess) {
            (void)hipGetLastError();
            return fail(h, NPP_ERR_HIP, "action routes: hipMalloc of " + std::to_string(n_steps) + " flags / frames rows failed");
        }
        HIP_TRY(h, hipStreamSynchronize(h->stream));   // a queued append may still read the old rows
        R.flags = std::move(f);
        R.frames = std::move(x);
        R.rows = n_steps;
    }
    if (!o.d_flags) o.d_flags = R.flags.get();
    if (!o.d_frames) o.d_frames = R.frames.get();
    return NPP_OK;
}

// The append of one step launch, behind it: on the caller's stream, or -- after a split step -- once per part on the stream that
// stepped the part, by the path of the observation kernels, so npp_step still does not join
int route_append(npp_handle h, const uint8_t *d_actions, int n_steps, int frame_skip, const npp_step_out &o) {
    RouteArgs r = route_args(h);
    r.n_steps = n_steps;
    r.frame_skip = frame_skip;
    r.actions = d_actions;
    r.flags = o.d_flags;
    r.frames = o.d_frames;
    return obs_launch(h, base_args(h), false, false, [&](const KernelArgs &ka, hipStream_t st) {
        RouteArgs q = r;
        q.phase = ka.phase;
        q.phase_id = ka.phase_id;
        return launch_route_append(q, st);
    });
}

// reward mode "pbrs": what both kernels of npp_reward.hip read (the caller fills in the rows, the outputs or the envs)
RewardArgs reward_args(npp_handle h) {
    const LevelSet &L = h->ls;
    const Reward &w = h->rw;
    RewardArgs a{};
    a.n = h->n;
    a.f64 = h->env.f64.get();
    a.u32 = h->env.u32.get();
    a.ent_bits = L.ent.get();
    a.env_level = h->env.level.get();
    a.hdr = L.hdr.get();
    a.rh = L.reach.hdr.get();
    a.rblob = L.reach.blob.get();
    a.rl = w.levels.get();
    const double q[6] = {w.params.death_penalty, w.params.level_completion_reward, w.params.switch_activation_reward,
                         w.params.time_penalty_per_step, w.params.pbrs_objective_weight, w.params.pbrs_gamma};
    std::memcpy(a.params, q, sizeof(q));
    a.sd = w.sd.get();
    a.si = w.si.get();
    a.md = L.reach.miss();
    a.stamp2 = w.stamp2.get();
    a.raw2 = w.raw2.get();
    a.end_bits = (h->flags & NPP_FLAG_AUTORESET) ? (int)(NPP_F_WON | NPP_F_DEAD | NPP_F_TRUNCATED) : 0;
    a.wp_bonus = w.wp_on ? w.wp_bonus.get() : nullptr;
    return a;
}

// the sequential path waypoints: what both kernels of npp_waypoint.hip read
WaypointArgs waypoint_args(npp_handle h) {
    const Reward &w = h->rw;
    WaypointArgs a{};
    a.n = h->n;
    a.f64 = h->env.f64.get();
    a.env_level = h->env.level.get();
    a.wh = w.wp_hdr.get();
    a.wblob = w.wp_blob.get();
    a.params[0] = w.wp_params.collection_radius;
    a.params[1] = w.wp_params.out_of_order_scale;
    a.params[2] = w.wp_params.progress_scale;
    a.state = w.wp_state.get();
    a.end_bits = (h->flags & NPP_FLAG_AUTORESET) ? (int)(NPP_F_WON | NPP_F_DEAD | NPP_F_TRUNCATED) : 0;
    a.bonus = w.wp_bonus.get();
    return a;
}

// an episode start outside the step kernel: the reward state of the envs under the device mask (null = all), or of the `count` envs
// listed in d_envs (those whose d_status entry, when given, is 0), restarts on the state they are in.  The caller has joined the
// streams; no-op with the mode off.
int reward_restart(npp_handle h, const uint8_t *d_mask, const int32_t *d_envs = nullptr, const int32_t *d_status = nullptr, int count = 0, int init = 0) {
    if (!h->rw.mode) return NPP_OK;
    RewardArgs a = reward_args(h);
    a.mask = d_mask;
    a.envs = d_envs;
    a.env_status = d_status;
    a.count = count;
    HIP_TRY(h, launch_reward_restart(a, init, h->stream));
    if (h->rw.wp_on) {   // the calculator's reset() empties the waypoint collection state too
        WaypointArgs q = waypoint_args(h);
        q.mask = d_mask;
        q.envs = d_envs;
        q.env_status = d_status;
        q.count = count;
        HIP_TRY(h, launch_waypoint_restart(q, h->stream));
    }
    h->rw.flags = nullptr;
    h->rw.frames = nullptr;
    return NPP_OK;
}

int reward_restart_range(npp_handle h, int env0, int count) {
    if (!h->rw.mode) return NPP_OK;
    std::vector<uint8_t> mask((size_t)h->n, 0);
    std::fill(mask.begin() + env0, mask.begin() + env0 + count, 1);
    HIP_TRY(h, hipMemcpy(h->env.mask.get(), mask.data(), mask.size(), hipMemcpyHostToDevice));
    return reward_restart(h, h->env.mask.get());
}

// ---- episode statistics (npp_set_episode_stats; the rule: npp_episode.hpp, the kernels: npp_episode.hip).  Nothing below launches
// or allocates while they are off.
EpisodeArgs episode_args(npp_handle h) {
    const Episode &E = h->ep;
    EpisodeArgs a{};
    a.n = h->n;
    a.n_levels = E.n_levels;
    a.i32 = E.i32.get();
    a.f64 = E.f64.get();
    a.table = E.table.get();
    a.env_level = h->env.level.get();
    a.autoreset = (h->flags & NPP_FLAG_AUTORESET) ? 1 : 0;
    return a;
}

// an EP_EV_* event for the envs under the device mask (null = all), or for the `count` envs listed in d_envs (those whose d_status
// entry, when given, is 0), on the caller's stream; the caller has joined the streams
int episode_event(npp_handle h, int event, const uint8_t *d_mask, const int32_t *d_envs = nullptr, const int32_t *d_status = nullptr, int count = 0) {
    if (!h->ep.on) return NPP_OK;
    EpisodeArgs a = episode_args(h);
    a.mask = d_mask;
    a.envs = d_envs;
    a.env_status = d_status;
    a.count = count;
    HIP_TRY(h, launch_episode_event(a, event, h->stream));
    return NPP_OK;
}

// `fresh` = the entities are created for the first time since the level was assigned (the state a replay starts from);
// any later reset is a Simulator.reset(), after which Entity.index no longer starts at 0 (see ZOO_HEAD in npp_internal.hpp)
int reset_impl(npp_handle h, const uint8_t *env_mask, int fresh, int fast = 0, int automatic = 0) {
    if (!h) return NPP_ERR_INVALID;
    if (h->ls.levels.empty()) return fail(h, NPP_ERR_STATE, "npp_reset: no levels loaded");
    ON_DEVICE_JOINED(h);
    KernelArgs a = base_args(h);
    a.reset_fresh = fresh;
    a.fast_reset = fresh ? 0 : fast;
    a.reset_auto = automatic;
    if (env_mask) {
        HIP_TRY(h, hipMemcpyAsync(h->env.mask.get(), env_mask, (size_t)h->n, hipMemcpyHostToDevice, h->stream));
        a.reset_mask = h->env.mask.get();
    }
    HIP_TRY(h, launch_reset(a, h->stream));
    if (int rc = route_event(h, ROUTE_EV_FLIP, a.reset_mask)) return rc;   // (action routes) the episode of a reset env is over
    if (h->pm.mode) {   // (action masking) the counters count observations since the env's last reset
        HIP_TRY(h, launch_path_mask_restart(h->n, a.reset_mask, h->pm.plane(0, h->n), h->pm.plane(1, h->n), h->stream));
        h->pm.flags = nullptr;
    }
    if (int rc = reward_restart(h, a.reset_mask)) return rc;   // (reward mode "pbrs") an episode start
    if (int rc = episode_event(h, EP_EV_RESET, a.reset_mask)) return rc;   // (episode statistics) a running episode is abandoned
    if (env_mask) HIP_TRY(h, hipStreamSynchronize(h->stream));  // env_mask is caller memory: finish the copy
    return NPP_OK;
}

// Level pool: the envs with (flags[e] & bits) draw a level (npp_pool.hip); those that drew another one are reset as after
// npp_assign_levels -- fresh Simulator.reset, reachability cache row and per-episode dictionary dropped -- by the existing kernels
// under the draw's device mask, and, when `out` is given, their observation rows are rewritten by a masked observe launch.
// The caller has joined the streams.
GoalArgs goal_args(npp_handle h, const uint8_t *d_flags, int bits, int count) {
    Goal &G = h->goal;
    GoalArgs a{};
    a.g = GoalState{G.lv.get(), G.ring.get(), G.env.get(), G.d_base_of.get(), G.d_stage_of.get(), h->ls.n_base, h->n, G.ring_words,
                    G.params.rolling_window, G.need, G.params.auto_advance};
    a.flags = d_flags;
    a.bits = bits;
    a.count = count;
    a.env_level = h->env.level.get();
    a.trunc = h->env.trunc.get();
    a.level_trunc = h->dyn_trunc ? h->ls.d_level_trunc.get() : nullptr;
    a.changed = h->pool.changed.get();
    a.list = G.list.get();
    return a;
}

SweepArgs sweep_args(npp_handle h, const uint8_t *d_flags, int bits) {
    const Sweep &S = h->sweep;
    SweepArgs a{};
    a.n = h->n;
    a.n_jobs = S.n_jobs;
    a.jobs = S.jobs.get();
    a.counters = S.counters.get();
    a.env_job = S.env_job.get();
    a.prev_job = S.prev_job.get();
    a.flags = d_flags;
    a.bits = bits;
    a.env_level = h->env.level.get();
    a.trunc = h->env.trunc.get();
    a.level_trunc = h->dyn_trunc ? h->ls.d_level_trunc.get() : nullptr;
    a.changed = h->pool.changed.get();
    a.ep_i32 = h->ep.i32.get();
    a.ep_f64 = h->ep.f64.get();
    a.res_i32 = S.res_i32.get();
    a.res_f64 = S.res_f64.get();
    return a;
}

// (goal curriculum) With the mode on the same call runs its two launches around the draw: the bookkeeping of the envs that ended
// (counted only behind a step: `out` given) in front of it, the assignment to the variant of the level's stage behind it; `draw` =
// false leaves the pool's draw out (npp_reset: the envs restart on the level they have, at its current stage).
int pool_redraw(npp_handle h, const uint8_t *d_flags, int bits, const npp_step_out *out, bool draw = true) {
    const LevelSet &L = h->ls;
    if (h->goal.on) HIP_TRY(h, launch_goal_update(goal_args(h, d_flags, bits, out ? 1 : 0), h->stream));
    PoolArgs p;
    p.n = h->n;
    p.flags = d_flags;
    p.bits = bits;
    p.cdf = L.pool_cdf.get();
    p.n_levels = (int)L.levels.size();
    p.last = h->pool.last;
    p.seed = h->pool.seed;
    p.count = h->env.count.get();
    p.env_level = h->env.level.get();
    p.trunc = h->env.trunc.get();
    p.level_trunc = h->dyn_trunc ? L.d_level_trunc.get() : nullptr;
    p.changed = h->pool.changed.get();
    if (draw && h->pool.on) HIP_TRY(h, launch_pool_draw(p, h->stream));
    // (evaluation sweep) behind a step the next job of the list takes the place of the draw; npp_sweep_start comes here with the
    // changed mask it wrote itself
    if (h->sweep.on && out) HIP_TRY(h, launch_sweep_assign(sweep_args(h, d_flags, bits), h->stream));
    if (h->goal.on) HIP_TRY(h, launch_goal_assign(goal_args(h, d_flags, bits, out ? 1 : 0), h->stream));
    h->pool.dirty = true;
    KernelArgs a = base_args(h);
    a.reset_mask = h->pool.changed.get();
    a.reset_fresh = 1;
    a.fast_reset = 0;   // (base_args carries the auto-reset's NPP_FLAG_FAST_RESET) a new level is a Simulator.reset
    HIP_TRY(h, launch_reset(a, h->stream));
    // (action routes) after a step the envs whose episode ended were flipped by the append: their empty route makes this a no-op
    if (int rc = route_event(h, ROUTE_EV_FLIP, a.reset_mask)) return rc;
    if (L.reach.key) HIP_TRY(h, launch_reach_drop(a, L.reach.key.get(), L.reach.miss(), h->stream));
    if (out) {
        KernelArgs o = base_args(h);
        o.n_ticks = 0;
        o.mode = 0;
        o.autoreset = 0;
        if (int rc = fill_obs_out(h, o, out)) return rc;
        o.out.flags = nullptr; o.out.reward = nullptr; o.out.frames = nullptr; o.out.terminal_state = nullptr; o.out.work = nullptr;
        o.obs_mask = h->pool.changed.get();
        HIP_TRY(h, launch_step(o, h->stream));
    }
    // (reward mode "pbrs") after a step the reward launch restarts the envs whose episode ended, on their new level, from the step's
    // flags; an explicit draw (npp_draw_levels) is an episode start of its own
    // (episode statistics) likewise: after a step the ending row has not been accumulated yet, and the accumulation itself starts the
    // new episode on the level drawn here
    if (!out) {
        if (int rc = reward_restart(h, h->pool.changed.get())) return rc;
        if (int rc = episode_event(h, EP_EV_RESET, h->pool.changed.get())) return rc;
    }
    return NPP_OK;
}

// (evaluation sweep) the sweep ends: every env keeps the level it plays now, the assignment is the host's again, and the result
// planes stay for npp_sweep_view.  The caller is on the device with the streams joined.
int sweep_end(npp_handle h) {
    if (!h->sweep.on) return NPP_OK;
    if (int rc = pull_levels(h)) return rc;
    h->sweep.on = false;
    plan_geometry(h);
    return NPP_OK;
}

// (goal curriculum) base level ids -> the variant of each level's current stage, read from the device
int goal_map_levels(npp_handle h, const int32_t *base_ids, int n, std::vector<int32_t> &out) {
    const Goal &G = h->goal;
    const int nb = h->ls.n_base;
    std::vector<int32_t> lv((size_t)GL_N * nb);
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    HIP_TRY(h, hipMemcpy(lv.data(), G.lv.get(), G.lv.bytes(), hipMemcpyDeviceToHost));
    out.resize(n);
    for (int i = 0; i < n; i++) {
        const int b = base_ids[i];
        if (b < 0 || b >= nb) return fail(h, NPP_ERR_INVALID, "npp_assign_levels: with the goal curriculum on the ids are base level ids");
        out[i] = lv[(size_t)GL_NUM_STAGES * nb + b] > 0 ? lv[(size_t)GL_VARIANT0 * nb + b] + lv[(size_t)GL_STAGE * nb + b] : b;
    }
    return NPP_OK;
}

ArchiveLayout record_layout(npp_handle h) {
    const LevelSet &L = h->ls;
    return archive_layout(L.n_words_max, L.zoo ? L.zoo_words : 0, h->rt.cap);
}

// the live state the record kernels (npp_archive.hip) move, for records laid out by `lay`; the caller fills in which entries and
// records, and nulls what a restore is to leave alone
ArchiveArgs record_args(npp_handle h, const ArchiveLayout &lay) {
    const LevelSet &L = h->ls;
    ArchiveArgs a{};
    a.lay = lay;
    a.n = h->n;
    a.f64 = h->env.f64.get();
    a.u32 = h->env.u32.get();
    a.ent = L.ent.get();
    a.sc = h->env.sc.get();
    a.zoo = lay.zoo_words ? L.zoo.get() : nullptr;
    a.trunc = h->env.trunc.get();
    a.draws = h->env.count.get();
    a.env_level = h->env.level.get();
    a.hdr = L.hdr.get();
    a.reach_key = L.reach.key.get();
    a.reach_cache = L.reach.cache.get();
    a.reach_last_episode = L.reach.last_episode.get();
    if (lay.route_cap) {
        a.route_hdr = h->rt.hdr.get();
        a.route_act = h->rt.act.get();
    }
    return a;
}

}  // namespace

extern "C" {

const char *npp_last_error(npp_handle h) { return h ? h->err.c_str() : host_error().c_str(); }

int npp_create(int n_envs, int device_id, unsigned flags, npp_handle *out) {
    if (!out || n_envs <= 0) return fail(nullptr, NPP_ERR_INVALID, "npp_create: n_envs must be > 0 and out non-NULL");
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count == 0)
        return fail(nullptr, NPP_ERR_HIP, "npp_create: no HIP device available (this library has no CPU fallback)");
    if (device_id < 0 || device_id >= count) return fail(nullptr, NPP_ERR_INVALID, "npp_create: bad device_id");
    DeviceGuard dg(device_id);
    if (dg.err != hipSuccess) return fail(nullptr, NPP_ERR_HIP, std::string("npp_create: hipSetDevice: ") + hipGetErrorString(dg.err));
    npp_handle h = new npp_handle_s();
    h->n = n_envs;
    h->device = device_id;
    h->flags = flags;
    size_t N = (size_t)n_envs;
    EnvState &s = h->env;
    if (s.f64.alloc(NF64 * N) != hipSuccess || s.u32.alloc(NU32 * N) != hipSuccess || s.level.alloc(N) != hipSuccess ||
        s.trunc.alloc(N) != hipSuccess || s.mask.alloc(N) != hipSuccess || s.sc.alloc(48 * N) != hipSuccess || s.count.alloc(N) != hipSuccess) {
        delete h;
        return fail(nullptr, NPP_ERR_HIP, "npp_create: hipMalloc failed");
    }
    h->env_level.assign(N, 0);
    h->trunc.assign(N, 10000);  // MAX_TIME_IN_FRAMES fallback (gym_environment/constants.py:8)
    hipMemcpy(s.trunc.get(), h->trunc.data(), s.trunc.bytes(), hipMemcpyHostToDevice);
    hipMemset(s.level.get(), 0, s.level.bytes());
    hipMemset(s.count.get(), 0, s.count.bytes());
    *out = h;
    return NPP_OK;
}

int npp_destroy(npp_handle h) {
    if (!h) return NPP_OK;
    DeviceGuard dg(h->device);
    hipDeviceSynchronize();
    delete h;
    return NPP_OK;
}

int npp_set_stream(npp_handle h, void *hip_stream) {
    if (!h) return NPP_ERR_INVALID;
    if (h->stream != (hipStream_t)hip_stream) h->tune.restart();   // the autotuner's window events live on the old stream: start its cycle over
    if (h->ov.live_parts > 1 || h->ov.n_cuts) {   // a split step may still be in flight: its other streams join the OLD stream
        ON_DEVICE_JOINED(h);
    }
    if (h->stream != (hipStream_t)hip_stream) h->ov.owned_valid = false;   // (observation overlap) streams are chosen again at the next split step
    h->stream = (hipStream_t)hip_stream;
    return NPP_OK;
}

int npp_sync(npp_handle h) {
    if (!h) return NPP_ERR_INVALID;
    ON_DEVICE_JOINED(h);
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    return NPP_OK;
}

int npp_snapshot(npp_handle h) {
    if (!h) return NPP_ERR_INVALID;
    if (h->ls.levels.empty()) return fail(h, NPP_ERR_STATE, "npp_snapshot: no levels loaded");
    if (h->sweep.on) return fail(h, NPP_ERR_STATE, "npp_snapshot: an evaluation sweep is running (npp_sweep_stop first)");
    ON_DEVICE_JOINED(h);
    Snapshot &s = h->snap;
    const ArchiveLayout lay = record_layout(h);
    if (!s.rec || s.lay.n_words_max != lay.n_words_max || s.lay.zoo_words != lay.zoo_words || s.lay.route_cap != lay.route_cap) {
        HIP_TRY(h, s.rec.alloc((size_t)h->n * lay.words));
        s.lay = lay;
    }
    ArchiveArgs a = record_args(h, lay);   // identity mode: record e <- env e, no meta rows
    a.n_slots = a.count = h->n;
    a.rec = s.rec.get();
    HIP_TRY(h, launch_archive_store(a, h->stream));
    s.ovr = h->ovr;
    s.gen = h->assign_gen;
    return NPP_OK;
}

int npp_restore(npp_handle h, const uint8_t *env_mask) {
    if (!h) return NPP_ERR_INVALID;
    const Snapshot &s = h->snap;
    if (h->sweep.on) return fail(h, NPP_ERR_STATE, "npp_restore: an evaluation sweep is running and a restored env's job would be undefined (npp_sweep_stop first)");
    if (!s.rec || s.gen != h->assign_gen) return fail(h, NPP_ERR_STATE, "npp_restore: no snapshot for the current level assignment");
    ON_DEVICE_JOINED(h);
    ArchiveArgs a = record_args(h, s.lay);   // identity mode: env e <- record e under the mask
    a.n_slots = a.count = h->n;
    a.rec = s.rec.get();
    if (env_mask) {
        HIP_TRY(h, hipMemcpyAsync(h->env.mask.get(), env_mask, (size_t)h->n, hipMemcpyHostToDevice, h->stream));
        a.mask = h->env.mask.get();
    }
    if (h->pool.ever) {   // the pool changed levels since npp_load_levels: the snapshot's levels come back with the state
        a.level_out = h->env.level.get();
        h->pool.dirty = true;
    } else {              // levels, draw counts and the live truncation limits are as they were at npp_snapshot or set since
        a.trunc = nullptr;
        a.draws = nullptr;
    }
    HIP_TRY(h, launch_archive_restore(a, h->stream));
    if (int rc = reward_restart(h, a.mask)) return rc;   // (reward mode "pbrs") records carry no reward state: it restarts on the restored one
    if (int rc = episode_event(h, EP_EV_RESTORE, a.mask)) return rc;   // (episode statistics) an episode begun by a restore
    if (env_mask) HIP_TRY(h, hipStreamSynchronize(h->stream));
    // the restored zoo blocks carry the repositioning flags / coordinates of the snapshot (head words 3..7): the host's
    // view of them (which decides whether the zoo kernels run) is restored with them
    if (s.ovr.size() == h->ovr.size()) {
        for (int e = 0; e < h->n; e++)
            if (!env_mask || env_mask[e]) h->ovr[e] = s.ovr[e];
        h->n_ovr = 0;
        for (int e = 0; e < h->n; e++) h->n_ovr += h->ovr[e] != 0;
        plan_geometry(h, true);   // restoring a checkpoint every few hundred steps must not keep the autotuner in its warm-up
    } else if (h->pool.ever) {
        plan_geometry(h, true);
    }
    return NPP_OK;
}

namespace {
// the refusals the three archive calls share: once levels move on the device, or an entity is repositioned, the host cannot
// know what a record's tables belong to
int archive_refusal(npp_handle h, const char *who) {
    if (h->pool.on) return fail(h, NPP_ERR_STATE, std::string(who) + ": the level pool is on (npp_set_level_pool)");
    if (h->sweep.on) return fail(h, NPP_ERR_STATE, std::string(who) + ": an evaluation sweep is running (npp_sweep_stop first)");
    if (h->n_ovr) return fail(h, NPP_ERR_STATE, std::string(who) + ": an exit switch / door is repositioned (npp_set_entity_pos)");
    return NPP_OK;
}

int archive_move(npp_handle h, const char *who, bool store, const int32_t *d_envs, const int32_t *d_slots, int count, int32_t *d_status) {
    if (!h) return NPP_ERR_INVALID;
    if (count < 0 || (count > 0 && (!d_envs || !d_slots))) return fail(h, NPP_ERR_INVALID, std::string(who) + ": bad arguments");
    if (!h->ar.n_slots) return fail(h, NPP_ERR_STATE, std::string(who) + ": no archive (npp_archive_create)");
    if (int rc = archive_refusal(h, who)) return rc;
    if (store && h->cells.on) return fail(h, NPP_ERR_STATE, std::string(who) + ": the cell index owns the slots (npp_archive_cells_create)");
    ON_DEVICE_JOINED(h);
    const Archive &A = h->ar;
    ArchiveArgs a = record_args(h, A.lay);
    a.n_slots = A.n_slots;
    a.count = count;
    a.envs = d_envs;
    a.slots = d_slots;
    a.status = d_status;
    if (!store && h->rw.mode && !d_status && count > 0) {   // (reward mode "pbrs") which entries restored decides which envs restart
        Reward &w = h->rw;
        if (w.restore_cap < (size_t)count) {
            DevBuf<int32_t> t;
            HIP_TRY(h, t.alloc((size_t)count));
            w.restore_status = std::move(t);
            w.restore_cap = (size_t)count;
        }
        a.status = w.restore_status.get();
    }
    if (!store && h->ep.on && !a.status && count > 0) {   // (episode statistics) likewise
        Episode &E = h->ep;
        if (E.restore_cap < (size_t)count) {
            DevBuf<int32_t> t;
            HIP_TRY(h, t.alloc((size_t)count));
            HIP_TRY(h, hipStreamSynchronize(h->stream));   // a queued event may still read the old row
            E.restore_status = std::move(t);
            E.restore_cap = (size_t)count;
        }
        a.status = E.restore_status.get();
    }
    a.rec = A.rec.get();
    a.meta_f64 = A.meta_f64.get();
    a.meta_i32 = A.meta_i32.get();
    if (!store) a.draws = nullptr;   // (the pool is refused: a restored env keeps its draw count)
    HIP_TRY(h, store ? launch_archive_store(a, h->stream) : launch_archive_restore(a, h->stream));
    if (!store && count > 0)   // (reward mode "pbrs") records carry no reward state: it restarts on the restored one
        if (int rc = reward_restart(h, nullptr, d_envs, a.status, count)) return rc;
    if (!store && count > 0)   // (episode statistics) the entries that restored begin an episode there
        if (int rc = episode_event(h, EP_EV_RESTORE, nullptr, d_envs, a.status, count)) return rc;
    // a restored env takes the record's truncation limit on the device: the host mirror is read back where a host path needs it
    if (!store && count > 0) h->pool.dirty = true;
    return NPP_OK;
}
}  // namespace

int npp_archive_create(npp_handle h, int n_slots) {
    if (!h) return NPP_ERR_INVALID;
    if (n_slots < 0) return fail(h, NPP_ERR_INVALID, "npp_archive_create: n_slots must be >= 0 (0 frees the archive)");
    ON_DEVICE_JOINED(h);
    if (n_slots == 0) {
        HIP_TRY(h, hipStreamSynchronize(h->stream));   // queued store / restore launches still read the records
        h->ar = Archive();
        h->cells = Cells();
        return NPP_OK;
    }
    if (h->ls.levels.empty()) return fail(h, NPP_ERR_STATE, "npp_archive_create: no levels loaded");
    if (int rc = archive_refusal(h, "npp_archive_create")) return rc;
    Archive A;   // complete or not at all: a failed allocation leaves the previous archive in place
    A.lay = record_layout(h);
    const size_t S = (size_t)n_slots;
    if (A.rec.alloc(S * A.lay.words) != hipSuccess || A.meta_f64.alloc(S * ARCHIVE_META_F64) != hipSuccess ||
        A.meta_i32.alloc(S * ARCHIVE_META_I32) != hipSuccess) {
        (void)hipGetLastError();
        return fail(h, NPP_ERR_HIP, "npp_archive_create: hipMalloc of " + std::to_string(n_slots) + " slots of " +
                                        std::to_string(A.lay.words * 4) + " bytes failed");
    }
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    HIP_TRY(h, hipMemsetAsync(A.rec.get(), 0, A.rec.bytes(), h->stream));
    HIP_TRY(h, hipMemsetAsync(A.meta_f64.get(), 0, A.meta_f64.bytes(), h->stream));
    HIP_TRY(h, hipMemsetAsync(A.meta_i32.get(), 0, A.meta_i32.bytes(), h->stream));
    A.n_slots = n_slots;
    h->ar = std::move(A);
    h->cells = Cells();   // (a cell index described the slots of the old archive)
    return NPP_OK;
}

int npp_archive_store(npp_handle h, const int32_t *d_envs, const int32_t *d_slots, int count, int32_t *d_status) {
    return archive_move(h, "npp_archive_store", true, d_envs, d_slots, count, d_status);
}

int npp_archive_restore(npp_handle h, const int32_t *d_envs, const int32_t *d_slots, int count, int32_t *d_status) {
    return archive_move(h, "npp_archive_restore", false, d_envs, d_slots, count, d_status);
}

int npp_archive_meta_view(npp_handle h, const double **d_f64, const int32_t **d_i32) {
    if (!h) return NPP_ERR_INVALID;
    if (!h->ar.n_slots) return fail(h, NPP_ERR_STATE, "npp_archive_meta_view: no archive (npp_archive_create)");
    if (d_f64) *d_f64 = h->ar.meta_f64.get();
    if (d_i32) *d_i32 = h->ar.meta_i32.get();
    return NPP_OK;
}

int npp_archive_num_slots(npp_handle h) { return h ? h->ar.n_slots : 0; }
int npp_archive_record_bytes(npp_handle h) { return h && h->ar.n_slots ? h->ar.lay.words * 4 : 0; }

int npp_set_routes(npp_handle h, int capacity) {
    if (!h) return NPP_ERR_INVALID;
    if (capacity < 0) return fail(h, NPP_ERR_INVALID, "npp_set_routes: capacity must be >= 0 (0 switches the routes off)");
    if (h->ar.n_slots)
        return fail(h, NPP_ERR_STATE, "npp_set_routes: a checkpoint archive exists and its records' layout depends on the routes "
                                      "(call it before npp_archive_create)");
    ON_DEVICE_JOINED(h);
    Routes r;   // complete or not at all: a failed allocation leaves the previous state in place
    if (capacity > 0) {
        r.cap = route_round_cap(capacity);
        if (r.hdr.alloc((size_t)h->n * ROUTE_HDR_WORDS) != hipSuccess || r.act.alloc((size_t)h->n * 2 * r.cap) != hipSuccess) {
            (void)hipGetLastError();
            return fail(h, NPP_ERR_HIP, "npp_set_routes: hipMalloc of " + std::to_string(h->n) + " x 2 routes of " + std::to_string(r.cap) +
                                            " bytes failed");
        }
    }
    HIP_TRY(h, hipStreamSynchronize(h->stream));   // queued appends / record moves still use the old buffers
    h->rt = std::move(r);
    h->snap = Snapshot();   // its records were laid out for the old capacity
    if (h->rt.cap) {
        HIP_TRY(h, hipMemsetAsync(h->rt.act.get(), 0, h->rt.act.bytes(), h->stream));
        if (int rc = route_event(h, ROUTE_EV_INIT, nullptr)) return rc;
    }
    return NPP_OK;
}

int npp_route_view(npp_handle h, const uint8_t **d_actions, const int32_t **d_hdr, int *capacity) {
    if (!h) return NPP_ERR_INVALID;
    if (!h->rt.cap) return fail(h, NPP_ERR_STATE, "npp_route_view: action routes are off (npp_set_routes)");
    if (d_actions) *d_actions = h->rt.act.get();
    if (d_hdr) *d_hdr = h->rt.hdr.get();
    if (capacity) *capacity = h->rt.cap;
    return NPP_OK;
}

int npp_archive_route_view(npp_handle h, const uint32_t **d_records, int64_t *hdr_offset_words, int64_t *stride_words) {
    if (!h) return NPP_ERR_INVALID;
    if (!h->ar.n_slots) return fail(h, NPP_ERR_STATE, "npp_archive_route_view: no archive (npp_archive_create)");
    if (!h->ar.lay.route_cap) return fail(h, NPP_ERR_STATE, "npp_archive_route_view: action routes are off (npp_set_routes)");
    if (d_records) *d_records = h->ar.rec.get();
    if (hdr_offset_words) *hdr_offset_words = h->ar.lay.off_route;
    if (stride_words) *stride_words = h->ar.lay.words;
    return NPP_OK;
}

int npp_set_episode_stats(npp_handle h, int enable) {
    if (!h) return NPP_ERR_INVALID;
    if (enable && h->ls.levels.empty()) return fail(h, NPP_ERR_STATE, "npp_set_episode_stats: no levels loaded");
    ON_DEVICE_JOINED(h);
    Episode e;   // complete or not at all: a failed allocation leaves the previous state in place
    if (enable) {
        e.n_levels = (int)h->ls.levels.size();
        if (e.i32.alloc((size_t)EP_NI * h->n) != hipSuccess || e.f64.alloc((size_t)EP_ND * h->n) != hipSuccess ||
            e.table.alloc((size_t)e.n_levels * EP_COLS) != hipSuccess) {
            (void)hipGetLastError();
            return fail(h, NPP_ERR_HIP, "npp_set_episode_stats: hipMalloc of the records of " + std::to_string(h->n) + " envs and the table of " +
                                            std::to_string(e.n_levels) + " levels failed");
        }
        e.on = true;
    }
    HIP_TRY(h, hipStreamSynchronize(h->stream));   // queued accumulations / events still use the old planes
    if (!enable && h->sweep.on)   // (evaluation sweep) its results are the episode records: without them it ends
        if (int rc = sweep_end(h)) return rc;
    h->ep = std::move(e);
    if (h->ep.on) {
        HIP_TRY(h, hipMemsetAsync(h->ep.table.get(), 0, h->ep.table.bytes(), h->stream));
        if (int rc = episode_event(h, EP_EV_INIT, nullptr)) return rc;
    }
    return NPP_OK;
}

int npp_episode_accumulate(npp_handle h, const uint8_t *d_flags, const uint16_t *d_frames, const float *d_reward, const float *d_components,
                           int n_steps, uint8_t *d_ended) {
    if (!h) return NPP_ERR_INVALID;
    if (!h->ep.on) return fail(h, NPP_ERR_STATE, "npp_episode_accumulate: episode statistics are off (npp_set_episode_stats)");
    if (!d_flags || !d_frames || !d_reward || n_steps <= 0)
        return fail(h, NPP_ERR_INVALID, "npp_episode_accumulate: flags, frames and reward rows and n_steps > 0 are required");
    if (d_components && ((uintptr_t)d_components & 7))
        return fail(h, NPP_ERR_INVALID, "npp_episode_accumulate: d_components must be 8-byte aligned");
    ON_DEVICE_JOINED(h);
    EpisodeArgs a = episode_args(h);
    a.n_steps = n_steps;
    a.flags = d_flags;
    a.frames = d_frames;
    a.reward = d_reward;
    a.comps = d_components;
    a.ended = d_ended;
    HIP_TRY(h, launch_episode(a, h->stream));
    // (evaluation sweep) the finished half of the records of the envs whose job ended in the step, into the jobs' result rows
    if (h->sweep.on && n_steps == 1) HIP_TRY(h, launch_sweep_collect(sweep_args(h, d_flags, 0), h->stream));
    return NPP_OK;
}

int npp_episode_restart(npp_handle h, const uint8_t *d_mask, int from_restore) {
    if (!h) return NPP_ERR_INVALID;
    if (!h->ep.on) return fail(h, NPP_ERR_STATE, "npp_episode_restart: episode statistics are off (npp_set_episode_stats)");
    ON_DEVICE_JOINED(h);
    return episode_event(h, from_restore ? EP_EV_RESTORE : EP_EV_RESET, d_mask);
}

int npp_episode_view(npp_handle h, const int32_t **d_i32, const double **d_f64, const uint64_t **d_table) {
    if (!h) return NPP_ERR_INVALID;
    if (!h->ep.on) return fail(h, NPP_ERR_STATE, "npp_episode_view: episode statistics are off (npp_set_episode_stats)");
    if (d_i32) *d_i32 = h->ep.i32.get();
    if (d_f64) *d_f64 = h->ep.f64.get();
    if (d_table) *d_table = reinterpret_cast<const uint64_t *>(h->ep.table.get());
    return NPP_OK;
}

int npp_episode_table_reset(npp_handle h) {
    if (!h) return NPP_ERR_INVALID;
    if (!h->ep.on) return fail(h, NPP_ERR_STATE, "npp_episode_table_reset: episode statistics are off (npp_set_episode_stats)");
    ON_DEVICE_JOINED(h);
    HIP_TRY(h, hipMemsetAsync(h->ep.table.get(), 0, h->ep.table.bytes(), h->stream));
    return NPP_OK;
}

namespace {
// what explore and select share: the refusals, the join, the tables
int cells_args(npp_handle h, const char *who, CellArgs &a) {
    if (!h) return NPP_ERR_INVALID;
    if (!h->cells.on) return fail(h, NPP_ERR_STATE, std::string(who) + ": no cell index (npp_archive_cells_create)");
    if (int rc = archive_refusal(h, who)) return rc;
    ON_DEVICE_JOINED(h);
    const Cells &c = h->cells;
    a = CellArgs{};
    a.n = h->n;
    a.n_levels = (int)h->ls.levels.size();
    a.n_slots = h->ar.n_slots;
    a.f64 = h->env.f64.get();
    a.u32 = h->env.u32.get();
    a.ent = h->ls.ent.get();
    a.env_level = h->env.level.get();
    a.hdr = h->ls.hdr.get();
    a.best = c.best.get();
    a.cell_slot = c.cell_slot.get();
    a.cell_score = c.cell_score.get();
    a.visits = c.visits.get();
    a.chosen = c.chosen.get();
    a.slot_key = c.slot_key.get();
    a.n_used = c.n_used.get();
    a.env_key = c.env_key.get();
    a.slot_of_env = c.slot_of_env.get();
    a.cdf = c.cdf.get();
    a.seed = c.seed;
    a.call = c.call;
    return NPP_OK;
}

// one explore (npp_archive_explore, and every tick of npp_archive_seed): propose, assign, and the winners' states by the kernel
// that writes every record and meta row
int explore_launch(npp_handle h, const CellArgs &a) {
    HIP_TRY(h, launch_cells_propose(a, h->stream));
    HIP_TRY(h, launch_cells_assign(a, h->stream));
    const Archive &A = h->ar;
    ArchiveArgs s = record_args(h, A.lay);
    s.n_slots = A.n_slots;
    s.count = h->n;
    s.envs = h->cells.iota.get();
    s.slots = h->cells.slot_of_env.get();
    s.rec = A.rec.get();
    s.meta_f64 = A.meta_f64.get();
    s.meta_i32 = A.meta_i32.get();
    HIP_TRY(h, launch_archive_store(s, h->stream));
    return NPP_OK;
}
}  // namespace

int npp_archive_cells_create(npp_handle h, int enable, uint64_t seed) {
    if (!h) return NPP_ERR_INVALID;
    ON_DEVICE_JOINED(h);
    if (!enable) {
        HIP_TRY(h, hipStreamSynchronize(h->stream));   // queued explore / select launches still read the tables
        h->cells = Cells();
        return NPP_OK;
    }
    if (!h->ar.n_slots) return fail(h, NPP_ERR_STATE, "npp_archive_cells_create: no archive (npp_archive_create)");
    if (int rc = archive_refusal(h, "npp_archive_cells_create")) return rc;
    Cells c;   // complete or not at all: a failed allocation leaves the previous state in place
    const size_t K = h->ls.levels.size() * (size_t)NPP_CELLS_PER_LEVEL, N = (size_t)h->n;
    if (c.best.alloc(K) != hipSuccess || c.cdf.alloc(K) != hipSuccess || c.cell_slot.alloc(K) != hipSuccess ||
        c.cell_score.alloc(K) != hipSuccess || c.visits.alloc(K) != hipSuccess || c.chosen.alloc(K) != hipSuccess ||
        c.slot_key.alloc((size_t)h->ar.n_slots) != hipSuccess || c.n_used.alloc(1) != hipSuccess || c.env_key.alloc(N) != hipSuccess ||
        c.slot_of_env.alloc(N) != hipSuccess || c.iota.alloc(N) != hipSuccess) {
        (void)hipGetLastError();
        return fail(h, NPP_ERR_HIP, "npp_archive_cells_create: hipMalloc of the tables of " + std::to_string(K) + " keys failed");
    }
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    std::vector<int32_t> iota(N);
    for (size_t e = 0; e < N; e++) iota[e] = (int32_t)e;
    HIP_TRY(h, hipMemcpy(c.iota.get(), iota.data(), c.iota.bytes(), hipMemcpyHostToDevice));
    HIP_TRY(h, hipMemsetAsync(c.best.get(), 0, c.best.bytes(), h->stream));
    HIP_TRY(h, hipMemsetAsync(c.cdf.get(), 0, c.cdf.bytes(), h->stream));
    HIP_TRY(h, hipMemsetAsync(c.cell_slot.get(), 0xff, c.cell_slot.bytes(), h->stream));   // -1
    HIP_TRY(h, hipMemsetAsync(c.cell_score.get(), 0, c.cell_score.bytes(), h->stream));
    HIP_TRY(h, hipMemsetAsync(c.visits.get(), 0, c.visits.bytes(), h->stream));
    HIP_TRY(h, hipMemsetAsync(c.chosen.get(), 0, c.chosen.bytes(), h->stream));
    HIP_TRY(h, hipMemsetAsync(c.slot_key.get(), 0xff, c.slot_key.bytes(), h->stream));
    HIP_TRY(h, hipMemsetAsync(c.n_used.get(), 0, c.n_used.bytes(), h->stream));
    HIP_TRY(h, hipMemsetAsync(c.env_key.get(), 0xff, c.env_key.bytes(), h->stream));
    HIP_TRY(h, hipMemsetAsync(c.slot_of_env.get(), 0xff, c.slot_of_env.bytes(), h->stream));
    // the index owns every slot from now on: the archive starts empty
    HIP_TRY(h, hipMemsetAsync(h->ar.meta_f64.get(), 0, h->ar.meta_f64.bytes(), h->stream));
    HIP_TRY(h, hipMemsetAsync(h->ar.meta_i32.get(), 0, h->ar.meta_i32.bytes(), h->stream));
    c.on = true;
    c.seed = seed;
    c.call = 0;
    h->cells = std::move(c);
    return NPP_OK;
}

int npp_archive_explore(npp_handle h, const float *d_score, const uint8_t *d_mask, int32_t *d_status) {
    CellArgs a;
    if (int rc = cells_args(h, "npp_archive_explore", a)) return rc;
    a.score = d_score;
    a.mask = d_mask;
    a.status = d_status;
    return explore_launch(h, a);
}

int npp_archive_select(npp_handle h, const uint8_t *d_mask, int32_t *d_slots) {
    if (h && !d_slots) return fail(h, NPP_ERR_INVALID, "npp_archive_select: d_slots must be non-NULL");
    CellArgs a;
    if (int rc = cells_args(h, "npp_archive_select", a)) return rc;
    a.mask = d_mask;
    a.slots_out = d_slots;
    HIP_TRY(h, launch_cells_cdf(a, h->stream));
    HIP_TRY(h, launch_cells_pick(a, h->stream));
    h->cells.call++;
    return NPP_OK;
}

int npp_archive_cells_view(npp_handle h, const int32_t **d_cell_slot, const float **d_cell_score, const uint32_t **d_visits,
                           const uint32_t **d_chosen, const int32_t **d_slot_key, const int32_t **d_n_used) {
    if (!h) return NPP_ERR_INVALID;
    if (!h->cells.on) return fail(h, NPP_ERR_STATE, "npp_archive_cells_view: no cell index (npp_archive_cells_create)");
    const Cells &c = h->cells;
    if (d_cell_slot) *d_cell_slot = c.cell_slot.get();
    if (d_cell_score) *d_cell_score = c.cell_score.get();
    if (d_visits) *d_visits = c.visits.get();
    if (d_chosen) *d_chosen = c.chosen.get();
    if (d_slot_key) *d_slot_key = c.slot_key.get();
    if (d_n_used) *d_n_used = c.n_used.get();
    return NPP_OK;
}

int npp_set_launch_geometry(npp_handle h, int lanes_per_env, int waves_per_block) {
    if (!h) return NPP_ERR_INVALID;
    if (lanes_per_env < 0 || lanes_per_env > 64 || (lanes_per_env & (lanes_per_env - 1)) || waves_per_block < 0 || waves_per_block > 4)
        return fail(h, NPP_ERR_INVALID, "npp_set_launch_geometry: lanes_per_env must be 0 or a power of two <= 64, waves_per_block 0..4");
    h->lanes_per_env = lanes_per_env;
    h->waves_per_block = waves_per_block;
    plan_geometry(h);
    return NPP_OK;
}

int npp_get_launch_geometry(npp_handle h, int *lanes_per_env, int *waves_per_block) {
    if (!h) return NPP_ERR_INVALID;
    if (lanes_per_env) *lanes_per_env = h->plan.g;
    if (waves_per_block) *waves_per_block = h->plan.wpb;
    return NPP_OK;
}

static int install_levels(npp_handle h, LevelSet &next);

int npp_set_goal_curriculum(npp_handle h, int enable, const NppGoalCurriculumParams *params) {
    if (!h) return fail(nullptr, NPP_ERR_INVALID, "npp_set_goal_curriculum: NULL handle");
    if (h->ls.levels.empty()) return fail(h, NPP_ERR_STATE, "npp_set_goal_curriculum: no levels loaded");
    if (!enable && !h->goal.on) return NPP_OK;
    if (h->sweep.on) return fail(h, NPP_ERR_STATE, "npp_set_goal_curriculum: an evaluation sweep is running (npp_sweep_stop first)");
    NppGoalCurriculumParams q;
    if (params) q = *params; else npp_goal_default_params(&q);
    if (enable && (!(q.stage_distance_interval > 0.0) || !std::isfinite(q.stage_distance_interval) || !(q.advancement_threshold >= 0.0) ||
                   !(q.advancement_threshold <= 1.0) || q.rolling_window < 1 || q.rolling_window > GOAL_MAX_WINDOW))
        return fail(h, NPP_ERR_INVALID, "npp_set_goal_curriculum: interval must be > 0, threshold in [0, 1], window in 1..8192");
    ON_DEVICE_JOINED(h);
    if (int rc = pull_levels(h)) return rc;
    std::vector<int32_t> base_assign((size_t)h->n);
    for (int e = 0; e < h->n; e++) base_assign[e] = h->goal.on ? h->goal.base_of[h->env_level[e]] : h->env_level[e];
    // the new set is built whole, as npp_load_levels builds it: a refused call leaves the handle as it was
    LevelSet next;
    next.n_base = h->ls.n_base;
    next.maps = h->ls.maps;
    const int nb = next.n_base;
    next.levels.resize(nb);
    Goal G;
    G.params = q;
    G.stages.resize(nb);
    G.variant0.assign(nb, 0);
    std::string err;
    for (int i = 0; i < nb; i++) {
        if (!compile_level(next.maps[i].data(), (int64_t)next.maps[i].size(), next.levels[i], err))
            return fail(h, NPP_ERR_INVALID, "npp_set_goal_curriculum: level " + std::to_string(i) + ": " + err);
        G.base_of.push_back(i);
        G.stage_of.push_back(-1);
    }
    for (int i = 0; enable && i < nb; i++) {
        ReachBuilt R;
        build_reach(next.levels[i], R);
        if (!goal_stage_table(next.levels[i], R, q.stage_distance_interval, G.stages[i]))
            return fail(h, NPP_ERR_INVALID, "npp_set_goal_curriculum: level " + std::to_string(i) + " has more than 1024 stages at this interval");
        G.variant0[i] = G.stages[i].num_stages > 0 ? (int32_t)next.levels.size() : i;
        for (int st = 0; st < G.stages[i].num_stages; st++) {
            next.levels.emplace_back();
            if (!compile_level_variant(next.maps[i].data(), (int64_t)next.maps[i].size(), G.stages[i].pos.data() + 4 * (size_t)st, next.levels.back(), err))
                return fail(h, NPP_ERR_INVALID, "npp_set_goal_curriculum: level " + std::to_string(i) + " stage " + std::to_string(st) + ": " + err);
            G.base_of.push_back(i);
            G.stage_of.push_back(st);
        }
    }
    const size_t nl = next.levels.size(), N = (size_t)h->n;
    if (enable) {
        G.ring_words = (q.rolling_window + 31) / 32;
        G.need = goal_need(q.rolling_window, q.advancement_threshold);
        G.all.assign(nl, 1.0);
        HIP_TRY(h, G.lv.alloc((size_t)GL_N * nb));
        HIP_TRY(h, G.ring.alloc((size_t)nb * G.ring_words));
        HIP_TRY(h, G.env.alloc((size_t)GE_N * N));
        HIP_TRY(h, G.d_base_of.alloc(nl));
        HIP_TRY(h, G.d_stage_of.alloc(nl));
        HIP_TRY(h, G.list.alloc(2 * N));
        if (!h->pool.changed) {
            HIP_TRY(h, h->pool.changed.alloc(N));
            HIP_TRY(h, h->pool.flags.alloc(N));
            HIP_TRY(h, hipMemset(h->pool.flags.get(), 0, N));
        }
        std::vector<int32_t> lv((size_t)GL_N * nb, 0);
        for (int i = 0; i < nb; i++) {
            lv[(size_t)GL_PENDING * nb + i] = -1;
            lv[(size_t)GL_NUM_STAGES * nb + i] = G.stages[i].num_stages;
            lv[(size_t)GL_VARIANT0 * nb + i] = G.variant0[i];
        }
        HIP_TRY(h, hipMemcpy(G.lv.get(), lv.data(), G.lv.bytes(), hipMemcpyHostToDevice));
        HIP_TRY(h, hipMemset(G.ring.get(), 0, G.ring.bytes()));
        HIP_TRY(h, hipMemset(G.env.get(), 0, G.env.bytes()));
        HIP_TRY(h, hipMemset(G.list.get(), 0, G.list.bytes()));
        HIP_TRY(h, hipMemcpy(G.d_base_of.get(), G.base_of.data(), G.d_base_of.bytes(), hipMemcpyHostToDevice));
        HIP_TRY(h, hipMemcpy(G.d_stage_of.get(), G.stage_of.data(), G.d_stage_of.bytes(), hipMemcpyHostToDevice));
    }
    if (int rc = install_levels(h, next)) return rc;   // (switches the mode off, as for any new set)
    if (enable) {
        h->goal = std::move(G);
        h->goal.on = true;
        h->pool.ever = true;   // levels change on the device from here on: snapshots carry them
    }
    plan_geometry(h);
    return npp_assign_levels(h, nullptr, base_assign.data(), h->n);
}

int npp_goal_set_stage(npp_handle h, int level, int stage) {
    if (!h) return fail(nullptr, NPP_ERR_INVALID, "npp_goal_set_stage: NULL handle");
    if (!h->goal.on) return fail(h, NPP_ERR_STATE, "npp_goal_set_stage: the goal curriculum is off (npp_set_goal_curriculum)");
    const int nb = h->ls.n_base;
    if (level < -1 || level >= nb || stage < 0) return fail(h, NPP_ERR_INVALID, "npp_goal_set_stage: level is -1 or a base level id, stage >= 0");
    ON_DEVICE_JOINED(h);
    std::vector<int32_t> pend(nb);
    int32_t *d_pend = h->goal.lv.get() + (size_t)GL_PENDING * nb;
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    HIP_TRY(h, hipMemcpy(pend.data(), d_pend, sizeof(int32_t) * nb, hipMemcpyDeviceToHost));
    for (int l = level < 0 ? 0 : level; l < (level < 0 ? nb : level + 1); l++) {
        const int ns = h->goal.stages[l].num_stages;
        if (ns > 0) pend[l] = stage < ns - 1 ? stage : ns - 1;
    }
    HIP_TRY(h, hipMemcpy(d_pend, pend.data(), sizeof(int32_t) * nb, hipMemcpyHostToDevice));
    return NPP_OK;
}

int npp_goal_view(npp_handle h, const int32_t **d_level_words, const uint32_t **d_ring, const int32_t **d_env_words, int *n_base, int *ring_words,
                  int *need) {
    if (!h) return fail(nullptr, NPP_ERR_INVALID, "npp_goal_view: NULL handle");
    if (!h->goal.on) return fail(h, NPP_ERR_STATE, "npp_goal_view: the goal curriculum is off (npp_set_goal_curriculum)");
    static_assert(GL_N == NPP_GOAL_LEVEL_WORDS && GE_N == NPP_GOAL_ENV_WORDS, "npp_amd.h describes the planes");
    if (d_level_words) *d_level_words = h->goal.lv.get();
    if (d_ring) *d_ring = h->goal.ring.get();
    if (d_env_words) *d_env_words = h->goal.env.get();
    if (n_base) *n_base = h->ls.n_base;
    if (ring_words) *ring_words = h->goal.ring_words;
    if (need) *need = h->goal.need;
    return NPP_OK;
}

int npp_goal_tables(npp_handle h, int32_t *base_of, int32_t *stage_of, int *n_base) {
    if (!h) return fail(nullptr, NPP_ERR_INVALID, "npp_goal_tables: NULL handle");
    if (!h->goal.on) return fail(h, NPP_ERR_STATE, "npp_goal_tables: the goal curriculum is off (npp_set_goal_curriculum)");
    if (base_of) std::memcpy(base_of, h->goal.base_of.data(), sizeof(int32_t) * h->goal.base_of.size());
    if (stage_of) std::memcpy(stage_of, h->goal.stage_of.data(), sizeof(int32_t) * h->goal.stage_of.size());
    if (n_base) *n_base = h->ls.n_base;
    return NPP_OK;
}

int npp_goal_stage_positions(npp_handle h, int level, int32_t *num_stages, double *dist, double *orig, int stage_cap, double *pos) {
    if (!h) return fail(nullptr, NPP_ERR_INVALID, "npp_goal_stage_positions: NULL handle");
    if (!h->goal.on) return fail(h, NPP_ERR_STATE, "npp_goal_stage_positions: the goal curriculum is off (npp_set_goal_curriculum)");
    if (level < 0 || level >= h->ls.n_base || stage_cap < 0) return fail(h, NPP_ERR_INVALID, "npp_goal_stage_positions: bad arguments");
    const GoalStages &S = h->goal.stages[level];
    if (num_stages) *num_stages = S.num_stages;
    if (dist) { dist[0] = S.d_switch; dist[1] = S.d_exit; dist[2] = S.d_combined; }
    if (orig) std::memcpy(orig, S.orig, sizeof(S.orig));
    for (size_t i = 0; pos && i < S.pos.size() && i < 4 * (size_t)stage_cap; i++) pos[i] = S.pos[i];
    return NPP_OK;
}

int npp_num_envs(npp_handle h) { return h ? h->n : 0; }
int npp_num_levels(npp_handle h) { return h ? (int)h->ls.levels.size() : 0; }

int npp_load_levels(npp_handle h, const double *blob, const int64_t *offsets, int n_levels) {
    if (!h || !blob || !offsets || n_levels <= 0) return fail(h, NPP_ERR_INVALID, "npp_load_levels: bad arguments");
    ON_DEVICE_JOINED(h);
    // The new set is built whole in `next` and swapped in only once it is complete and fits: a failed call leaves the previous
    // set loaded.  Everything that can fail short of a device error comes before the first device write.
    LevelSet next;
    std::vector<CompiledLevel> &lv = next.levels;
    lv.resize(n_levels);
    for (int i = 0; i < n_levels; i++) {
        std::string err;
        if (offsets[i + 1] < offsets[i] || !compile_level(blob + offsets[i], offsets[i + 1] - offsets[i], lv[i], err))
            return fail(h, NPP_ERR_INVALID, "npp_load_levels: level " + std::to_string(i) + ": " + err);
        if (lv[i].unsupported_mask && !(h->flags & NPP_FLAG_ALLOW_UNSUPPORTED)) {
            std::string t;
            for (int b = 0; b < 32; b++)
                if (lv[i].unsupported_mask & (1u << b)) t += (t.empty() ? "" : ",") + std::to_string(b);
            return fail(h, NPP_ERR_UNSUPPORTED, "npp_load_levels: level " + std::to_string(i) +
                                                    " uses entity types outside the accelerated path: " + t);
        }
    }
    next.n_base = n_levels;
    next.maps.resize(n_levels);
    for (int i = 0; i < n_levels; i++) next.maps[i].assign(blob + offsets[i], blob + offsets[i + 1]);
    return install_levels(h, next);
}

// packs and uploads a compiled level set and swaps it in (npp_load_levels; npp_set_goal_curriculum with its variants behind the base
// levels); the caller is on the device with the streams joined
static int install_levels(npp_handle h, LevelSet &next) {
    std::vector<CompiledLevel> &lv = next.levels;
    const int n_levels = (int)lv.size();
    // ---- pack the blob
    std::vector<unsigned char> host;
    std::vector<LevelHdr> &hdrs = next.hdrs;
    hdrs.resize(n_levels);
    auto append = [&](const void *p, size_t bytes, uint32_t align) -> uint32_t {
        uint32_t off = align_up((uint32_t)host.size(), align);
        host.resize(off + bytes);
        if (bytes) std::memcpy(host.data() + off, p, bytes);
        return off;
    };
    for (int i = 0; i < n_levels; i++) {
        const CompiledLevel &L = lv[i];
        LevelHdr &H = hdrs[i];
        std::memset(&H, 0, sizeof(H));
        uint32_t hot_bytes = align_up(HOT_SEGS + 2u * (uint32_t)L.segs.size(), 16);
        std::vector<unsigned char> hot(hot_bytes, 0);
        std::memcpy(hot.data() + HOT_SEG_START, L.seg_start.data(), 2 * L.seg_start.size());
        std::memcpy(hot.data() + HOT_ENT_START, L.ent_start.data(), 2 * L.ent_start.size());
        std::memcpy(hot.data() + HOT_BOUNDS, L.cell_bounds.data(), L.cell_bounds.size());
        if (!L.segs.empty()) std::memcpy(hot.data() + HOT_SEGS, L.segs.data(), 2 * L.segs.size());
        H.off_hot = append(hot.data(), hot.size(), 16);
        H.hot_bytes = hot_bytes;
        H.off_ent_x = append(L.ent_x.data(), 8 * L.ent_x.size(), 8);
        H.off_ent_y = append(L.ent_y.data(), 8 * L.ent_y.size(), 8);
        H.off_ent_meta = append(L.ent_meta.data(), 4 * L.ent_meta.size(), 4);
        H.off_init_words = append(L.ent_init_words.data(), 4 * L.ent_init_words.size(), 4);
        H.off_tiles = append(L.tiles.data(), L.tiles.size(), 4);
        H.off_raster = append(L.raster_order.data(), 2 * L.raster_order.size(), 4);
        H.off_doors = append(L.door_segs.data(), 8 * L.door_segs.size(), 8);
        H.n_door = (uint32_t)(L.door_segs.size() / 5);
        H.has_zoo = L.has_zoo ? 1u : 0u;
        H.off_ent_seq = append(L.ent_seq.data(), 2 * L.ent_seq.size(), 4);
        H.off_ent_cell = append(L.ent_cell.data(), 2 * L.ent_cell.size(), 4);
        H.off_mov_meta = append(L.mov_meta.data(), 4 * L.mov_meta.size(), 4);
        H.off_mov_x0 = append(L.mov_x0.data(), 8 * L.mov_x0.size(), 8);
        H.off_mov_y0 = append(L.mov_y0.data(), 8 * L.mov_y0.size(), 8);
        H.off_edges = append(L.edges.data(), 4 * L.edges.size(), 8);
        H.off_door_tab = append(L.door_tab.data(), 4 * L.door_tab.size(), 4);
        H.off_ent_rank = append(L.ent_rank.data(), 2 * L.ent_rank.size(), 4);
        H.off_mov_rank = append(L.mov_rank.data(), 2 * L.mov_rank.size(), 4);
        H.off_ent_perm = append(L.ent_perm.data(), 2 * L.ent_perm.size(), 4);
        H.off_ent_ident = append(L.ent_ident.data(), 2 * L.ent_ident.size(), 4);
        H.off_keep_words = append(L.ent_keep_words.data(), 4 * L.ent_keep_words.size(), 4);
        H.off_draw_recs = append(L.draw_recs.data(), 4 * L.draw_recs.size(), 16);
        H.n_mov = (uint32_t)L.mov_meta.size();
        H.n_zdoor = (uint32_t)(L.door_tab.size() / 2);
        H.n_created = (uint32_t)L.n_created;
        H.n_balls = (uint32_t)L.n_balls;
        H.ball_first = 0;
        for (size_t m = 0; m < L.mov_meta.size(); m++)
            if ((L.mov_meta[m] & 7u) == MK_BALL) { H.ball_first = (uint32_t)m; break; }
        H.db_count = L.db_count;
        for (int k = 0; k < 5; k++) H.locked_slots[k] = L.locked_slots[k];
        // every level's block is initialised by the reset kernel (locked doors have an edge counter too)
        next.zoo_doors = std::max(next.zoo_doors, (int)H.n_zdoor);
        next.zoo_movers = std::max(next.zoo_movers, (int)H.n_mov);
        H.n_seg = (uint32_t)L.segs.size();
        H.n_ent = (uint32_t)L.ent_x.size();
        H.n_words = (uint32_t)L.ent_init_words.size();
        H.n_think = (uint32_t)L.n_thinkable;
        H.obs_switch = L.obs_switch;
        H.obs_door = L.obs_door;
        H.spawn_x = L.spawn_x; H.spawn_y = L.spawn_y;
        if (L.obs_switch >= 0) {   // exit_switch_position / exit_door_position (nplay_headless.py:578-616)
            H.sw_x = L.ent_x[L.obs_switch]; H.sw_y = L.ent_y[L.obs_switch];
            H.door_x = L.ent_x[L.obs_door]; H.door_y = L.ent_y[L.obs_door];
        }
        next.n_words_max = std::max(next.n_words_max, (int)H.n_words);
        H.fits_lds = 1;
        next.hot_max = std::max(next.hot_max, hot_bytes);
    }
    zoo_block_plan(lv, next.zoo_doors, next.zoo_movers);
    for (int i = 0; i < n_levels; i++)   // round-1 fault: a block sized over zoo levels only was overrun
        if ((int)hdrs[i].n_zdoor > next.zoo_doors || (int)hdrs[i].n_mov > next.zoo_movers)
            return fail(h, NPP_ERR_STATE, "npp_load_levels: zoo block plan does not cover level " + std::to_string(i));
    next.zoo_words = zoo_words_for(next.zoo_doors, next.zoo_movers);
    {   // the plan the call ends with (every env on level 0, nothing repositioned, the pool off) must fit LDS
        const Plan p = make_plan(next, h->n, std::vector<int32_t>((size_t)h->n, 0), h->lanes_per_env, h->waves_per_block, false, nullptr);
        if (lds_bytes(p.lds_hot_cap, next.n_words_max, (64 / p.g) * p.wpb, p.zoo_active ? next.zoo_words : 0) > LDS_BUDGET)
            return fail(h, NPP_ERR_INVALID, "npp_load_levels: entity tables exceed LDS");
    }
    const size_t N = (size_t)h->n;
    HIP_TRY(h, next.zoo.alloc((size_t)next.zoo_words * N));
    HIP_TRY(h, next.blob.alloc(host.size(), 16));
    HIP_TRY(h, next.hdr.alloc(n_levels));
    HIP_TRY(h, next.ent.alloc((size_t)next.n_words_max * N));
    // ---- upload and swap in (queued work may still read the old set: it is released at the swap)
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    HIP_TRY(h, hipMemset(h->env.count.get(), 0, h->env.count.bytes()));   // a new level set turns the level pool off; draw counts restart
    HIP_TRY(h, hipMemset(next.zoo.get(), 0, next.zoo.bytes()));
    HIP_TRY(h, hipMemcpy(next.blob.get(), host.data(), host.size(), hipMemcpyHostToDevice));
    HIP_TRY(h, hipMemcpy(next.hdr.get(), hdrs.data(), next.hdr.bytes(), hipMemcpyHostToDevice));
    HIP_TRY(h, hipMemset(next.ent.get(), 0, next.ent.bytes()));
    h->ls = std::move(next);
    h->ar = Archive();   // the checkpoint archive's records were laid out for the old set
    h->cells = Cells();  // (the cell index goes with the archive)
    h->demo = Demo();    // (demonstration player) its level ids named levels of the old set
    h->ep = Episode();   // (episode statistics) the table had a row per level of the old set: the feature is off
    h->rw = Reward();    // (reward mode "pbrs") the levels' constants and every env's reward state belonged to the old set: the mode is off
    h->snap = Snapshot();   // likewise
    h->pool.on = h->pool.ever = h->pool.dirty = false;   // (its weights were per level of the old set)
    h->pool.w.clear();
    h->goal = Goal();    // (goal curriculum) the variants belonged to the old set: the mode is off
    h->sweep = Sweep();  // (evaluation sweep) its jobs named levels of the old set: it ends, and its results go
    h->ovr.assign(h->n, 0);
    h->n_ovr = 0;
    h->assign_gen++;
    std::fill(h->env_level.begin(), h->env_level.end(), 0);
    plan_geometry(h);
    HIP_TRY(h, hipMemset(h->env.level.get(), 0, h->env.level.bytes()));
    if (h->dyn_trunc)
        if (int rc = apply_dynamic_truncation(h, nullptr)) return rc;
    if (int rc = route_event(h, ROUTE_EV_INIT, nullptr)) return rc;   // (action routes) level ids lost their meaning: both routes empty
    return reset_impl(h, nullptr, 1);
}

int npp_assign_levels(npp_handle h, const int32_t *env_ids, const int32_t *level_ids, int n) {
    if (!h || !level_ids || n <= 0) return fail(h, NPP_ERR_INVALID, "npp_assign_levels: bad arguments");
    if (h->ls.levels.empty()) return fail(h, NPP_ERR_STATE, "npp_assign_levels: no levels loaded");
    if (!env_ids && n != h->n) return fail(h, NPP_ERR_INVALID, "npp_assign_levels: env_ids == NULL needs n == n_envs");
    if (h->sweep.on) return fail(h, NPP_ERR_STATE, "npp_assign_levels: an evaluation sweep is running and assigns the levels itself (npp_sweep_stop first)");
    ON_DEVICE_JOINED(h);
    if (int rc = pull_levels(h)) return rc;   // (level pool) the whole mirror is uploaded below
    std::vector<int32_t> mapped;
    if (h->goal.on) {   // (goal curriculum) base ids in, the variant of each level's current stage out
        if (int rc = goal_map_levels(h, level_ids, n, mapped)) return rc;
        level_ids = mapped.data();
    }
    std::vector<uint8_t> mask(h->n, 0);
    for (int i = 0; i < n; i++) {   // validate everything before touching the assignment: an error must leave host and device in step
        int e = env_ids ? env_ids[i] : i;
        if (e < 0 || e >= h->n || level_ids[i] < 0 || level_ids[i] >= (int)h->ls.levels.size())
            return fail(h, NPP_ERR_INVALID, "npp_assign_levels: index out of range");
    }
    for (int i = 0; i < n; i++) {
        int e = env_ids ? env_ids[i] : i;
        h->env_level[e] = level_ids[i];
        mask[e] = 1;
        if (!h->ovr.empty() && h->ovr[e]) { h->ovr[e] = 0; h->n_ovr--; }   // a new level: nothing is repositioned
    }
    h->assign_gen++;
    plan_geometry(h);
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    HIP_TRY(h, hipMemcpy(h->env.level.get(), h->env_level.data(), h->env.level.bytes(), hipMemcpyHostToDevice));
    const Reach &r = h->ls.reach;
    if (r.key) {   // a new level: the env's cached reachability vector belongs to the old one
        KernelArgs a = base_args(h);
        HIP_TRY(h, hipMemcpy(h->env.mask.get(), mask.data(), (size_t)h->n, hipMemcpyHostToDevice));
        a.reset_mask = h->env.mask.get();
        HIP_TRY(h, launch_reach_drop(a, r.key.get(), r.miss(), h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
    }
    if (h->dyn_trunc)
        if (int rc = apply_dynamic_truncation(h, mask.data())) return rc;
    return reset_impl(h, mask.data(), 1);
}

int npp_reset(npp_handle h, const uint8_t *env_mask) { return npp_reset_ex(h, env_mask, 0); }

int npp_reset_ex(npp_handle h, const uint8_t *env_mask, int mode) {
    if (!h) return NPP_ERR_INVALID;
    if (mode < 0 || mode > 2) return fail(h, NPP_ERR_INVALID, "npp_reset_ex: mode must be 0, 1 or 2");
    if (h->goal.on) {   // (goal curriculum) the envs restart on the variant of their level's current stage, assigned as the pool assigns
        if (h->ls.levels.empty()) return fail(h, NPP_ERR_STATE, "npp_reset: no levels loaded");
        ON_DEVICE_JOINED(h);
        uint8_t *d_mask = h->env.mask.get();
        if (env_mask) HIP_TRY(h, hipMemcpyAsync(d_mask, env_mask, (size_t)h->n, hipMemcpyHostToDevice, h->stream));
        else HIP_TRY(h, hipMemsetAsync(d_mask, 1, (size_t)h->n, h->stream));
        if (int rc = pool_redraw(h, d_mask, 0xff, nullptr, false)) return rc;
        HIP_TRY(h, hipStreamSynchronize(h->stream));   // env_mask is caller memory; the mask buffer is reused below
    }
    const int fast = mode == 2 || (mode == 0 && (h->flags & NPP_FLAG_FAST_RESET));
    // mode 0 follows NppEnvironment.reset: the first reset after a level assignment reloads the map (Simulator.reset), later ones
    // are fast resets; the per-env "no reset yet" bit lives in the state planes (npp_state.hpp: S_FRESH)
    return reset_impl(h, env_mask, 0, fast ? 1 : 0, mode == 0 ? 1 : 0);
}

int npp_set_truncation_limit(npp_handle h, const int32_t *limits, int32_t all) {
    if (!h) return NPP_ERR_INVALID;
    ON_DEVICE_JOINED(h);
    if (limits) h->trunc.assign(limits, limits + h->n);
    else h->trunc.assign(h->n, all);
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    HIP_TRY(h, hipMemcpy(h->env.trunc.get(), h->trunc.data(), h->env.trunc.bytes(), hipMemcpyHostToDevice));
    return NPP_OK;
}

int npp_set_dynamic_truncation(npp_handle h, int enable) {
    if (!h) return NPP_ERR_INVALID;
    h->dyn_trunc = enable != 0;
    if (!h->dyn_trunc || h->ls.levels.empty()) return NPP_OK;
    ON_DEVICE_JOINED(h);
    if (h->pool.on || h->sweep.on)
        if (int rc = upload_level_trunc(h)) return rc;
    return apply_dynamic_truncation(h, nullptr);
}

int npp_set_level_pool(npp_handle h, const double *weights, int n_levels, uint64_t seed) {
    if (!h) return NPP_ERR_INVALID;
    Pool &P = h->pool;
    if (!weights) {   // off: every env keeps the level it plays now
        if (!P.on) return NPP_OK;
        ON_DEVICE_JOINED(h);
        if (int rc = pull_levels(h)) return rc;
        P.on = false;
        plan_geometry(h);
        return NPP_OK;
    }
    if (h->ls.levels.empty()) return fail(h, NPP_ERR_STATE, "npp_set_level_pool: no levels loaded");
    if (h->sweep.on) return fail(h, NPP_ERR_STATE, "npp_set_level_pool: an evaluation sweep is running (npp_sweep_stop first)");
    std::vector<double> padded;
    if (h->goal.on && n_levels == h->ls.n_base) {   // (goal curriculum) one weight per BASE level: the variants are never drawn
        padded.assign(weights, weights + n_levels);
        padded.resize(h->ls.levels.size(), 0.0);
        weights = padded.data();
        n_levels = (int)padded.size();
    } else if (h->goal.on) {
        return fail(h, NPP_ERR_INVALID, "npp_set_level_pool: with the goal curriculum on the weights are per base level");
    }
    std::vector<double> cdf;
    int last = 0;
    std::string err;
    if (!pool_cdf(weights, n_levels, (int)h->ls.levels.size(), cdf, last, err)) return fail(h, NPP_ERR_INVALID, "npp_set_level_pool: " + err);
    if (h->n_ovr) return fail(h, NPP_ERR_STATE, "npp_set_level_pool: an exit switch / door is repositioned (npp_set_entity_pos)");
    if (h->ar.n_slots) return fail(h, NPP_ERR_STATE, "npp_set_level_pool: a checkpoint archive exists (npp_archive_create)");
    ON_DEVICE_JOINED(h);
    const size_t N = (size_t)h->n;
    DevBuf<double> &d_cdf = h->ls.pool_cdf;
    HIP_TRY(h, hipStreamSynchronize(h->stream));   // the previous CDF may still be read by queued draws
    if (!d_cdf) HIP_TRY(h, d_cdf.alloc(cdf.size()));
    if (!P.changed) {
        HIP_TRY(h, P.changed.alloc(N));
        HIP_TRY(h, P.flags.alloc(N));
        HIP_TRY(h, hipMemset(P.flags.get(), 0, N));
    }
    HIP_TRY(h, hipMemcpy(d_cdf.get(), cdf.data(), sizeof(double) * cdf.size(), hipMemcpyHostToDevice));
    if (!P.on || seed != P.seed) HIP_TRY(h, hipMemset(h->env.count.get(), 0, h->env.count.bytes()));   // a new stream of draws
    if (h->dyn_trunc)
        if (int rc = upload_level_trunc(h)) return rc;
    const bool was_on = P.on;
    P.w.assign(weights, weights + n_levels);
    P.seed = seed;
    P.last = last;
    P.on = P.ever = true;
    // the step-variant autotuner decides once for the pool: a weight update keeps its decision unless it switches the zoo kernels
    plan_geometry(h, was_on);
    return NPP_OK;
}

int npp_draw_levels(npp_handle h, const uint8_t *env_mask) {
    if (!h) return NPP_ERR_INVALID;
    if (!h->pool.on) return fail(h, NPP_ERR_STATE, "npp_draw_levels: the level pool is off (npp_set_level_pool)");
    ON_DEVICE_JOINED(h);
    uint8_t *d_mask = h->env.mask.get();
    if (env_mask) HIP_TRY(h, hipMemcpyAsync(d_mask, env_mask, (size_t)h->n, hipMemcpyHostToDevice, h->stream));
    else HIP_TRY(h, hipMemsetAsync(d_mask, 1, (size_t)h->n, h->stream));
    if (int rc = pool_redraw(h, d_mask, 0xff, nullptr)) return rc;
    if (env_mask) HIP_TRY(h, hipStreamSynchronize(h->stream));   // env_mask is caller memory: finish the copy
    return NPP_OK;
}

int npp_sweep_start(npp_handle h, const int32_t *jobs, int n_jobs) {
    if (!h) return fail(nullptr, NPP_ERR_INVALID, "npp_sweep_start: NULL handle");
    if (h->ls.levels.empty()) return fail(h, NPP_ERR_STATE, "npp_sweep_start: no levels loaded");
    if (n_jobs <= 0) return fail(h, NPP_ERR_STATE, "npp_sweep_start: n_jobs must be > 0 (an empty job list has nothing to play)");
    if (!jobs) return fail(h, NPP_ERR_INVALID, "npp_sweep_start: jobs is NULL");
    const int n_levels = (int)h->ls.levels.size(), n = h->n;
    for (int j = 0; j < n_jobs; j++)
        if (jobs[j] < 0 || jobs[j] >= n_levels)
            return fail(h, NPP_ERR_INVALID, "npp_sweep_start: job " + std::to_string(j) + " names level " + std::to_string(jobs[j]) +
                                                ", outside the " + std::to_string(n_levels) + " loaded levels");
    if (!h->ep.on) return fail(h, NPP_ERR_STATE, "npp_sweep_start: episode statistics are off and the results are their records (npp_set_episode_stats)");
    if (!(h->flags & NPP_FLAG_AUTORESET)) return fail(h, NPP_ERR_STATE, "npp_sweep_start: the handle was created without NPP_FLAG_AUTORESET and jobs are handed out at the auto-reset");
    if (h->pool.on) return fail(h, NPP_ERR_STATE, "npp_sweep_start: the level pool is on (npp_set_level_pool(h, NULL, 0, 0) first)");
    if (h->goal.on) return fail(h, NPP_ERR_STATE, "npp_sweep_start: the goal curriculum is on (npp_set_goal_curriculum(h, 0, NULL) first)");
    if (h->ar.n_slots) return fail(h, NPP_ERR_STATE, "npp_sweep_start: a checkpoint archive exists (npp_archive_create(h, 0) first)");
    if (h->n_ovr) return fail(h, NPP_ERR_STATE, "npp_sweep_start: an exit switch / door is repositioned (npp_set_entity_pos)");
    ON_DEVICE_JOINED(h);
    if (int rc = sweep_end(h)) return rc;   // a second start begins clean
    if (int rc = pull_levels(h)) return rc;
    const size_t N = (size_t)n, J = (size_t)n_jobs;
    Sweep S;   // complete or not at all: a failed allocation leaves the handle without a sweep and with its old results
    if (S.jobs.alloc(J) != hipSuccess || S.counters.alloc(3) != hipSuccess || S.env_job.alloc(N) != hipSuccess || S.prev_job.alloc(N) != hipSuccess ||
        S.res_i32.alloc((size_t)SWEEP_RI * J) != hipSuccess || S.res_f64.alloc((size_t)SWEEP_RD * J) != hipSuccess) {
        (void)hipGetLastError();
        return fail(h, NPP_ERR_HIP, "npp_sweep_start: hipMalloc of the state of " + std::to_string(n_jobs) + " jobs failed");
    }
    Pool &P = h->pool;
    if (!P.changed) {   // the changed mask and the flags row the sweep shares with the level pool
        HIP_TRY(h, P.changed.alloc(N));
        HIP_TRY(h, P.flags.alloc(N));
        HIP_TRY(h, hipMemset(P.flags.get(), 0, N));
    }
    if (h->dyn_trunc)
        if (int rc = upload_level_trunc(h)) return rc;
    S.n_jobs = n_jobs;
    S.w.assign((size_t)n_levels, 0.0);
    for (int j = 0; j < n_jobs; j++) S.w[jobs[j]] = 1.0;
    // Start: env e < min(n, J) takes job e and is put on its level; the others are idle and keep theirs
    std::vector<int32_t> env_job(N), prev(N, -1), res((size_t)SWEEP_RI * J, 0);
    std::vector<uint8_t> mask(N, 0);
    for (int e = 0; e < n; e++) {
        const int j = env_job[e] = sweep_start_job(e, n_jobs);
        if (j < 0) continue;
        mask[e] = 1;
        h->env_level[e] = jobs[j];
        if (h->dyn_trunc) h->trunc[e] = h->ls.level_trunc[jobs[j]];
    }
    for (size_t j = 0; j < J; j++) res[(size_t)SWEEP_R_ENV * J + j] = -1;
    const int32_t counters[3] = {n < n_jobs ? n : n_jobs, 0, n_jobs};
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    HIP_TRY(h, hipMemcpy(S.jobs.get(), jobs, S.jobs.bytes(), hipMemcpyHostToDevice));
    HIP_TRY(h, hipMemcpy(S.counters.get(), counters, sizeof(counters), hipMemcpyHostToDevice));
    HIP_TRY(h, hipMemcpy(S.env_job.get(), env_job.data(), S.env_job.bytes(), hipMemcpyHostToDevice));
    HIP_TRY(h, hipMemcpy(S.prev_job.get(), prev.data(), S.prev_job.bytes(), hipMemcpyHostToDevice));
    HIP_TRY(h, hipMemcpy(S.res_i32.get(), res.data(), S.res_i32.bytes(), hipMemcpyHostToDevice));
    HIP_TRY(h, hipMemset(S.res_f64.get(), 0, S.res_f64.bytes()));
    HIP_TRY(h, hipMemcpy(h->env.level.get(), h->env_level.data(), h->env.level.bytes(), hipMemcpyHostToDevice));
    HIP_TRY(h, hipMemcpy(h->env.trunc.get(), h->trunc.data(), h->env.trunc.bytes(), hipMemcpyHostToDevice));
    HIP_TRY(h, hipMemcpy(P.changed.get(), mask.data(), N, hipMemcpyHostToDevice));
    h->sweep = std::move(S);
    h->sweep.on = true;
    h->assign_gen++;   // (a snapshot of the old assignment no longer restores)
    plan_geometry(h);
    // every env with a job is reset as after npp_assign_levels, under the mask written above (no draw, no assignment launch)
    return pool_redraw(h, nullptr, 0, nullptr, false);
}

int npp_sweep_stop(npp_handle h) {
    if (!h) return fail(nullptr, NPP_ERR_INVALID, "npp_sweep_stop: NULL handle");
    if (!h->sweep.on) return NPP_OK;
    ON_DEVICE_JOINED(h);
    return sweep_end(h);
}

int npp_sweep_view(npp_handle h, const int32_t **d_env_job, const int32_t **d_results_i32, const double **d_results_f64,
                   const int32_t **d_counters, int *n_jobs) {
    if (!h) return fail(nullptr, NPP_ERR_INVALID, "npp_sweep_view: NULL handle");
    const Sweep &S = h->sweep;
    if (!S.n_jobs) return fail(h, NPP_ERR_STATE, "npp_sweep_view: no evaluation sweep was started on this level set (npp_sweep_start)");
    if (d_env_job) *d_env_job = S.env_job.get();
    if (d_results_i32) *d_results_i32 = S.res_i32.get();
    if (d_results_f64) *d_results_f64 = S.res_f64.get();
    if (d_counters) *d_counters = S.counters.get();
    if (n_jobs) *n_jobs = S.n_jobs;
    return NPP_OK;
}

int npp_env_level_view(npp_handle h, const int32_t **d_levels) {
    if (!h || !d_levels) return fail(h, NPP_ERR_INVALID, "npp_env_level_view: bad arguments");
    *d_levels = h->env.level.get();
    return NPP_OK;
}

int npp_get_env_levels(npp_handle h, int32_t *host_out) {
    if (!h || !host_out) return fail(h, NPP_ERR_INVALID, "npp_get_env_levels: bad arguments");
    ON_DEVICE_JOINED(h);
    if (int rc = pull_levels(h)) return rc;
    std::memcpy(host_out, h->env_level.data(), sizeof(int32_t) * (size_t)h->n);
    return NPP_OK;
}

namespace {
// 256 launches of warm-up (episodes desynchronise: right after a reset every env sits at its spawn and the launches are dominated by
// the levels with a crease under the spawn, which favours variant 2 -- a first cut that tuned on launches 48 .. 288 picked it for the
// mixed set and lost 10 %), then 9 interleaved windows of 48 launches; the decision is re-examined every 16 384 launches
constexpr int TUNE_WARM = 256, TUNE_WINDOW = 48, TUNE_ROUNDS = 3, TUNE_AGAIN = 16384;
// called by npp_step before every launch; returns the variant to launch.  *pair >= 0: a measured launch -- npp_step records
// ev[2 * pair] right before and ev[2 * pair + 1] right after the step kernel, so that only the kernel itself is timed
// (observation kernels and the caller's own work on the stream, whose cost varies with the state, stay outside: ADVICE r2)
int tune_next(npp_handle h, int *pair) {
    Tuner &T = h->tune;
    *pair = -1;
    if (T.pin >= 0) return T.pin;
    if (h->plan.g != 16 || h->plan.zoo_active) return 0;   // only the plain G = 16 kernels have variants
    if (T.tuned) {
        static const long again = [] { const char *ev = std::getenv("NPP_TUNE_AGAIN"); return ev ? std::atol(ev) : (long)TUNE_AGAIN; }();   // tests shorten it
        if (++T.since < again) return T.variant;
        T.tuned = false; T.state = 0; T.count = TUNE_WARM; T.since = 0;   // measure again, no warm-up needed
    }
    const int n_win = 3 * TUNE_ROUNDS;
    if (T.state == 0) {   // warm-up on variant 0
        if (++T.count <= TUNE_WARM) return T.variant;
        if (T.ev.empty()) {
            T.ev.resize((size_t)2 * TUNE_WINDOW * n_win);
            for (Event &e : T.ev)
                if (e.create(hipEventDefault) != hipSuccess) {   // no events: stay on variant 0
                    T.ev.clear();
                    T.tuned = true; T.variant = 0;
                    return 0;
                }
        }
        T.state = 1; T.count = 0;
    }
    if (T.state <= n_win) {   // window w measures variant (w - 1) % 3
        const int w = T.state;
        *pair = (w - 1) * TUNE_WINDOW + T.count;
        if (++T.count == TUNE_WINDOW) { T.state++; T.count = 0; }
        return (w - 1) % 3;
    }
    // all windows recorded: decide as soon as the last launch has been reached by the GPU (no waiting)
    if (hipEventQuery(T.ev.back().get()) == hipSuccess) {
        float t[3] = {0.f, 0.f, 0.f};
        bool ok = true;
        for (int w = 0; w < n_win && ok; w++)
            for (int k = 0; k < TUNE_WINDOW && ok; k++) {
                float ms = 0.f;
                const size_t p = (size_t)w * TUNE_WINDOW + k;
                ok = hipEventElapsedTime(&ms, T.ev[2 * p].get(), T.ev[2 * p + 1].get()) == hipSuccess;
                t[w % 3] += ms;
            }
        int best = 0;
        if (ok) for (int v = 1; v < 3; v++) if (t[v] < t[best]) best = v;
        // build 0 is the one that still spills (192 B of scratch per lane: 64-72 MB of HBM traffic per launch against 8-12 MB for the
        // other two, profiles/r03_*_summary.json `variants`): it has to win by more than 4 % to be taken (mines: it wins by 2.9 %,
        // doors by 2.1 % -- both go to a spill-free build; NPP_TUNE_MARGIN_PCT=0 restores the plain argmin)
        static const float margin = [] { const char *ev = std::getenv("NPP_TUNE_MARGIN_PCT"); return 1.f + 0.01f * (ev ? (float)std::atof(ev) : 4.f); }();
        if (ok && best == 0) {
            const int alt = t[1] <= t[2] ? 1 : 2;
            if (t[alt] <= t[0] * margin) best = alt;
        }
        T.variant = best; T.tuned = true; T.since = 0;
        return best;
    }
    return T.variant;
}
}  // namespace

int npp_set_obs_overlap_parts(npp_handle h, const int *cuts, int n_cuts) {
    if (!h || n_cuts < 0 || n_cuts > 3 || (n_cuts && !cuts)) return fail(h, NPP_ERR_INVALID, "npp_set_obs_overlap_parts: at most three cuts");
    for (int i = 0; i < n_cuts; i++)
        if (cuts[i] <= (i ? cuts[i - 1] : 0) || cuts[i] >= 100)
            return fail(h, NPP_ERR_INVALID, "npp_set_obs_overlap_parts: cuts must be ascending percentages in (0, 100)");
    ON_DEVICE_JOINED(h);
    Overlap &ov = h->ov;
    if (n_cuts > 0 && !ov.phase) {
        HIP_TRY(h, ov.phase.alloc(h->n));
        HIP_TRY(h, hipMemsetAsync(ov.phase.get(), 0, ov.phase.bytes(), h->stream));
        for (Event &e : ov.ov_ev) HIP_TRY(h, e.create(hipEventDisableTiming));
    }
    for (Event &e : ov.part_ev)
        if (!e) HIP_TRY(h, e.create(hipEventDisableTiming));
    for (Event &e : ov.side_ev)
        if (!e) HIP_TRY(h, e.create(hipEventDisableTiming));
    if (n_cuts != ov.n_cuts) ov.owned_valid = false;
    ov.phase_dirty = true;
    ov.n_cuts = n_cuts;
    for (int i = 0; i < n_cuts; i++) ov.cut_pct[i] = cuts[i];
    if (n_cuts > 0)
        if (int rc = calibrate_streams(h, streams_needed(h))) return rc;
    return NPP_OK;
}

int npp_set_obs_overlap(npp_handle h, int percent) {
    if (!h || percent < 0 || percent >= 100) return fail(h, NPP_ERR_INVALID, "npp_set_obs_overlap: percent must be in [0, 100)");
    return npp_set_obs_overlap_parts(h, &percent, percent > 0 ? 1 : 0);
}

int npp_join(npp_handle h) {
    if (!h) return NPP_ERR_INVALID;
    ON_DEVICE_JOINED(h);
    return NPP_OK;
}

int npp_set_step_variant(npp_handle h, int variant) {
    if (!h || variant < -1 || variant > 2) return fail(h, NPP_ERR_INVALID, "npp_set_step_variant: variant must be -1 (autotune) or 0..2");
    h->tune.pin = variant;
    h->tune.restart();
    return NPP_OK;
}

int npp_get_step_variant(npp_handle h, int *variant, int *tuned) {
    if (!h) return NPP_ERR_INVALID;
    const bool plain = h->plan.g == 16 && !h->plan.zoo_active;
    if (variant) *variant = plain ? h->tune.variant : 0;
    if (tuned) *tuned = (h->tune.tuned || h->tune.pin >= 0 || !plain) ? 1 : 0;
    return NPP_OK;
}

}  // extern "C"

namespace {
int step_impl(npp_handle h, const uint8_t *d_actions, int frame_skip, const npp_step_out *out) {
    ON_DEVICE_JOINED(h);
    KernelArgs a = base_args(h);
    a.inputs = d_actions;
    a.n_ticks = frame_skip;
    a.mode = 0;
    if (int rc = fill_obs_out(h, a, out)) return rc;
    Orders &o = h->ord;
    {   // heavy-first workgroup order: rebuilt from the per-block costs every 16th launch (and whenever the launch geometry changes)
        const int epb = (64 / (h->plan.g > 0 ? h->plan.g : 1)) * (h->plan.wpb > 0 ? h->plan.wpb : 1);
        const int blocks = (h->n + epb - 1) / epb;
        if (!o.wg_order) {
            HIP_TRY(h, o.wg_order.alloc(h->n));
            HIP_TRY(h, o.wg_cost.alloc(h->n));
            o.wg_blocks = 0;
        }
        const bool fresh = blocks != o.wg_blocks;
        if (fresh) h->tune.restart();
        if (fresh || o.step_launches % 16 == 0) {
            h->ov.phase_dirty = true;   // (observation overlap) the parts are pieces of this order
            if (fresh) HIP_TRY(h, hipMemsetAsync(o.wg_cost.get(), 0, o.wg_cost.bytes(), h->stream));
            HIP_TRY(h, launch_cost_order(o.wg_cost.get(), o.wg_order.get(), blocks, h->stream));
            HIP_TRY(h, hipMemsetAsync(o.wg_cost.get(), 0, (size_t)blocks * sizeof(uint32_t), h->stream));   // costs are maxima over the next 16 launches
            o.wg_blocks = blocks;
        }
        o.step_launches++;
        a.wg_order = o.wg_order.get();
        a.wg_cost = o.wg_cost.get();
    }
    int pair = -1;
    a.variant = tune_next(h, &pair);
    Overlap &ov = h->ov;
    if (ov.n_cuts > 0 && ov.phase && pair < 0 && (h->tune.tuned || h->tune.pin >= 0 || h->plan.g != 16 || h->plan.zoo_active)) {
        // observation overlap: the pieces of the heavy-first order as launches of their own, the most expensive first; the
        // observation entry points called next launch one kernel per part.  Only with workgroups of whole reachability groups (16
        // envs) and never on a launch the autotuner is timing.
        const int epb = (64 / h->plan.g) * h->plan.wpb, blocks = (h->n + epb - 1) / epb;
        int edge[5] = {0, 0, 0, 0, 0};   // part q = n_cuts - i covers order entries [edge[i], edge[i + 1])
        bool ok = epb % 16 == 0;
        for (int i = 0; i < ov.n_cuts; i++) {
            edge[i + 1] = (int)((long long)blocks * ov.cut_pct[i] / 100);
            ok = ok && edge[i + 1] > edge[i];
        }
        edge[ov.n_cuts + 1] = blocks;
        ok = ok && edge[ov.n_cuts + 1] > edge[ov.n_cuts];
        if (ok) {
            // the one-wavefront-per-SIMD build holds 310 registers: beside it neither another part nor an observation kernel finds
            // room on the SIMD, which is the point of the split (doors, full Dict: 502 us per step with it, 435-442 with build 0)
            if (a.variant == 2) a.variant = 0;
            if (!ov.owned_valid || ov.owned_for != h->stream)   // (first split step after npp_set_stream: one-off, synchronises)
                if (int rc = calibrate_streams(h, streams_needed(h))) return rc;
            if (ov.phase_dirty) {   // the env -> part map, on the caller's stream ahead of the fork
                HIP_TRY(h, launch_phase_assign(o.wg_order.get(), blocks, epb, h->n, edge, ov.n_cuts + 1, ov.phase.get(), h->stream));
                ov.phase_dirty = false;
            }
            HIP_TRY(h, hipEventRecord(ov.ov_ev[0].get(), h->stream));
            hipError_t e = hipSuccess;
            for (int i = 0; i <= ov.n_cuts && e == hipSuccess; i++) {
                const int q = ov.n_cuts - i;
                KernelArgs ap = a;
                ap.wg_first = edge[i]; ap.wg_count = edge[i + 1] - edge[i];
                if (ov.part_stream[q] != h->stream) e = hipStreamWaitEvent(ov.part_stream[q], ov.ov_ev[0].get(), 0);
                if (e == hipSuccess) e = launch_step(ap, ov.part_stream[q]);
            }
            ov.live_parts = ov.n_cuts + 1;   // (only now: a part that failed to launch leaves the others to be joined right here)
            if (e != hipSuccess) {
                (void)join_streams(h);
                return fail(h, NPP_ERR_HIP, std::string("npp_step: part launch: ") + hipGetErrorString(e));
            }
            return NPP_OK;
        }
    }
    if (pair >= 0) hipEventRecord(h->tune.ev[2 * (size_t)pair].get(), h->stream);
    const hipError_t le = launch_step(a, h->stream);
    if (pair >= 0) hipEventRecord(h->tune.ev[2 * (size_t)pair + 1].get(), h->stream);
    HIP_TRY(h, le);
    return NPP_OK;
}
}  // namespace

extern "C" {

int npp_step(npp_handle h, const uint8_t *d_actions, int frame_skip, const npp_step_out *out) {
    if (!h || !d_actions || frame_skip <= 0) return fail(h, NPP_ERR_INVALID, "npp_step: bad arguments");
    if (h->ls.levels.empty()) return fail(h, NPP_ERR_STATE, "npp_step: no levels loaded");
    const bool pool = (h->pool.on || h->goal.on || h->sweep.on) && (h->flags & NPP_FLAG_AUTORESET);   // (goal curriculum, evaluation sweep: the same tail)
    if (!pool && !h->rt.cap && !h->pm.mode && !h->rw.mode) return step_impl(h, d_actions, frame_skip, out);
    npp_step_out o;
    std::memset(&o, 0, sizeof(o));
    if (out) o = *out;
    if (h->pm.mode) {   // action masking: npp_path_action_mask reads the step's flags row (the counters' latch)
        if (!o.d_flags) o.d_flags = h->pm.flagbuf.get();
        h->pm.flags = o.d_flags;
    }
    if (h->rt.cap) {   // action routes: the append behind the step reads the step's flags and frames rows
        ON_DEVICE_JOINED(h);
        if (int rc = route_rows(h, o, 1)) return rc;
    }
    if (h->rw.mode) {   // reward mode "pbrs": npp_step_reward reads the step's flags and frames rows
        if (!o.d_flags) o.d_flags = h->rw.flagbuf.get();
        if (!o.d_frames) o.d_frames = h->rw.framebuf.get();
        h->rw.flags = o.d_flags;
        h->rw.frames = o.d_frames;
    }
    if (pool && !o.d_flags) o.d_flags = h->pool.flags.get();
    if (int rc = step_impl(h, d_actions, frame_skip, &o)) return rc;
    if (h->rt.cap) {
        ON_DEVICE(h);
        if (int rc = route_append(h, d_actions, 1, frame_skip, o)) return rc;
    }
    if (!pool) return NPP_OK;
    // level pool: the step as without it, then (joined) the draw for the envs whose episode ended -- read from the step's flags
    ON_DEVICE_JOINED(h);
    return pool_redraw(h, o.d_flags, NPP_F_WON | NPP_F_DEAD | NPP_F_TRUNCATED, &o);
}

int npp_step_many(npp_handle h, const uint8_t *d_actions, int n_steps, int frame_skip, const npp_step_out *out) {
    if (!h || !d_actions || frame_skip <= 0 || n_steps <= 0) return fail(h, NPP_ERR_INVALID, "npp_step_many: bad arguments");
    if (h->ls.levels.empty()) return fail(h, NPP_ERR_STATE, "npp_step_many: no levels loaded");
    if (h->goal.on)
        return fail(h, NPP_ERR_STATE, "npp_step_many: the goal curriculum is on and the launch's inner steps have no episode boundary its "
                                      "bookkeeping could see (npp_set_goal_curriculum(h, 0, NULL) first)");
    if (h->rw.mode)
        return fail(h, NPP_ERR_STATE, "npp_step_many: reward mode \"pbrs\" is on and the launch's inner steps have no observation "
                                      "(npp_set_reward_mode(h, 0, NULL) first)");
    ON_DEVICE_JOINED(h);
    KernelArgs a = base_args(h);
    a.inputs = d_actions;
    a.n_ticks = frame_skip;
    a.n_steps = n_steps;
    a.mode = 0;
    h->pm.flags = nullptr;   // (action masking) several steps: no single flags row describes the observation
    npp_step_out o;
    if (h->rt.cap) {   // action routes: the append walks the launch's n_steps flags / frames rows
        std::memset(&o, 0, sizeof(o));
        if (out) o = *out;
        if (int rc = route_rows(h, o, n_steps)) return rc;
        out = &o;
    }
    if (int rc = fill_obs_out(h, a, out)) return rc;
    a.out.terminal_state = nullptr;   // pre-reset observations exist for single steps only
    HIP_TRY(h, launch_step(a, h->stream));
    if (h->rt.cap) return route_append(h, d_actions, n_steps, frame_skip, o);
    return NPP_OK;
}

int npp_tick(npp_handle h, const uint8_t *d_inputs, int n_ticks) {
    if (!h || !d_inputs || n_ticks <= 0) return fail(h, NPP_ERR_INVALID, "npp_tick: bad arguments");
    if (h->ls.levels.empty()) return fail(h, NPP_ERR_STATE, "npp_tick: no levels loaded");
    ON_DEVICE_JOINED(h);
    KernelArgs a = base_args(h);
    a.inputs = d_inputs;
    a.n_ticks = n_ticks;
    a.mode = 1;
    a.autoreset = 0;
    HIP_TRY(h, launch_step(a, h->stream));
    if (int rc = episode_event(h, EP_EV_TICK, nullptr)) return rc;   // (episode statistics) the current episodes hold frames no row counted
    return route_event(h, ROUTE_EV_TICK, nullptr);   // (action routes) raw input bytes: the current routes no longer lead here
}

int npp_observe(npp_handle h, const npp_step_out *out) {
    if (!h || !out) return fail(h, NPP_ERR_INVALID, "npp_observe: bad arguments");
    if (h->ls.levels.empty()) return fail(h, NPP_ERR_STATE, "npp_observe: no levels loaded");
    ON_DEVICE_JOINED(h);
    KernelArgs a = base_args(h);
    a.n_ticks = 0;
    a.mode = 0;
    a.autoreset = 0;
    if (int rc = fill_obs_out(h, a, out)) return rc;
    HIP_TRY(h, launch_step(a, h->stream));
    return NPP_OK;
}

}  // extern "C"

namespace {
// player_frame of every env into d_out + env * stride (and, with mirror != 0, also mirror bytes further on)
int render_player_frame(npp_handle h, uint8_t *d_out, uint32_t stride, uint32_t mirror) {
    if (h->ls.levels.empty()) return fail(h, NPP_ERR_STATE, "npp_render_player_frame: no levels loaded");
    ON_DEVICE(h);
    bool tables = !h->ls.canvas;   // (observation overlap) something the second stream has to wait for was put on the caller's stream
    if (int rc = ensure_canvas(h)) return rc;
    KernelArgs a = base_args(h);
    {   // heavy-first env order, rebuilt from the last launch's per-env clocks on every 8th launch
        Orders &o = h->ord;
        if (!o.pf_order) {
            HIP_TRY(h, o.pf_order.alloc(h->n));
            HIP_TRY(h, o.pf_cost.alloc(h->n));
            HIP_TRY(h, hipMemsetAsync(o.pf_cost.get(), 0, o.pf_cost.bytes(), h->stream));
            o.pf_launches = 0;
        }
        if (o.pf_launches % 8 < 2) {
            HIP_TRY(h, launch_cost_order(o.pf_cost.get(), o.pf_order.get(), h->n, h->stream));
            tables = true;
        }
        o.pf_launches++;
        a.wg_order = o.pf_order.get();
        a.wg_cost = o.pf_cost.get();
    }
    const int centered = (h->flags & NPP_FLAG_FRAME_CENTERED) ? 1 : 0;
    return obs_launch(h, a, true, tables,
                      [&](const KernelArgs &ka, hipStream_t st) { return launch_render(ka, d_out, centered, st, stride, mirror); });
}
}  // namespace

extern "C" {

int npp_render_player_frame(npp_handle h, uint8_t *d_out) {
    if (!h || !d_out) return fail(h, NPP_ERR_INVALID, "npp_render_player_frame: bad arguments");
    h->aug.pf_out = d_out;   // (frame augmentation reads the unstacked frame there)
    return render_player_frame(h, d_out, 84 * 84, 0);
}

int npp_set_frame_stack(npp_handle h, int visual_k, int state_k, int padding) {
    if (!h || visual_k < 0 || visual_k > 12 || state_k < 0 || state_k > 12 || padding < 0 || padding > 1)
        return fail(h, NPP_ERR_INVALID, "npp_set_frame_stack: stack sizes must be 0 (off) or 1..12 and padding 0 (zero) or 1 (repeat)");
    ON_DEVICE_JOINED(h);
    HIP_TRY(h, hipStreamSynchronize(h->stream));   // the old rings may still be read by queued work
    FrameStack &fs = h->fs;
    fs = FrameStack();
    const size_t N = (size_t)h->n;
    if (visual_k) {
        HIP_TRY(h, fs.frames.alloc(N * 2 * visual_k * 84 * 84));
        HIP_TRY(h, hipMemsetAsync(fs.frames.get(), 0, fs.frames.bytes(), h->stream));
    }
    if (state_k) {
        HIP_TRY(h, fs.state.alloc(N * 2 * state_k * NPP_GAME_STATE_DIM));
        HIP_TRY(h, hipMemsetAsync(fs.state.get(), 0, fs.state.bytes(), h->stream));
    }
    fs.vk = visual_k; fs.sk = state_k; fs.repeat = padding;
    fs.vhead = visual_k ? visual_k - 1 : 0;   // the first push completes position 0
    fs.shead = state_k ? state_k - 1 : 0;
    return NPP_OK;
}

int npp_frame_stack_render(npp_handle h) {
    if (!h) return NPP_ERR_INVALID;
    if (!h->fs.vk) return fail(h, NPP_ERR_STATE, "npp_frame_stack_render: visual stacking is off (npp_set_frame_stack)");
    const int K = h->fs.vk, q = (h->fs.vhead + 1) % K;
    const uint32_t slot = 84 * 84, stride = (uint32_t)(2 * K) * slot;
    // position q lives in slots q and q + K; slot 0 is never inside a window, so position 0 is written once
    uint8_t *dst = h->fs.frames.get() + (size_t)(q ? q : K) * slot;
    return render_player_frame(h, dst, stride, q ? (uint32_t)K * slot : 0u);
}

int npp_frame_stack_push(npp_handle h, const float *d_game_state, const float *d_terminal_state, const uint8_t *d_flags,
                         int reset_bits, int reset_all, float *d_terminal_stack) {
    if (!h || !d_game_state || (!reset_all && reset_bits && !d_flags) || (d_terminal_stack && !d_terminal_state))
        return fail(h, NPP_ERR_INVALID, "npp_frame_stack_push: bad arguments");
    if (!h->fs.vk && !h->fs.sk) return fail(h, NPP_ERR_STATE, "npp_frame_stack_push: frame stacking is off (npp_set_frame_stack)");
    if (d_terminal_stack && !h->fs.sk) return fail(h, NPP_ERR_STATE, "npp_frame_stack_push: a terminal stack needs state stacking");
    ON_DEVICE_JOINED(h);
    if (h->fs.vk) h->fs.vhead = (h->fs.vhead + 1) % h->fs.vk;
    if (h->fs.sk) h->fs.shead = (h->fs.shead + 1) % h->fs.sk;
    StackArgs a;
    a.n = h->n;
    a.visual_k = h->fs.vk; a.state_k = h->fs.sk;
    a.vhead = h->fs.vhead; a.shead = h->fs.shead;
    a.repeat = h->fs.repeat;
    a.reset_bits = d_flags ? reset_bits : 0;
    a.reset_all = reset_all ? 1 : 0;
    a.flags = d_flags;
    a.game_state = d_game_state;
    a.terminal_state = d_terminal_state;
    a.frames = h->fs.frames.get();
    a.state = h->fs.state.get();
    a.terminal_stack = d_terminal_stack;
    HIP_TRY(h, launch_stack_push(a, h->stream));
    return NPP_OK;
}

int npp_frame_stack_view(npp_handle h, int which, void **base, int64_t *offset, int64_t *batch_stride) {
    if (!h || (which != 0 && which != 1) || !base || !offset || !batch_stride) return fail(h, NPP_ERR_INVALID, "npp_frame_stack_view: bad arguments");
    const int K = which == 0 ? h->fs.vk : h->fs.sk;
    if (!K) return fail(h, NPP_ERR_STATE, "npp_frame_stack_view: that stack is off (npp_set_frame_stack)");
    const int64_t E = which == 0 ? 84 * 84 : NPP_GAME_STATE_DIM;
    const int head = which == 0 ? h->fs.vhead : h->fs.shead;
    *base = which == 0 ? (void *)h->fs.frames.get() : (void *)h->fs.state.get();
    *offset = (int64_t)(head + 1) * E;
    *batch_stride = (int64_t)2 * K * E;
    return NPP_OK;
}

int npp_set_frame_augmentation(npp_handle h, int enable, double p, double scale, uint64_t seed) {
    if (!h) return NPP_ERR_INVALID;
    FrameAug &A = h->aug;
    if (!enable) {
        if (!A.on && !A.pf) return NPP_OK;
        ON_DEVICE_JOINED(h);
        HIP_TRY(h, hipStreamSynchronize(h->stream));   // the buffers may still be written by a queued call
        A.on = false;
        A.pf.reset(); A.gv.reset(); A.params.reset();
        return NPP_OK;
    }
    if (!(p >= 0.0 && p <= 1.0)) return fail(h, NPP_ERR_INVALID, "npp_set_frame_augmentation: p must be between 0.0 and 1.0");
    const int s10 = scale == 0.7 ? 7 : scale == 1.0 ? 10 : scale == 1.3 ? 13 : 0;
    if (!s10) return fail(h, NPP_ERR_INVALID, "npp_set_frame_augmentation: scale must be 0.7 (light), 1.0 (medium) or 1.3 (strong)");
    if (!(h->fs.vk || A.pf_out) || !A.gv_out)
        return fail(h, NPP_ERR_INVALID, "npp_set_frame_augmentation: the handle has no visual outputs (render player_frame, or stack it, "
                                        "and global_view first)");
    ON_DEVICE_JOINED(h);
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    const size_t N = (size_t)h->n;
    const int k = h->fs.vk ? h->fs.vk : 1;
    A.on = false;
    if (A.pf.size() != N * k * NPP_FRAME_H * NPP_FRAME_W) HIP_TRY(h, A.pf.alloc(N * k * NPP_FRAME_H * NPP_FRAME_W));
    if (!A.gv) HIP_TRY(h, A.gv.alloc(N * AUG_GV_H * AUG_GV_W));
    HIP_TRY(h, hipMemsetAsync(A.pf.get(), 0, A.pf.bytes(), h->stream));
    HIP_TRY(h, hipMemsetAsync(A.gv.get(), 0, A.gv.bytes(), h->stream));
    A.k = k; A.p = p; A.s10 = s10; A.seed = seed; A.count = 0;
    A.on = true;
    return NPP_OK;
}

int npp_frame_augment(npp_handle h, const int32_t *host_params) {
    if (!h) return NPP_ERR_INVALID;
    FrameAug &A = h->aug;
    if (!A.on) return fail(h, NPP_ERR_STATE, "npp_frame_augment: frame augmentation is off (npp_set_frame_augmentation)");
    if (A.k != (h->fs.vk ? h->fs.vk : 1))
        return fail(h, NPP_ERR_STATE, "npp_frame_augment: the visual stack changed since npp_set_frame_augmentation (call it again)");
    const uint8_t *pf_src = h->fs.vk ? h->fs.frames.get() + (size_t)(h->fs.vhead + 1) * NPP_FRAME_H * NPP_FRAME_W : A.pf_out;
    if (!pf_src || !A.gv_out) return fail(h, NPP_ERR_STATE, "npp_frame_augment: nothing was rendered since the outputs changed");
    if (((uintptr_t)pf_src | (uintptr_t)A.gv_out) & 15)
        return fail(h, NPP_ERR_INVALID, "npp_frame_augment: the rendered player_frame / global_view buffers must be 16-byte aligned");
    const size_t N = (size_t)h->n;
    if (host_params) {
        const AugParams *P = reinterpret_cast<const AugParams *>(host_params);
        for (size_t i = 0; i < 2 * N; i++)
            if (!aug_params_ok(P[i], (i & 1) ? AUG_GV_H : AUG_PF_H, (i & 1) ? AUG_GV_W : AUG_PF_W))
                return fail(h, NPP_ERR_INVALID, "npp_frame_augment: parameters of env " + std::to_string(i / 2) + ", target " +
                                                    std::to_string(i & 1) + " are outside the image or the arithmetic's range");
    }
    ON_DEVICE_JOINED(h);
    if (host_params) {
        if (!A.params) HIP_TRY(h, A.params.alloc(2 * N * AUG_WORDS));
        HIP_TRY(h, hipMemcpyAsync(A.params.get(), host_params, A.params.bytes(), hipMemcpyHostToDevice, h->stream));
    }
    AugArgs a;
    a.n = h->n;
    a.k = A.k;
    a.pf_src = pf_src;
    a.pf_stride = (size_t)(h->fs.vk ? 2 * h->fs.vk : 1) * NPP_FRAME_H * NPP_FRAME_W;
    a.gv_src = A.gv_out;
    a.pf_dst = A.pf.get();
    a.gv_dst = A.gv.get();
    a.params = host_params ? A.params.get() : nullptr;
    a.seed = A.seed;
    a.count = A.count;
    a.p = A.p;
    a.s10 = A.s10;
    HIP_TRY(h, launch_frame_augment(a, h->stream));
    A.count++;
    if (host_params) HIP_TRY(h, hipStreamSynchronize(h->stream));   // host_params is caller memory: finish the copy
    return NPP_OK;
}

int npp_frame_augment_view(npp_handle h, int which, void **base, int64_t *bytes) {
    if (!h || (which != 0 && which != 1) || !base || !bytes) return fail(h, NPP_ERR_INVALID, "npp_frame_augment_view: bad arguments");
    if (!h->aug.on) return fail(h, NPP_ERR_STATE, "npp_frame_augment_view: frame augmentation is off (npp_set_frame_augmentation)");
    const DevBuf<uint8_t> &b = which == 0 ? h->aug.pf : h->aug.gv;
    *base = (void *)b.get();
    *bytes = (int64_t)b.bytes();
    return NPP_OK;
}

int npp_set_entity_pos(npp_handle h, int env, int kind, double x, double y) {
    if (!h || env < 0 || env >= h->n || (kind != 0 && kind != 1)) return fail(h, NPP_ERR_INVALID, "npp_set_entity_pos: bad arguments");
    if (h->ls.levels.empty()) return fail(h, NPP_ERR_STATE, "npp_set_entity_pos: no levels loaded");
    if (h->pool.on) return fail(h, NPP_ERR_STATE, "npp_set_entity_pos: the level pool is on (npp_set_level_pool)");
    if (h->sweep.on && x == x && y == y) return fail(h, NPP_ERR_STATE, "npp_set_entity_pos: an evaluation sweep is running (npp_sweep_stop first)");
    if (h->ar.n_slots && x == x && y == y) return fail(h, NPP_ERR_STATE, "npp_set_entity_pos: a checkpoint archive exists (npp_archive_create)");
    {
        ON_DEVICE_JOINED(h);
        if (int rc = pull_levels(h)) return rc;
    }
    const CompiledLevel &L = h->ls.levels[h->env_level[env]];
    if (L.obs_switch < 0) return fail(h, NPP_ERR_STATE, "npp_set_entity_pos: the env's level has no exit switch / door");
    ON_DEVICE_JOINED(h);
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    double *blk = h->ls.zoo.get() + (size_t)env * h->ls.zoo_words;
    uint64_t w3 = 0;
    HIP_TRY(h, hipMemcpy(&w3, blk + 3, 8, hipMemcpyDeviceToHost));
    const bool clear = !(x == x) || !(y == y);   // NaN clears the override
    const uint32_t bit = kind == 0 ? ZOO_OVR_SWITCH : ZOO_OVR_DOOR;
    uint32_t flags = (uint32_t)w3;
    flags = clear ? (flags & ~bit) : (flags | bit);
    w3 = (w3 & 0xffffffff00000000ull) | flags;
    HIP_TRY(h, hipMemcpy(blk + 3, &w3, 8, hipMemcpyHostToDevice));
    if (!clear) {
        double xy[2] = {x, y};
        HIP_TRY(h, hipMemcpy(blk + (kind == 0 ? 4 : 6), xy, 16, hipMemcpyHostToDevice));
    }
    const uint8_t before = h->ovr[env];
    h->ovr[env] = (uint8_t)flags;
    h->n_ovr += (flags != 0) - (before != 0);
    plan_geometry(h);
    return NPP_OK;
}

int npp_switch_states(npp_handle h, float *d_out) {
    if (!h || !d_out) return fail(h, NPP_ERR_INVALID, "npp_switch_states: bad arguments");
    if (h->ls.levels.empty()) return fail(h, NPP_ERR_STATE, "npp_switch_states: no levels loaded");
    ON_DEVICE(h);
    KernelArgs a = base_args(h);
    return obs_launch(h, a, false, false, [&](const KernelArgs &ka, hipStream_t st) { return launch_switch_states(ka, d_out, st); });
}

int npp_reachability(npp_handle h, float *d_features, float *d_mine_sdf, int32_t *d_status) {
    return npp_reachability_ex(h, d_features, d_mine_sdf, d_status, nullptr);
}

int npp_reachability_ex(npp_handle h, float *d_features, float *d_mine_sdf, int32_t *d_status, float *d_switch_states) {
    if (!h || (!d_features && !d_mine_sdf)) return fail(h, NPP_ERR_INVALID, "npp_reachability: bad arguments");
    if (h->ls.levels.empty()) return fail(h, NPP_ERR_STATE, "npp_reachability: no levels loaded");
    if (h->n_ovr) return fail(h, NPP_ERR_UNSUPPORTED, "npp_reachability: exit switch / door repositioned with npp_set_entity_pos");
    ON_DEVICE(h);
    const bool tables = !h->ls.reach.hdr;
    if (int rc = ensure_reach(h)) return rc;
    KernelArgs a = base_args(h);
    const Reach &r = h->ls.reach;
    return obs_launch(h, a, false, tables, [&](const KernelArgs &ka, hipStream_t st) {   // (tables: ensure_reach has just built them)
        return launch_reach(ka, r.hdr.get(), r.blob.get(), r.key.get(), r.cache.get(), r.miss(), d_features, d_mine_sdf, d_status, d_switch_states,
                            nullptr, nullptr, st);
    });
}

int npp_set_minimal_observation(npp_handle h, int enable) {
    if (!h) return NPP_ERR_INVALID;
    h->mini.on = enable != 0;
    h->mini.rows = nullptr;   // the next step / observe launch says where the rows are
    return NPP_OK;
}

int npp_minimal_observation(npp_handle h, float *d_out, int32_t *d_status) {
    if (!h || !d_out) return fail(h, NPP_ERR_INVALID, "npp_minimal_observation: bad arguments");
    if (h->ls.levels.empty()) return fail(h, NPP_ERR_STATE, "npp_minimal_observation: no levels loaded");
    if (!h->mini.on) return fail(h, NPP_ERR_STATE, "npp_minimal_observation: switch the mode on first (npp_set_minimal_observation)");
    if (!h->mini.rows)
        return fail(h, NPP_ERR_STATE, "npp_minimal_observation: no npp_step / npp_observe since the mode was switched on (they write the mine rows)");
    if (h->n_ovr) return fail(h, NPP_ERR_UNSUPPORTED, "npp_reachability: exit switch / door repositioned with npp_set_entity_pos");
    ON_DEVICE(h);
    const bool tables = !h->ls.reach.hdr;
    if (int rc = ensure_reach(h)) return rc;   // (refuses what npp_reachability refuses, with its message)
    KernelArgs a = base_args(h);
    const Reach &r = h->ls.reach;
    const float *rows = h->mini.rows;
    return obs_launch(h, a, false, tables, [&](const KernelArgs &ka, hipStream_t st) {
        return launch_reach(ka, r.hdr.get(), r.blob.get(), r.key.get(), r.cache.get(), r.miss(), nullptr, nullptr, d_status, nullptr, d_out, rows, st);
    });
}

int npp_set_action_masking(npp_handle h, int mode) {
    if (!h) return fail(nullptr, NPP_ERR_INVALID, "npp_set_action_masking: NULL handle");
    if (mode < 0 || mode > 2) return fail(h, NPP_ERR_INVALID, "npp_set_action_masking: mode must be 0 (off), 1 (hard) or 2 (soft)");
    PathMask &pm = h->pm;
    if (mode && !pm.counters) {
        ON_DEVICE(h);
        DevBuf<uint32_t> c;
        DevBuf<uint8_t> f;
        if (c.alloc(4 * (size_t)h->n) != hipSuccess || f.alloc((size_t)h->n) != hipSuccess) {
            (void)hipGetLastError();
            return fail(h, NPP_ERR_HIP, "npp_set_action_masking: hipMalloc of the counters failed");
        }
        HIP_TRY(h, hipMemsetAsync(c.get(), 0, c.bytes(), h->stream));
        HIP_TRY(h, hipMemsetAsync(f.get(), 0, f.bytes(), h->stream));
        pm.counters = std::move(c);
        pm.flagbuf = std::move(f);
    }
    if (!mode || !pm.mode) pm.flags = nullptr;   // off, or on again: no step of this mode has run
    if (mode && !pm.mode) {   // off -> on: observations went by uncounted, so the live counters restart (the latched ones stay)
        ON_DEVICE(h);
        HIP_TRY(h, hipMemsetAsync(pm.plane(0, h->n), 0, 2 * (size_t)h->n * sizeof(uint32_t), h->stream));
    }
    pm.mode = mode;
    return NPP_OK;
}

int npp_path_action_mask(npp_handle h, int8_t *d_action_mask, int8_t *d_direction, int32_t *d_status) {
    if (!h) return fail(nullptr, NPP_ERR_INVALID, "npp_path_action_mask: NULL handle");
    PathMask &pm = h->pm;
    if (!pm.mode) return fail(h, NPP_ERR_STATE, "npp_path_action_mask: action masking is off (npp_set_action_masking)");
    if (pm.mode == 1 && !d_action_mask) return fail(h, NPP_ERR_INVALID, "npp_path_action_mask: hard mode needs d_action_mask");
    if (h->ls.levels.empty()) return fail(h, NPP_ERR_STATE, "npp_path_action_mask: no levels loaded");
    if (h->n_ovr) return fail(h, NPP_ERR_UNSUPPORTED, "npp_path_action_mask: exit switch / door repositioned with npp_set_entity_pos");
    ON_DEVICE_JOINED(h);
    if (int rc = ensure_reach(h)) return rc;   // (refuses what npp_reachability refuses, with its message; built on the first call)
    const LevelSet &L = h->ls;
    PathMaskArgs a{};
    a.n = h->n;
    a.f64 = h->env.f64.get();
    a.ent_bits = L.ent.get();
    a.env_level = h->env.level.get();
    a.hdr = L.hdr.get();
    a.rh = L.reach.hdr.get();
    a.rblob = L.reach.blob.get();
    a.flags = pm.flags;
    a.end_bits = (h->flags & NPP_FLAG_AUTORESET) ? (int)(NPP_F_WON | NPP_F_DEAD | NPP_F_TRUNCATED) : 0;
    a.mask = pm.mode == 1 ? d_action_mask : nullptr;
    a.dir = d_direction;
    a.status = d_status;
    a.observed = pm.plane(0, h->n); a.applied = pm.plane(1, h->n);
    a.last_observed = pm.plane(2, h->n); a.last_applied = pm.plane(3, h->n);
    HIP_TRY(h, launch_path_mask(a, h->stream));
    pm.flags = nullptr;   // consumed: a second call before the next step latches nothing
    return NPP_OK;
}

int npp_path_mask_stats_view(npp_handle h, const uint32_t **d_observed, const uint32_t **d_applied, const uint32_t **d_last_observed,
                             const uint32_t **d_last_applied) {
    if (!h) return fail(nullptr, NPP_ERR_INVALID, "npp_path_mask_stats_view: NULL handle");
    if (!h->pm.counters) return fail(h, NPP_ERR_STATE, "npp_path_mask_stats_view: action masking was never switched on (npp_set_action_masking)");
    if (d_observed) *d_observed = h->pm.plane(0, h->n);
    if (d_applied) *d_applied = h->pm.plane(1, h->n);
    if (d_last_observed) *d_last_observed = h->pm.plane(2, h->n);
    if (d_last_applied) *d_last_applied = h->pm.plane(3, h->n);
    return NPP_OK;
}

int npp_set_reward_params(npp_handle h, const NppRewardParams *params) {
    if (!h) return fail(nullptr, NPP_ERR_INVALID, "npp_set_reward_params: NULL handle");
    NppRewardParams q;
    if (params) q = *params; else npp_reward_default_params(&q);
    const double v[6] = {q.death_penalty, q.level_completion_reward, q.switch_activation_reward, q.time_penalty_per_step,
                         q.pbrs_objective_weight, q.pbrs_gamma};
    for (double x : v)
        if (!std::isfinite(x)) return fail(h, NPP_ERR_INVALID, "npp_set_reward_params: non-finite value");
    h->rw.params = q;
    return NPP_OK;
}

int npp_set_reward_mode(npp_handle h, int mode, const NppRewardParams *params) {
    if (!h) return fail(nullptr, NPP_ERR_INVALID, "npp_set_reward_mode: NULL handle");
    if (mode < 0 || mode > 1) return fail(h, NPP_ERR_INVALID, "npp_set_reward_mode: mode must be 0 (sparse) or 1 (pbrs)");
    Reward &w = h->rw;
    if (!mode) {
        w.mode = 0;
        w.wp_on = 0;
        w.flags = nullptr; w.frames = nullptr;
        return NPP_OK;
    }
    if (h->ls.levels.empty()) return fail(h, NPP_ERR_STATE, "npp_set_reward_mode: no levels loaded");
    if (h->n_ovr) return fail(h, NPP_ERR_UNSUPPORTED, "npp_set_reward_mode: exit switch / door repositioned with npp_set_entity_pos");
    if (int rc = npp_set_reward_params(h, params)) return rc;
    ON_DEVICE_JOINED(h);
    std::vector<ReachBuilt> built;   // every level's host tables, built ONCE: by ensure_reach when it builds, else below
    if (int rc = ensure_reach(h, &built)) return rc;   // (refuses what npp_reachability refuses, with its message)
    const size_t N = (size_t)h->n, nl = h->ls.levels.size();
    if (!w.levels) {
        std::vector<RewardLevel> rl(nl);
        bool any_miss = false;
        ReachBuilt one;
        for (size_t i = 0; i < nl; i++) {
            if (built.empty()) build_reach(h->ls.levels[i], one);
            const ReachBuilt &R = built.empty() ? one : built[i];
            std::string note;
            if (!reward_level_constants(h->ls.levels[i], R, rl[i], note))
                return fail(h, NPP_ERR_UNSUPPORTED, "npp_set_reward_mode: level " + std::to_string(i) + ": " + note + " (DESIGN.md 20)");
            any_miss = any_miss || R.hdr.miss_exit;
        }
        Reward t;   // complete or not at all
        HIP_TRY(h, t.levels.alloc(nl));
        HIP_TRY(h, hipMemcpy(t.levels.get(), rl.data(), t.levels.bytes(), hipMemcpyHostToDevice));
        HIP_TRY(h, t.sd.alloc((size_t)RW_ND * N));
        HIP_TRY(h, t.si.alloc((size_t)RW_NI * N));
        HIP_TRY(h, t.flagbuf.alloc(N));
        HIP_TRY(h, t.framebuf.alloc(N));
        if (any_miss) {
            HIP_TRY(h, t.stamp2.alloc(REACH_CELLS * N));
            HIP_TRY(h, hipMemset(t.stamp2.get(), 0, t.stamp2.bytes()));
            HIP_TRY(h, t.raw2.alloc(REACH_CELLS * N));
        }
        t.params = w.params;
        w = std::move(t);
    }
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (w.stamp2) HIP_TRY(h, hipMemset(w.stamp2.get(), 0, w.stamp2.bytes()));   // (every env's epoch restarts at 1 below)
    w.mode = 1;
    return reward_restart(h, nullptr, nullptr, nullptr, 0, 1);   // switching on resets all reward state
}

namespace {
int waypoint_params_check(npp_handle h, const char *who, const NppWaypointParams &q) {
    const double v[4] = {q.collection_radius, q.out_of_order_scale, q.progress_scale, q.progress_spacing};
    for (double x : v)
        if (!std::isfinite(x)) return fail(h, NPP_ERR_INVALID, std::string(who) + ": non-finite value");
    if (!(q.collection_radius >= 0.0) || q.collection_radius > WP_MAX_RADIUS)
        return fail(h, NPP_ERR_INVALID, std::string(who) + ": collection_radius must lie in [0, 24] (the kernel walks the 3 x 3 cells of 24 px around the ninja)");
    if (!(q.progress_spacing > 0.0)) return fail(h, NPP_ERR_INVALID, std::string(who) + ": progress_spacing must be positive");
    return NPP_OK;
}
}  // namespace

int npp_set_waypoint_params(npp_handle h, const NppWaypointParams *params) {
    if (!h) return fail(nullptr, NPP_ERR_INVALID, "npp_set_waypoint_params: NULL handle");
    NppWaypointParams q;
    if (params) q = *params; else npp_waypoint_default_params(&q);
    q.progress_spacing = h->rw.wp_hdr ? h->rw.wp_params.progress_spacing : 12.0;   // takes effect in npp_set_reward_waypoints only
    if (int rc = waypoint_params_check(h, "npp_set_waypoint_params", q)) return rc;
    h->rw.wp_params = q;
    return NPP_OK;
}

int npp_set_reward_waypoints(npp_handle h, int on, const NppWaypointParams *params) {
    if (!h) return fail(nullptr, NPP_ERR_INVALID, "npp_set_reward_waypoints: NULL handle");
    Reward &w = h->rw;
    if (on && h->goal.on)
        return fail(h, NPP_ERR_STATE, "npp_set_reward_waypoints: the goal curriculum is on and the waypoints towards the moved goals are not "
                                      "computed (npp_set_goal_curriculum(h, 0, NULL) first)");
    if (!w.mode) return fail(h, NPP_ERR_STATE, "npp_set_reward_waypoints: reward mode \"pbrs\" is off (npp_set_reward_mode)");
    if (!on) {
        w.wp_on = 0;
        return NPP_OK;
    }
    if (h->n_ovr) return fail(h, NPP_ERR_UNSUPPORTED, "npp_set_reward_waypoints: exit switch / door repositioned with npp_set_entity_pos");
    NppWaypointParams q;
    if (params) q = *params; else npp_waypoint_default_params(&q);
    if (int rc = waypoint_params_check(h, "npp_set_reward_waypoints", q)) return rc;
    ON_DEVICE_JOINED(h);
    const size_t N = (size_t)h->n, nl = h->ls.levels.size();
    std::vector<WaypointHdr> hdr(nl);
    std::vector<unsigned char> blob;
    std::vector<std::vector<uint32_t>> recs(nl);
    ReachBuilt R;
    for (size_t i = 0; i < nl; i++) {
        build_reach(h->ls.levels[i], R);
        WaypointBuilt W;
        std::string note;
        if (!build_waypoints(h->ls.levels[i], R, q.progress_spacing, W, note))
            return fail(h, NPP_ERR_UNSUPPORTED, "npp_set_reward_waypoints: level " + std::to_string(i) + ": " + note + " (DESIGN.md 23)");
        pack_waypoints(W, hdr[i], blob);
        recs[i] = W.rec;
    }
    if (blob.empty()) blob.resize(4, 0);
    // complete or not at all
    DevBuf<WaypointHdr> d_hdr;
    DevBuf<unsigned char> d_blob;
    HIP_TRY(h, d_hdr.alloc(nl));
    HIP_TRY(h, d_blob.alloc(blob.size()));
    if (!w.wp_state) {
        DevBuf<uint32_t> st;
        DevBuf<double> bonus;
        HIP_TRY(h, st.alloc((size_t)WP_NI * N));
        HIP_TRY(h, bonus.alloc(N));
        w.wp_state = std::move(st);
        w.wp_bonus = std::move(bonus);
    }
    HIP_TRY(h, hipStreamSynchronize(h->stream));   // (a launch in flight may still read the old tables)
    HIP_TRY(h, hipMemcpy(d_hdr.get(), hdr.data(), d_hdr.bytes(), hipMemcpyHostToDevice));
    HIP_TRY(h, hipMemcpy(d_blob.get(), blob.data(), d_blob.bytes(), hipMemcpyHostToDevice));
    w.wp_hdr = std::move(d_hdr);
    w.wp_blob = std::move(d_blob);
    w.wp_rec = std::move(recs);
    w.wp_params = q;
    w.wp_on = 1;
    HIP_TRY(h, launch_waypoint_restart(waypoint_args(h), h->stream));   // switching on empties every env's collection state
    return NPP_OK;
}

int npp_reward_waypoints(npp_handle h, int level, double *out_xy, uint8_t *out_phase, int cap, int32_t *count) {
    if (!h) return fail(nullptr, NPP_ERR_INVALID, "npp_reward_waypoints: NULL handle");
    const Reward &w = h->rw;
    if (!w.wp_on) return fail(h, NPP_ERR_STATE, "npp_reward_waypoints: the path waypoints are off (npp_set_reward_waypoints)");
    if (level < 0 || (size_t)level >= w.wp_rec.size() || cap < 0 || !count) return fail(h, NPP_ERR_INVALID, "npp_reward_waypoints: bad level, cap or count");
    const std::vector<uint32_t> &r = w.wp_rec[(size_t)level];
    *count = (int32_t)r.size();
    for (size_t i = 0; i < r.size() && i < (size_t)cap; i++) {
        if (out_xy) { out_xy[2 * i] = (double)(r[i] & 0xfffu); out_xy[2 * i + 1] = (double)((r[i] >> 12) & 0xfffu); }
        if (out_phase) out_phase[i] = (uint8_t)((r[i] >> 24) & 1u);
    }
    return NPP_OK;
}

int npp_step_reward(npp_handle h, float *d_reward, float *d_components, int32_t *d_status) {
    return npp_step_reward_wp(h, d_reward, d_components, d_status, nullptr, nullptr);
}

int npp_step_reward_wp(npp_handle h, float *d_reward, float *d_components, int32_t *d_status, float *d_wp_bonus, int32_t *d_wp_info) {
    if (!h) return fail(nullptr, NPP_ERR_INVALID, "npp_step_reward: NULL handle");
    Reward &w = h->rw;
    if (!w.mode) return fail(h, NPP_ERR_STATE, "npp_step_reward: reward mode \"pbrs\" is off (npp_set_reward_mode)");
    if (!d_reward) return fail(h, NPP_ERR_INVALID, "npp_step_reward: d_reward is NULL");
    if (h->n_ovr) return fail(h, NPP_ERR_UNSUPPORTED, "npp_step_reward: exit switch / door repositioned with npp_set_entity_pos");
    if (!w.flags || !w.frames) return fail(h, NPP_ERR_STATE, "npp_step_reward: no npp_step since the last call (one call per step)");
    ON_DEVICE_JOINED(h);
    if (w.wp_on) {   // the step's waypoint bonus, in front of the reward launch that adds it
        WaypointArgs q = waypoint_args(h);
        q.flags = w.flags;
        q.bonus_out = d_wp_bonus;
        q.info_out = d_wp_info;
        HIP_TRY(h, launch_waypoint(q, h->stream));
    }
    RewardArgs a = reward_args(h);
    a.flags = w.flags;
    a.frames = w.frames;
    a.reward = d_reward;
    a.comps = d_components;
    a.status = d_status;
    HIP_TRY(h, launch_reward(a, h->stream));
    w.flags = nullptr;   // consumed
    w.frames = nullptr;
    return NPP_OK;
}

}  // extern "C"

namespace {
// the features that keep books per step, per reset or per stream part: the player ticks outside all of them
// (npp_archive_seed shares all but the routes, which it writes itself)
const char *player_refusal(npp_handle h) {
    if (h->rw.mode) return "reward mode \"pbrs\" is on (npp_set_reward_mode(h, 0, NULL) first)";
    if (h->pm.mode) return "action masking is on (npp_set_action_masking(h, 0) first)";
    if (h->fs.vk || h->fs.sk) return "frame stacking is on (npp_set_frame_stack(h, 0, 0, 0) first)";
    if (h->pool.on) return "the level pool is on (npp_set_level_pool(h, NULL, 0, 0) first)";
    if (h->goal.on) return "the goal curriculum is on and the replays belong to the base levels (npp_set_goal_curriculum(h, 0, NULL) first)";
    if (h->ov.n_cuts) return "the observation overlap is on (npp_set_obs_overlap(h, 0) first)";
    if (h->sweep.on) return "an evaluation sweep is running (npp_sweep_stop(h) first)";
    return nullptr;
}
const char *demo_refusal(npp_handle h) {
    if (h->rt.cap) return "action routes are on (npp_set_routes(h, 0) first)";
    return player_refusal(h);
}
}  // namespace

extern "C" {

int npp_demo_create(npp_handle h, const uint8_t *inputs, const int64_t *offsets, const int32_t *levels, int n_replays, int frame_skip,
                    int64_t max_transitions, unsigned key_flags) {
    if (!h) return fail(nullptr, NPP_ERR_INVALID, "npp_demo_create: NULL handle");
    if (n_replays <= 0 || !offsets || !levels || (key_flags & ~(unsigned)DEMO_KEYS_ALL))
        return fail(h, NPP_ERR_INVALID, "npp_demo_create: bad arguments");
    if (h->ls.levels.empty()) return fail(h, NPP_ERR_STATE, "npp_demo_create: no levels loaded");
    if (const char *why = demo_refusal(h)) return fail(h, NPP_ERR_STATE, std::string("npp_demo_create: ") + why);
    if (offsets[0] != 0) return fail(h, NPP_ERR_INVALID, "npp_demo_create: offsets[0] must be 0");
    std::vector<int64_t> len((size_t)n_replays);
    for (int r = 0; r < n_replays; r++) {
        len[r] = offsets[r + 1] - offsets[r];   // (a negative one is the plan's to refuse)
        if (levels[r] < 0 || levels[r] >= (int)h->ls.levels.size())
            return fail(h, NPP_ERR_INVALID, "npp_demo_create: replay " + std::to_string(r) + ": level id out of range");
    }
    const int64_t total = offsets[n_replays];
    if (total > 0 && !inputs) return fail(h, NPP_ERR_INVALID, "npp_demo_create: inputs is NULL");
    Demo d;   // complete or not at all
    const char *why = nullptr;
    if (!demo_plan(len.data(), n_replays, frame_skip, max_transitions, h->n, d.plan, &why))
        return fail(h, NPP_ERR_INVALID, std::string("npp_demo_create: ") + why);
    ON_DEVICE_JOINED(h);
    if (key_flags & (DEMO_REACH | DEMO_MINE_SDF)) {   // (refuses what npp_reachability refuses, with its message)
        if (h->n_ovr) return fail(h, NPP_ERR_UNSUPPORTED, "npp_demo_create: exit switch / door repositioned with npp_set_entity_pos");
        if (int rc = ensure_reach(h)) return rc;
    }
    const size_t N = (size_t)h->n, R = (size_t)n_replays, rounds = d.plan.round_ticks.size();
    d.n_replays = n_replays;
    d.fs = frame_skip;
    d.keys = key_flags;
    d.levels.assign(levels, levels + n_replays);
    std::vector<int32_t> slot(std::max<size_t>(rounds, 1) * N, -1);
    for (size_t i = 0; i < d.plan.order.size(); i++) slot[i] = d.plan.order[i];   // round i / N, env i % N
    HIP_TRY(h, d.inputs.alloc((size_t)std::max<int64_t>(total, 1)));
    HIP_TRY(h, d.offsets.alloc(R + 1));
    HIP_TRY(h, d.row_base.alloc(R));
    HIP_TRY(h, d.rows.alloc(R));
    HIP_TRY(h, d.rep_level.alloc(R));
    HIP_TRY(h, d.slot.alloc(slot.size()));
    HIP_TRY(h, d.staging.alloc((size_t)frame_skip * N));
    HIP_TRY(h, d.gs.alloc(N * NPP_GAME_STATE_DIM));
    HIP_TRY(h, d.mask.alloc(N * NPP_ACTION_DIM));
    HIP_TRY(h, d.epos.alloc(N * NPP_ENTITY_POS_DIM));
    HIP_TRY(h, d.flags.alloc(N));
    HIP_TRY(h, d.pos.alloc(N * 6));
    if (key_flags & DEMO_SPATIAL) HIP_TRY(h, d.sc.alloc(N * NPP_SPATIAL_CONTEXT_DIM));
    if (key_flags & DEMO_REACH) HIP_TRY(h, d.reach.alloc(N * REACH_DIM));
    if (key_flags & DEMO_MINE_SDF) HIP_TRY(h, d.sdf.alloc(N * 3));
    if (key_flags & (DEMO_REACH | DEMO_MINE_SDF)) HIP_TRY(h, d.rstatus.alloc(N));
    if (key_flags & DEMO_SWITCH_STATES) HIP_TRY(h, d.sw.alloc(N * 25));
    if (total > 0) HIP_TRY(h, hipMemcpy(d.inputs.get(), inputs, (size_t)total, hipMemcpyHostToDevice));
    HIP_TRY(h, hipMemcpy(d.offsets.get(), offsets, d.offsets.bytes(), hipMemcpyHostToDevice));
    HIP_TRY(h, hipMemcpy(d.row_base.get(), d.plan.row_base.data(), d.row_base.bytes(), hipMemcpyHostToDevice));
    HIP_TRY(h, hipMemcpy(d.rows.get(), d.plan.rows.data(), d.rows.bytes(), hipMemcpyHostToDevice));
    HIP_TRY(h, hipMemcpy(d.rep_level.get(), levels, d.rep_level.bytes(), hipMemcpyHostToDevice));
    HIP_TRY(h, hipMemcpy(d.slot.get(), slot.data(), d.slot.bytes(), hipMemcpyHostToDevice));
    HIP_TRY(h, hipStreamSynchronize(h->stream));   // a queued play of the previous object may still read its tables
    d.on = true;
    h->demo = std::move(d);
    return NPP_OK;
}

int npp_demo_destroy(npp_handle h) {
    if (!h) return fail(nullptr, NPP_ERR_INVALID, "npp_demo_destroy: NULL handle");
    if (!h->demo.on) return NPP_OK;
    ON_DEVICE_JOINED(h);
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    h->demo = Demo();
    return NPP_OK;
}

int npp_demo_rows(npp_handle h, int64_t *rows_total, int32_t *n_rounds, int64_t *ticks_total) {
    if (!h) return fail(nullptr, NPP_ERR_INVALID, "npp_demo_rows: NULL handle");
    if (!h->demo.on) return fail(h, NPP_ERR_STATE, "npp_demo_rows: no demo object (npp_demo_create)");
    const DemoPlan &p = h->demo.plan;
    if (rows_total) *rows_total = p.rows_total;
    if (n_rounds) *n_rounds = (int32_t)p.round_ticks.size();
    if (ticks_total) *ticks_total = std::accumulate(p.round_ticks.begin(), p.round_ticks.end(), (int64_t)0);
    return NPP_OK;
}

int npp_demo_play(npp_handle h, const NppDemoOut *out) {
    if (!h) return fail(nullptr, NPP_ERR_INVALID, "npp_demo_play: NULL handle");
    Demo &d = h->demo;
    if (!d.on) return fail(h, NPP_ERR_STATE, "npp_demo_play: no demo object (npp_demo_create)");
    if (!out) return fail(h, NPP_ERR_INVALID, "npp_demo_play: out is NULL");
    if (const char *why = demo_refusal(h)) return fail(h, NPP_ERR_STATE, std::string("npp_demo_play: ") + why);
    const unsigned k = d.keys;
    if (((k & DEMO_GAME_STATE) && !out->d_game_state) || ((k & DEMO_ACTION_MASK) && !out->d_action_mask) ||
        ((k & DEMO_ENTITY_POS) && !out->d_entity_positions) || ((k & DEMO_SPATIAL) && !out->d_spatial_context) ||
        ((k & DEMO_REACH) && !out->d_reachability_features) || ((k & DEMO_MINE_SDF) && !out->d_mine_sdf_features) ||
        ((k & DEMO_SWITCH_STATES) && !out->d_switch_states) || ((k & DEMO_POSITIONS) && !out->d_positions))
        return fail(h, NPP_ERR_INVALID, "npp_demo_play: a plane of the object's key_flags has no destination");
    ON_DEVICE_JOINED(h);
    const int N = h->n;
    DemoArgs a{};
    a.n = N;
    a.fs = d.fs;
    a.inputs = d.inputs.get();
    a.offsets = d.offsets.get();
    a.rows = d.rows.get();
    a.row_base = d.row_base.get();
    a.rep_level = d.rep_level.get();
    a.staging = d.staging.get();
    a.gs = d.gs.get(); a.epos = d.epos.get(); a.sc = d.sc.get(); a.reach = d.reach.get(); a.sdf = d.sdf.get(); a.sw = d.sw.get();
    a.mask = d.mask.get(); a.flags = d.flags.get(); a.pos = d.pos.get(); a.rstatus = d.rstatus.get();
    a.mask_ones = (k & DEMO_MASK_ENV) ? 0 : 1;
    // a plane that is off has no destination, whatever the caller's struct holds
    a.out.game_state = (k & DEMO_GAME_STATE) ? out->d_game_state : nullptr;
    a.out.action_mask = (k & DEMO_ACTION_MASK) ? out->d_action_mask : nullptr;
    a.out.entity_positions = (k & DEMO_ENTITY_POS) ? out->d_entity_positions : nullptr;
    a.out.spatial_context = (k & DEMO_SPATIAL) ? out->d_spatial_context : nullptr;
    a.out.reachability_features = (k & DEMO_REACH) ? out->d_reachability_features : nullptr;
    a.out.mine_sdf_features = (k & DEMO_MINE_SDF) ? out->d_mine_sdf_features : nullptr;
    a.out.switch_states = (k & DEMO_SWITCH_STATES) ? out->d_switch_states : nullptr;
    a.out.positions = (k & DEMO_POSITIONS) ? out->d_positions : nullptr;
    a.out.action = out->d_action; a.out.frame = out->d_frame; a.out.done = out->d_done; a.out.replay = out->d_replay;
    a.out.level = out->d_level; a.out.flags = out->d_flags; a.out.status = out->d_status;
    npp_step_out so;
    std::memset(&so, 0, sizeof(so));
    so.d_game_state = d.gs.get();
    so.d_action_mask = d.mask.get();
    so.d_entity_pos = d.epos.get();
    so.d_flags = d.flags.get();
    so.d_spatial_context = d.sc.get();
    so.d_positions = d.pos.get();
    std::vector<int32_t> lv((size_t)N);
    if (int rc = episode_event(h, EP_EV_CLEAR, nullptr)) return rc;   // (episode statistics) the player's ticks are nobody's episode
    for (size_t q = 0; q < d.plan.round_ticks.size(); q++) {
        // the round's levels (an env without a replay plays the level of the round's first) and the reference's load: a level
        // assignment plus Simulator.reset.  The assignment is npp_assign_levels' and synchronises as it always does; between
        // here and the end of the round nothing does
        const size_t first = q * (size_t)N;
        for (int e = 0; e < N; e++) {
            const size_t i = first + (size_t)e;
            lv[e] = d.levels[d.plan.order[i < d.plan.order.size() ? i : first]];
        }
        if (int rc = npp_assign_levels(h, nullptr, lv.data(), N)) return rc;
        if (int rc = npp_reset_ex(h, nullptr, 1)) return rc;
        a.slot = d.slot.get() + first;
        const int periods = d.plan.round_ticks[q] / d.fs;
        for (int p = 0; p < periods; p++) {
            a.period = p;
            HIP_TRY(h, launch_demo_feed(a, h->stream));
            if (int rc = npp_tick(h, d.staging.get(), d.fs)) return rc;
            if (int rc = npp_observe(h, &so)) return rc;
            if (k & (DEMO_REACH | DEMO_MINE_SDF)) {
                if (int rc = npp_reachability_ex(h, d.reach.get(), d.sdf.get(), d.rstatus.get(), d.sw.get())) return rc;
            } else if (k & DEMO_SWITCH_STATES) {
                if (int rc = npp_switch_states(h, d.sw.get())) return rc;
            }
            HIP_TRY(h, launch_demo_collect(a, h->stream));
        }
    }
    return episode_event(h, EP_EV_CLEAR, nullptr);
}

int npp_archive_seed(npp_handle h, const uint8_t *inputs, const int64_t *offsets, const int32_t *levels, int n_replays, int score_mode,
                     const float *d_scores, int32_t *d_counts) {
    if (!h) return fail(nullptr, NPP_ERR_INVALID, "npp_archive_seed: NULL handle");
    if (n_replays <= 0 || !offsets || !levels) return fail(h, NPP_ERR_INVALID, "npp_archive_seed: bad arguments");
    if (score_mode != SEED_PROGRESS && score_mode != SEED_FRAMES && score_mode != SEED_TABLE)
        return fail(h, NPP_ERR_INVALID, "npp_archive_seed: score_mode must be 0 (progress), 1 (frames) or 2 (table)");
    if (score_mode == SEED_TABLE && !d_scores) return fail(h, NPP_ERR_INVALID, "npp_archive_seed: score_mode 2 (table) needs d_scores");
    if (h->ls.levels.empty()) return fail(h, NPP_ERR_STATE, "npp_archive_seed: no levels loaded");
    // every refusal comes before the first change: a refused call leaves the handle and the index as they were
    if (h->sweep.on) return fail(h, NPP_ERR_STATE, "npp_archive_seed: an evaluation sweep is running (npp_sweep_stop(h) first)");
    CellArgs c;
    if (int rc = cells_args(h, "npp_archive_seed", c)) return rc;   // (no cell index; the causes npp_archive_explore names)
    if (const char *why = player_refusal(h)) return fail(h, NPP_ERR_STATE, std::string("npp_archive_seed: ") + why);
    if (offsets[0] != 0) return fail(h, NPP_ERR_INVALID, "npp_archive_seed: offsets[0] must be 0");
    std::vector<int64_t> len((size_t)n_replays);
    int64_t longest = 0;
    for (int r = 0; r < n_replays; r++) {
        len[r] = offsets[r + 1] - offsets[r];   // (a negative one is the plan's to refuse)
        longest = std::max(longest, len[r]);
        if (levels[r] < 0 || levels[r] >= (int)h->ls.levels.size())
            return fail(h, NPP_ERR_INVALID, "npp_archive_seed: replay " + std::to_string(r) + ": level id out of range");
    }
    const int64_t total = offsets[n_replays];
    if (total > 0 && !inputs) return fail(h, NPP_ERR_INVALID, "npp_archive_seed: inputs is NULL");
    DemoPlan plan;   // npp_demo_plan_host's, with frame_skip 1 and no cap: a row per tick
    const char *why = nullptr;
    if (!demo_plan(len.data(), n_replays, 1, longest, h->n, plan, &why)) return fail(h, NPP_ERR_INVALID, std::string("npp_archive_seed: ") + why);
    ON_DEVICE_JOINED(h);
    const size_t N = (size_t)h->n, R = (size_t)n_replays, rounds = plan.round_ticks.size();
    if (d_counts) HIP_TRY(h, hipMemsetAsync(d_counts, 0, R * 4 * sizeof(int32_t), h->stream));
    if (rounds == 0) return NPP_OK;   // every replay is empty: nothing to play, nothing changes
    std::vector<int32_t> slot(rounds * N, -1);
    for (size_t i = 0; i < plan.order.size(); i++) slot[i] = plan.order[i];   // round i / N, env i % N
    DevBuf<uint8_t> d_inputs, staging, action, mask, latch;
    DevBuf<int64_t> d_offsets;
    DevBuf<int32_t> d_slot, status;
    DevBuf<float> score;
    HIP_TRY(h, d_inputs.alloc((size_t)std::max<int64_t>(total, 1)));
    HIP_TRY(h, d_offsets.alloc(R + 1));
    HIP_TRY(h, d_slot.alloc(slot.size()));
    HIP_TRY(h, staging.alloc(N));
    HIP_TRY(h, action.alloc(N));
    HIP_TRY(h, mask.alloc(N));
    HIP_TRY(h, latch.alloc(N));
    HIP_TRY(h, status.alloc(N));
    HIP_TRY(h, score.alloc(N));
    if (total > 0) HIP_TRY(h, hipMemcpy(d_inputs.get(), inputs, (size_t)total, hipMemcpyHostToDevice));
    HIP_TRY(h, hipMemcpy(d_offsets.get(), offsets, d_offsets.bytes(), hipMemcpyHostToDevice));
    HIP_TRY(h, hipMemcpy(d_slot.get(), slot.data(), d_slot.bytes(), hipMemcpyHostToDevice));
    SeedArgs s{};
    s.n = h->n;
    s.score_mode = score_mode;
    s.inputs = d_inputs.get();
    s.offsets = d_offsets.get();
    s.scores = d_scores;
    s.staging = staging.get(); s.action = action.get(); s.mask = mask.get(); s.score = score.get(); s.latch = latch.get();
    s.counts = d_counts;
    s.u32 = h->env.u32.get();
    s.ent = h->ls.ent.get();
    s.env_level = h->env.level.get();
    s.hdr = h->ls.hdr.get();
    s.route_hdr = h->rt.hdr.get();
    s.route_act = h->rt.act.get();
    s.cap = h->rt.cap;
    c.score = score_mode == SEED_FRAMES ? nullptr : score.get();   // (frames: the index's own NULL score, read from the state)
    c.mask = mask.get();
    c.status = status.get();
    c.no_count = 1;
    std::vector<int32_t> lv(N);
    if (int rc = episode_event(h, EP_EV_CLEAR, nullptr)) return rc;   // (episode statistics) the player's ticks are nobody's episode
    for (size_t q = 0; q < rounds; q++) {
        // the round's levels and the reference's load, as npp_demo_play does them (the assignment synchronises as it always does;
        // between here and the end of the round nothing does).  Both flip the routes: every env starts the round on an empty one
        const size_t first = q * N;
        for (size_t e = 0; e < N; e++) {
            const size_t i = first + e;
            lv[e] = levels[plan.order[i < plan.order.size() ? i : first]];
        }
        if (int rc = npp_assign_levels(h, nullptr, lv.data(), h->n)) return rc;
        if (int rc = npp_reset_ex(h, nullptr, 1)) return rc;
        s.slot = d_slot.get() + first;
        for (int f = 0; f < plan.round_ticks[q]; f++) {
            s.tick = f;
            s.feed = 1;
            s.status = f > 0 ? status.get() : nullptr;
            HIP_TRY(h, launch_seed_feed(s, h->stream));
            KernelArgs a = base_args(h);   // npp_tick's launch, without its "not replayable" mark on every route
            a.inputs = staging.get();
            a.n_ticks = 1;
            a.mode = 1;
            a.autoreset = 0;
            HIP_TRY(h, launch_step(a, h->stream));
            if (s.cap) HIP_TRY(h, launch_seed_route(s, h->stream));
            if (int rc = explore_launch(h, c)) return rc;
        }
        if (d_counts && plan.round_ticks[q] > 0) {   // the verdicts of the round's last tick
            s.feed = 0;
            s.status = status.get();
            HIP_TRY(h, launch_seed_feed(s, h->stream));
        }
    }
    if (int rc = route_event(h, ROUTE_EV_INIT, nullptr)) return rc;   // the players' routes are nobody's episode
    if (int rc = episode_event(h, EP_EV_CLEAR, nullptr)) return rc;   // ... and so are the current episode records
    HIP_TRY(h, hipStreamSynchronize(h->stream));   // the queued launches read the tables freed here
    return NPP_OK;
}

int npp_graph_observation(npp_handle h, float *d_node_feats, uint16_t *d_edge_index, uint8_t *d_node_mask, uint8_t *d_edge_mask, int flags) {
    if (!h || !d_node_feats || !d_edge_index || !d_node_mask || !d_edge_mask || (flags & ~1))
        return fail(h, NPP_ERR_INVALID, "npp_graph_observation: bad arguments");
    if (((uintptr_t)d_node_feats | (uintptr_t)d_edge_index | (uintptr_t)d_edge_mask) & 15)
        return fail(h, NPP_ERR_INVALID, "npp_graph_observation: node features, edge index and edge mask must be 16-byte aligned");
    if (h->ls.levels.empty()) return fail(h, NPP_ERR_STATE, "npp_graph_observation: no levels loaded");
    if (h->goal.on)
        return fail(h, NPP_ERR_UNSUPPORTED, "npp_graph_observation: the goal curriculum is on and the graph rows on its variant levels are not pinned against the reference "
                                            "(npp_set_goal_curriculum(h, 0, NULL) first)");
    if (h->n_ovr) return fail(h, NPP_ERR_UNSUPPORTED, "npp_graph_observation: an entity is repositioned with npp_set_entity_pos");
    ON_DEVICE_JOINED(h);
    if (int rc = ensure_graph(h)) return rc;
    GraphObs &g = h->ls.graph;
    const void *rows[4] = {d_node_feats, d_edge_index, d_node_mask, d_edge_mask};
    GraphArgs a;
    a.n = h->n;
    a.n_levels = (int)h->ls.levels.size();
    a.all = (flags & 1) || !std::equal(rows, rows + 4, g.rows);
    a.env_level = h->env.level.get();
    a.row_level = g.row_level.get();
    a.hdr = g.hdr.get();
    a.blob = g.blob.get();
    a.feats = d_node_feats;
    a.edges = d_edge_index;
    a.node_mask = d_node_mask;
    a.edge_mask = d_edge_mask;
    HIP_TRY(h, launch_graph_rows(a, h->stream));
    std::copy(rows, rows + 4, g.rows);
    return NPP_OK;
}

int npp_render_frame(npp_handle h, int env0, int count, uint8_t *d_out) {
    if (!h || !d_out || env0 < 0 || count <= 0 || env0 + count > h->n) return fail(h, NPP_ERR_INVALID, "npp_render_frame: bad arguments");
    if (h->ls.levels.empty()) return fail(h, NPP_ERR_STATE, "npp_render_frame: no levels loaded");
    ON_DEVICE_JOINED(h);
    if (int rc = ensure_canvas(h)) return rc;
    KernelArgs a = base_args(h);
    HIP_TRY(h, launch_full_frame(a, env0, count, d_out, h->stream));
    return NPP_OK;
}

int npp_render_global_view(npp_handle h, uint8_t *d_out) {
    if (!h || !d_out) return fail(h, NPP_ERR_INVALID, "npp_render_global_view: bad arguments");
    if (h->ls.levels.empty()) return fail(h, NPP_ERR_STATE, "npp_render_global_view: no levels loaded");
    h->aug.gv_out = d_out;   // (frame augmentation reads global_view there)
    ON_DEVICE(h);
    const bool tables = !h->ls.gv.h || !h->ls.canvas;
    if (int rc = ensure_gv(h)) return rc;
    KernelArgs a = base_args(h);
    int max_records = 0;
    for (const LevelHdr &lh : h->ls.hdrs) max_records = std::max(max_records, (int)(lh.n_door + lh.n_ent + lh.n_mov));
    Orders &o = h->ord;
    const GvTables &t = h->ls.gv;
    const int reorder = (o.gv_launches++ % 4) < 2;   // the order is rebuilt on launches 0, 1, 4, 5, 8, ... (costs exist from launch 1 on)
    if (h->ov.live_parts > 1) {   // one kernel per part of a split step; the order table is rebuilt once, ahead of all of them
        if (reorder) HIP_TRY(h, launch_cost_order(o.gv_cost.get(), o.gv_order.get(), h->n, h->stream));
        return obs_launch(h, a, false, reorder || tables, [&](const KernelArgs &ka, hipStream_t st) {
            return launch_global_view(ka, max_records, t.p.get(), t.h.get(), t.v.get(), d_out, o.gv_order.get(), o.gv_cost.get(), 0, st);
        });
    }
    HIP_TRY(h, launch_global_view(a, max_records, t.p.get(), t.h.get(), t.v.get(), d_out, o.gv_order.get(), o.gv_cost.get(), reorder, h->stream));
    return NPP_OK;
}

int npp_dump_state(npp_handle h, int env0, int count, double *f64_out, int32_t *i32_out) {
    if (!h || env0 < 0 || count <= 0 || env0 + count > h->n) return fail(h, NPP_ERR_INVALID, "npp_dump_state: bad range");
    if (h->ls.levels.empty()) return fail(h, NPP_ERR_STATE, "npp_dump_state: no levels loaded");
    ON_DEVICE_JOINED(h);
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (int rc = pull_levels(h)) return rc;
    size_t N = (size_t)h->n;
    std::vector<double> f((size_t)NF64 * count);
    std::vector<uint32_t> u((size_t)NU32 * count);
    std::vector<uint32_t> w((size_t)h->ls.n_words_max * count);
    for (int k = 0; k < NF64; k++)
        HIP_TRY(h, hipMemcpy(f.data() + (size_t)k * count, h->env.f64.get() + k * N + env0, sizeof(double) * count, hipMemcpyDeviceToHost));
    for (int k = 0; k < NU32; k++)
        HIP_TRY(h, hipMemcpy(u.data() + (size_t)k * count, h->env.u32.get() + k * N + env0, sizeof(uint32_t) * count, hipMemcpyDeviceToHost));
    for (int k = 0; k < h->ls.n_words_max; k++)
        HIP_TRY(h, hipMemcpy(w.data() + (size_t)k * count, h->ls.ent.get() + k * N + env0, sizeof(uint32_t) * count, hipMemcpyDeviceToHost));
    for (int i = 0; i < count; i++) {
        auto F = [&](int k) { return f[(size_t)k * count + i]; };
        uint32_t words[NU32];
        for (int k = 0; k < NU32; k++) words[k] = state_word(u.data(), count, i, k);
        const int gjump = state_get(words, S_GJUMP), dslow = state_get(words, S_DSLOW);
        if (f64_out) {
            double *o = f64_out + (size_t)i * NPP_DUMP_F64;
            o[0] = F(F_X); o[1] = F(F_Y); o[2] = F(F_VX); o[3] = F(F_VY);
            o[4] = F(F_FNX); o[5] = F(F_FNY); o[6] = F(F_CNX); o[7] = F(F_CNY);
            o[8] = F(F_VXO); o[9] = F(F_VYO);
            o[10] = gjump ? 0.01111111111111111 : 0.06666666666666665;
            o[11] = dslow ? 0.8617738760127536 : 0.9933221725495059;
        }
        if (i32_out) {
            const int lvl = h->env_level[env0 + i];
            state_decode_row(words, exit_switch_state(w.data(), count, i, h->ls.levels[lvl].obs_switch), lvl, i32_out + (size_t)i * NPP_DUMP_I32);
        }
    }
    return NPP_OK;
}

int npp_set_ninja_state(npp_handle h, int env0, int count, const double *xyv) {
    if (!h || !xyv || env0 < 0 || count <= 0 || env0 + count > h->n) return fail(h, NPP_ERR_INVALID, "npp_set_ninja_state: bad arguments");
    if (h->ls.levels.empty()) return fail(h, NPP_ERR_STATE, "npp_set_ninja_state: no levels loaded");
    for (size_t i = 0; i < (size_t)count * 4; i++)
        if (!std::isfinite(xyv[i])) return fail(h, NPP_ERR_INVALID, "npp_set_ninja_state: non-finite value");
    ON_DEVICE_JOINED(h);
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    const size_t N = (size_t)h->n;
    const int plane[4] = {F_X, F_Y, F_VX, F_VY};
    std::vector<double> col((size_t)count);
    for (int k = 0; k < 4; k++) {
        for (int i = 0; i < count; i++) col[i] = xyv[(size_t)i * 4 + k];
        HIP_TRY(h, hipMemcpy(h->env.f64.get() + plane[k] * N + env0, col.data(), sizeof(double) * count, hipMemcpyHostToDevice));
    }
    return reward_restart_range(h, env0, count);   // (reward mode "pbrs") an injected state starts the env's reward state afresh
}

// field of a mover record as the reference holds it: drone dir, thwump state -1 / 0 / 1, shove thwump state; 0 for the rest
static int mover_field(uint32_t kind, uint32_t w0) {
    const int bits = (int)((w0 >> 11) & 3u);
    if (kind == MK_DRONE || kind == MK_MINI || kind == MK_SHOVE) return bits;
    return kind == MK_THWUMP ? bits - 1 : 0;
}

int npp_set_mover_state(npp_handle h, int env0, int count, int slot, const double *xyab, const int32_t *field) {
    if (!h || !xyab || env0 < 0 || count <= 0 || env0 + count > h->n || slot < 0) return fail(h, NPP_ERR_INVALID, "npp_set_mover_state: bad arguments");
    if (h->ls.levels.empty()) return fail(h, NPP_ERR_STATE, "npp_set_mover_state: no levels loaded");
    for (size_t i = 0; i < (size_t)count * 4; i++)
        if (!std::isfinite(xyab[i])) return fail(h, NPP_ERR_INVALID, "npp_set_mover_state: non-finite value");
    ON_DEVICE_JOINED(h);
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (int rc = pull_levels(h)) return rc;
    if (!h->ls.zoo) return fail(h, NPP_ERR_INVALID, "npp_set_mover_state: the level set has no movers");
    for (int i = 0; i < count; i++) {
        const CompiledLevel &L = h->ls.levels[h->env_level[env0 + i]];
        if (slot >= (int)L.mov_meta.size()) return fail(h, NPP_ERR_INVALID, "npp_set_mover_state: slot past the level's movers");
        const uint32_t kind = L.mov_meta[slot] & 7u;
        if ((kind == MK_THWUMP || kind == MK_SHOVE) && (xyab[(size_t)i * 4 + 2] != 0 || xyab[(size_t)i * 4 + 3] != 0))
            return fail(h, NPP_ERR_INVALID, "npp_set_mover_state: thwumps have no third and fourth value");
        if (!field) continue;
        const bool ok = kind == MK_THWUMP ? (field[i] >= -1 && field[i] <= 1)
                                          : ((kind == MK_DRONE || kind == MK_MINI) && field[i] >= 0 && field[i] <= 3);
        if (!ok) return fail(h, NPP_ERR_INVALID, "npp_set_mover_state: the mover's kind has no such state");
    }
    const int door_words = (h->ls.zoo_doors + 1) / 2;
    const size_t off = (size_t)ZOO_HEAD + door_words + (size_t)ZOO_MOV_WORDS * slot;
    if (off + ZOO_MOV_WORDS > (size_t)h->ls.zoo_words) return fail(h, NPP_ERR_INVALID, "npp_set_mover_state: slot past the zoo block");
    for (int i = 0; i < count; i++) {
        double *rec = h->ls.zoo.get() + (size_t)(env0 + i) * h->ls.zoo_words + off;
        HIP_TRY(h, hipMemcpy(rec, xyab + (size_t)i * 4, sizeof(double) * 4, hipMemcpyHostToDevice));
        if (!field) continue;
        uint32_t w0;   // low half of word 4: cell | bits << 11 | static attributes; the high half (list-order number) is not touched
        HIP_TRY(h, hipMemcpy(&w0, rec + 4, sizeof(w0), hipMemcpyDeviceToHost));
        const uint32_t kind = h->ls.levels[h->env_level[env0 + i]].mov_meta[slot] & 7u;
        const uint32_t bits = (uint32_t)(kind == MK_THWUMP ? field[i] + 1 : field[i]);
        w0 = (w0 & ~(3u << 11)) | (bits << 11);
        HIP_TRY(h, hipMemcpy(rec + 4, &w0, sizeof(w0), hipMemcpyHostToDevice));
    }
    return reward_restart_range(h, env0, count);   // (reward mode "pbrs") likewise
}

int npp_dump_movers(npp_handle h, int env, double *out, int max_rows, int *n_out) {
    if (!h || env < 0 || env >= h->n || !out || !n_out || max_rows < 0) return fail(h, NPP_ERR_INVALID, "npp_dump_movers: bad arguments");
    if (h->ls.levels.empty()) return fail(h, NPP_ERR_STATE, "npp_dump_movers: no levels loaded");
    ON_DEVICE_JOINED(h);
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (int rc = pull_levels(h)) return rc;
    const CompiledLevel &L = h->ls.levels[h->env_level[env]];
    const int n = (int)L.mov_meta.size();
    if (n > max_rows) return fail(h, NPP_ERR_INVALID, "npp_dump_movers: buffer too small");
    *n_out = n;
    if (!n) return NPP_OK;
    const int door_words = (h->ls.zoo_doors + 1) / 2;
    std::vector<double> rec((size_t)ZOO_MOV_WORDS * n);
    HIP_TRY(h, hipMemcpy(rec.data(), h->ls.zoo.get() + (size_t)env * h->ls.zoo_words + ZOO_HEAD + door_words, sizeof(double) * rec.size(),
                         hipMemcpyDeviceToHost));
    for (int m = 0; m < n; m++) {
        const double *p = rec.data() + (size_t)ZOO_MOV_WORDS * m;
        uint64_t wd;
        std::memcpy(&wd, p + 4, 8);
        double *o = out + (size_t)m * 5;
        o[0] = p[0]; o[1] = p[1]; o[2] = p[2]; o[3] = p[3];
        o[4] = (double)mover_field(L.mov_meta[m] & 7u, (uint32_t)wd);
    }
    return NPP_OK;
}

int npp_dump_entities(npp_handle h, int env, int32_t *out, int max, int *n_out) {
    if (!h || env < 0 || env >= h->n || !out || !n_out) return fail(h, NPP_ERR_INVALID, "npp_dump_entities: bad arguments");
    if (h->ls.levels.empty()) return fail(h, NPP_ERR_STATE, "npp_dump_entities: no levels loaded");
    ON_DEVICE_JOINED(h);
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (int rc = pull_levels(h)) return rc;
    const CompiledLevel &L = h->ls.levels[h->env_level[env]];
    std::vector<uint32_t> w(h->ls.n_words_max);
    for (int k = 0; k < h->ls.n_words_max; k++)
        HIP_TRY(h, hipMemcpy(&w[k], h->ls.ent.get() + (size_t)k * h->n + env, sizeof(uint32_t), hipMemcpyDeviceToHost));
    int n = (int)L.ent_map_order.size();
    if (n > max) n = max;
    for (int i = 0; i < n; i++) {
        int slot = L.ent_map_order[i];
        out[i] = ent_state(w.data(), 1, 0, slot);
    }
    *n_out = n;
    return NPP_OK;
}

int npp_entity_checksum(npp_handle h, int env0, int count, double *out) {
    if (!h || env0 < 0 || count <= 0 || env0 + count > h->n || !out) return fail(h, NPP_ERR_INVALID, "npp_entity_checksum: bad arguments");
    if (h->ls.levels.empty()) return fail(h, NPP_ERR_STATE, "npp_entity_checksum: no levels loaded");
    ON_DEVICE_JOINED(h);
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (int rc = pull_levels(h)) return rc;
    size_t N = (size_t)h->n;
    std::vector<uint32_t> w((size_t)h->ls.n_words_max * count);
    for (int k = 0; k < h->ls.n_words_max; k++)
        HIP_TRY(h, hipMemcpy(w.data() + (size_t)k * count, h->ls.ent.get() + k * N + env0, sizeof(uint32_t) * count, hipMemcpyDeviceToHost));
    std::vector<double> zb;
    if (h->ls.zoo) {
        zb.resize((size_t)h->ls.zoo_words * count);
        HIP_TRY(h, hipMemcpy(zb.data(), h->ls.zoo.get() + (size_t)env0 * h->ls.zoo_words, sizeof(double) * zb.size(), hipMemcpyDeviceToHost));
    }
    const int door_words = (h->ls.zoo_doors + 1) / 2;
    for (int i = 0; i < count; i++) {
        const CompiledLevel &L = h->ls.levels[h->env_level[env0 + i]];
        const double *blk = h->ls.zoo ? zb.data() + (size_t)i * h->ls.zoo_words : nullptr;
        uint64_t head3 = 0;
        if (blk) std::memcpy(&head3, blk + 3, 8);
        const uint32_t ovr = (uint32_t)head3;
        double sx = 0, sy = 0, svx = 0, svy = 0;
        long code = 0, act = 0;
        for (uint32_t ref : L.dic_order) {
            if (ref & 0x80000000u) {
                int m = (int)(ref & 0x7fffffffu);
                uint32_t kind = L.mov_meta[m] & 7u;
                if (!blk) { sx += L.mov_x0[m]; sy += L.mov_y0[m]; act += 1; continue; }
                const double *p = blk + ZOO_HEAD + door_words + ZOO_MOV_WORDS * m;
                uint64_t wd;
                std::memcpy(&wd, p + 4, 8);
                uint32_t w0 = (uint32_t)wd;
                sx += p[0]; sy += p[1];
                if (kind == MK_BOUNCE || kind == MK_BALL) { svx += p[2]; svy += p[3]; }
                if (kind == MK_DRONE || kind == MK_MINI) code += 11 * ((w0 >> 11) & 3u);
                if (kind == MK_THWUMP) code += 5 * (((int)((w0 >> 11) & 3u) - 1 + 7) % 7);
                if (kind == MK_SHOVE) code += 5 * ((w0 >> 11) & 3u) + 17 * ((w0 >> 13) & 1u);
                act += 1;
            } else {
                int s = (int)ref;
                uint32_t kind = L.ent_meta[s] & 15u;
                uint32_t st = ent_state(w.data(), count, i, s);
                if (blk && s == L.obs_switch && (ovr & ZOO_OVR_SWITCH)) { sx += blk[4]; sy += blk[5]; }
                else if (blk && s == L.obs_door && (ovr & ZOO_OVR_DOOR)) { sx += blk[6]; sy += blk[7]; }
                else { sx += L.ent_x[s]; sy += L.ent_y[s]; }
                if (kind == EK_MINE) { code += 5 * st; act += 1; }
                else if (kind == EK_EXIT) act += 1;                       // the door object itself never deactivates
                else if (kind == EK_LOCKED) { code += 3 * (st & 1u); act += st & 1u; }
                else if (kind == EK_DOOR_REG) { code += 3 * ((st >> 1) & 1u); act += 1; }
                else if (kind == EK_DOOR_TRAP) { code += 3 * (1u - (st & 1u)); act += st & 1u; }
                else if (kind == EK_BOOST) { code += 13 * ((st >> 1) & 1u); act += 1; }
                else act += st & 1u;
            }
        }
        double *o = out + (size_t)i * 6;
        o[0] = sx; o[1] = sy; o[2] = svx; o[3] = svy; o[4] = (double)code; o[5] = (double)act;
    }
    return NPP_OK;
}

int npp_dump_level_segments(npp_handle h, int level, int16_t *out, int max_rows, int *n_out) {
    if (!h || level < 0 || level >= (int)h->ls.levels.size() || !out || !n_out)
        return fail(h, NPP_ERR_INVALID, "npp_dump_level_segments: bad arguments");
    int r = dump_segments(h->ls.levels[level], out, max_rows);
    if (r < 0) return fail(h, NPP_ERR_INVALID, "npp_dump_level_segments: buffer too small");
    *n_out = r;
    return NPP_OK;
}

}  // extern "C"
