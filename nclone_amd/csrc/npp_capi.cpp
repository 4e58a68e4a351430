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
#include "npp_host.hpp"
#include "npp_internal.hpp"
#include "npp_level.hpp"
#include "npp_reach_build.hpp"

using namespace npp;

struct npp_handle_s {
    int n = 0;
    int device = 0;
    unsigned flags = 0;
    hipStream_t stream = nullptr;
    double *d_f64 = nullptr;
    uint32_t *d_u32 = nullptr;
    uint32_t *d_ent = nullptr;
    float *d_sc_cache = nullptr;
    double *d_zoo = nullptr;   // per-env zoo blocks (always allocated with the levels; at least the 8-word head)
    std::vector<uint8_t> ovr;  // per env: ZOO_OVR_* flags set through npp_set_entity_pos
    int n_ovr = 0;
    std::vector<uint8_t> s_ovr;   // the same at npp_snapshot (the zoo block's head words 3..7 travel with the snapshot)
    double *s_zoo = nullptr;
    int zoo_words = 0, zoo_doors = 0, zoo_movers = 0;
    int zoo_active = 0;        // some env is assigned a level with zoo entities
    // snapshot slot (npp_snapshot / npp_restore)
    double *s_f64 = nullptr;
    uint32_t *s_u32 = nullptr;
    uint32_t *s_ent = nullptr;
    float *s_sc = nullptr;
    int s_words = 0;
    unsigned long long assign_gen = 0, s_gen = ~0ull;
    int32_t *d_env_level = nullptr;
    int32_t *d_trunc = nullptr;
    std::vector<int32_t> trunc;            // host mirror of d_trunc
    bool dyn_trunc = false;                // npp_set_dynamic_truncation: per-level limit from the reachable surface area
    std::vector<int32_t> level_trunc;      // [n_levels] that limit (empty = not computed for the loaded set)
    uint8_t *d_mask = nullptr;
    unsigned char *d_blob = nullptr;
    uint8_t *d_canvas = nullptr;   // tile-layer coverage canvas of every level (render paths; built on first use)
    float *d_gv_h = nullptr;       // global_view: per-level picture / horizontal sums / view of the level right after a reset
    uint8_t *d_gv_v = nullptr, *d_gv_p = nullptr;
    unsigned char *d_gv_x = nullptr;   // global_view: per-env scratch of the split cell pass
    uint32_t *d_gv_order = nullptr, *d_gv_cost = nullptr;   // global_view: heavy-first launch order and the per-env cost it is built from
    long gv_launches = 0;
    uint32_t *d_pf_order = nullptr, *d_pf_cost = nullptr;   // npp_render_player_frame: heavy-first env order and the per-env cost behind it
    long pf_launches = 0;
    uint32_t *d_wg_order = nullptr, *d_wg_cost = nullptr;   // npp_step: heavy-first workgroup order and the per-block cost behind it
    int wg_blocks = 0;
    long step_launches = 0;
    // autotuner of the step-kernel build variant (npp_kernels.hip: VariantK): windows of TUNE_WINDOW launches per variant, timed
    // with one pair of HIP events each (never synchronised: the decision is taken once the last event has completed)
    int variant_pin = -1;            // -1 = autotune
    int variant = 0;                 // what npp_step launches now
    int tune_state = 0;              // 0 = warm-up, 1 .. TUNE_ROUNDS * 3 = measuring windows, > that = waiting for events / decided
    int tune_count = 0;              // launches inside the current state
    bool tuned = false;
    std::vector<hipEvent_t> tune_ev;   // one (start, end) pair per measured launch: 2 * TUNE_WINDOW * windows
    // cost-split launch (experiment, NPP_STEP_SPLIT = "percent:variant_heavy:variant_light"): the heaviest workgroups of the
    // heavy-first order run as their own launch of another build variant on a second stream, joined by events
    hipStream_t split_stream = nullptr;
    hipEvent_t split_ev[2] = {nullptr, nullptr};
    long tune_since = 0;             // launches since the last decision
    // observation overlap (npp_set_obs_overlap / npp_set_obs_overlap_parts): npp_step cuts its heavy-first workgroup order at
    // cut_pct[] percent and launches every piece ("part") as a kernel of its own -- part 0, the cheap tail of the order, on the
    // caller's stream, the others on part_stream[] -- and while live_parts > 1 every observation entry point launches one kernel per
    // part on the stream of the part it reads, so the observations of the cheap envs are produced while the expensive envs are still
    // stepping.  join_streams() makes the caller's stream wait for the others.
    int n_cuts = 0;                  // 0 = off
    int cut_pct[3] = {0, 0, 0};      // ascending, from the head (most expensive end) of the order
    int live_parts = 1;              // parts of the last npp_step still to be joined (1 = it was not split)
    bool phase_dirty = true;         // d_phase does not describe the current order / cuts
    uint8_t *d_phase = nullptr;      // [n] which part steps the env (npp_phase_kernel, rewritten when the order or the cuts change)
    hipStream_t part_stream[4] = {nullptr, nullptr, nullptr, nullptr};   // part 0 = the cheap tail of the order, on the caller's stream
    // the streams behind part_stream[1..] and side[][]: created by calibrate_streams(), which keeps only streams whose kernels were
    // SEEN to run beside the caller's and beside each other (HIP spreads a process's streams over four hardware queues; two streams
    // on one queue serialise, and which queue a new stream gets depends on every stream the process has created before)
    std::vector<hipStream_t> owned;
    hipStream_t owned_for = nullptr;   // the caller's stream they were chosen against
    bool owned_valid = false;
    hipEvent_t cal_ev[2] = {nullptr, nullptr};
    hipEvent_t part_ev[4] = {nullptr, nullptr, nullptr, nullptr};        // join
    hipEvent_t ov_ev[2] = {nullptr, nullptr};                           // fork / tables on the caller's stream ready
    // ... and with two parts (four hardware queues feed a process) the observation kernels need not wait for each other either: the
    // kinds (bit 0 global_view, 1 player_frame, 2 reachability, 3 switch_states) named in side_mask run on a side stream forked off
    // the stream that stepped the part -- side[0][p] for global_view, side[1][p] shared by the other three
    unsigned side_mask = 0;
    hipStream_t side[2][2] = {};
    hipEvent_t side_ev[2][2] = {};   // fork, then reused for the join
    bool side_busy[2][2] = {};
    // reachability observation (npp_reachability; built on first use): per-level tables + per-env cache
    ReachHdr *d_rhdr = nullptr;
    unsigned char *d_rblob = nullptr;
    uint32_t *d_rkey = nullptr, *s_rkey = nullptr;      // (ninja cell, exit_switch_activated) of the cached vector, 0 = none
    float *d_rcache = nullptr, *s_rcache = nullptr;     // [n][REACH_DIM + 1]
    int s_reach = 0;                                    // the snapshot slot holds a reachability cache
    ReachMissDev rmiss = {nullptr, nullptr, nullptr, nullptr};   // per-env dictionary of the miss branch (levels with ReachHdr::miss_exit only)
    // frame stacking (npp_set_frame_stack / npp_frame_stack_push, npp_stack.hip): one ring of 2 K slots per env and stacked key
    int fs_vk = 0, fs_sk = 0, fs_repeat = 0;   // stack sizes (0 = off) and padding
    int fs_vhead = 0, fs_shead = 0;            // ring position of the newest entry
    uint8_t *d_fs_frames = nullptr;            // [n][2 fs_vk][84 * 84]
    float *d_fs_state = nullptr;               // [n][2 fs_sk][41]
    // level pool (npp_set_level_pool, npp_pool.hip): with it on, the device changes env_level / d_trunc after a step, and the host
    // mirrors env_level / trunc are read back lazily (pull_levels) where a host path needs them
    bool pool_on = false;
    bool pool_ever = false;     // a pool was on since npp_load_levels: levels change without npp_assign_levels, snapshots carry them
    bool pool_dirty = false;    // the device may have drawn since env_level / trunc were read back
    uint64_t pool_seed = 0;
    int pool_last = 0;          // the last level of non-zero weight
    std::vector<double> pool_w;
    double *d_pool_cdf = nullptr;        // [n_levels]
    uint32_t *d_pool_count = nullptr;    // [n] draw counts
    uint8_t *d_pool_flags = nullptr;     // [n] step flags when the caller asked for none
    uint8_t *d_pool_changed = nullptr;   // [n] envs that drew another level (device reset / observe mask)
    int32_t *d_level_trunc = nullptr;    // [n_levels] dynamic truncation limit per level (pool + dynamic truncation)
    int32_t *s_level = nullptr, *s_trunc = nullptr;   // snapshot of env_level / d_trunc / d_pool_count
    uint32_t *s_count = nullptr;
    LevelHdr *d_hdr = nullptr;
    int n_words_max = 1;
    uint32_t hot_max = 0;      // largest staged-level size over the loaded set
    uint32_t lds_hot_cap = 0;  // LDS bytes reserved for a staged level under the current launch geometry
    int lanes_per_env = 0;     // 0 = choose from n_envs
    int waves_per_block = 0;
    int geo_g = 1, geo_wpb = 1;
    int lds_level = 0;         // all workgroups level-uniform and staged levels fit
    std::vector<CompiledLevel> levels;
    std::vector<LevelHdr> hdrs;
    std::vector<int32_t> env_level;
    std::string err;
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
    hipError_t e = hipSuccess;
    for (int k = 0; k < 2; k++)
        for (int p = 0; p < 2; p++)
            if (h->side_busy[k][p]) {
                h->side_busy[k][p] = false;
                if (e == hipSuccess) e = hipEventRecord(h->side_ev[k][p], h->side[k][p]);
                if (e == hipSuccess) e = hipStreamWaitEvent(h->stream, h->side_ev[k][p], 0);
            }
    for (int p = 0; p < h->live_parts && h->live_parts > 1; p++) {
        if (h->part_stream[p] == h->stream) continue;
        if (e == hipSuccess) e = hipEventRecord(h->part_ev[p], h->part_stream[p]);
        if (e == hipSuccess) e = hipStreamWaitEvent(h->stream, h->part_ev[p], 0);
    }
    h->live_parts = 1;
    return e;
}
// the stream observation kernel `kind` of part `part` is launched on: the part's own stream, or (two parts only) a side stream
// forked off it here.  `tables`: the caller's stream holds work the kernel needs (order tables) -- other streams wait for that.
hipError_t obs_stream(npp_handle h, int kind, int part, bool tables, hipStream_t *out) {
    hipStream_t src = h->part_stream[part];
    hipError_t e = hipSuccess;
    const bool aside = h->n_cuts == 1 && (h->side_mask >> kind & 1) != 0 && h->side[kind ? 1 : 0][part] != nullptr;
    kind = kind ? 1 : 0;
    hipStream_t dst = aside ? h->side[kind][part] : src;
    if (aside && !h->side_busy[kind][part]) {   // (a second call before the join just queues behind the first)
        e = hipEventRecord(h->side_ev[kind][part], src);
        if (e == hipSuccess) e = hipStreamWaitEvent(dst, h->side_ev[kind][part], 0);
        h->side_busy[kind][part] = true;
    }
    if (e == hipSuccess && tables && dst != h->stream) {
        e = hipEventRecord(h->ov_ev[1], h->stream);
        if (e == hipSuccess) e = hipStreamWaitEvent(dst, h->ov_ev[1], 0);
    }
    *out = dst;
    return e;
}

// Do kernels on streams a and b run side by side?  Two idle wavefronts of `ticks` each, one per stream: b's ends about when a's
// does, or a whole kernel later.  (Setup path: synchronises both streams.)
bool streams_overlap(npp_handle h, hipStream_t a, hipStream_t b, long long ticks, float single_ms) {
    if (hipStreamSynchronize(a) != hipSuccess || hipStreamSynchronize(b) != hipSuccess) return true;
    bool ok = hipEventRecord(h->cal_ev[0], a) == hipSuccess;
    ok = ok && launch_spin(ticks, a) == hipSuccess && launch_spin(ticks, b) == hipSuccess;
    ok = ok && hipEventRecord(h->cal_ev[1], b) == hipSuccess;
    ok = ok && hipStreamSynchronize(a) == hipSuccess && hipStreamSynchronize(b) == hipSuccess;
    float ms = 0.f;
    if (!ok || hipEventElapsedTime(&ms, h->cal_ev[0], h->cal_ev[1]) != hipSuccess) return true;   // cannot tell: take the stream
    return ms < 1.6f * single_ms;
}

// `need` streams of the handle's own that overlap with the caller's stream and with each other (see NppHandle::owned); when fewer
// can be found among 12 candidates the rest are streams that do not -- slower, never wrong.
int calibrate_streams(npp_handle h, int need) {
    if (h->owned_valid && h->owned_for == h->stream && (int)h->owned.size() >= need) return NPP_OK;
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    for (hipStream_t st : h->owned) hipStreamDestroy(st);
    h->owned.clear();
    if (!h->cal_ev[0]) {
        HIP_TRY(h, hipEventCreate(&h->cal_ev[0]));
        HIP_TRY(h, hipEventCreate(&h->cal_ev[1]));
    }
    const long long ticks = 3000;   // 30 us of the 100 MHz wall clock
    float single_ms = 0.03f;
    {   // what one such kernel takes between two events on one stream (launch overhead included)
        launch_spin(ticks, h->stream);   // warm: the code object
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        HIP_TRY(h, hipEventRecord(h->cal_ev[0], h->stream));
        HIP_TRY(h, launch_spin(ticks, h->stream));
        HIP_TRY(h, hipEventRecord(h->cal_ev[1], h->stream));
        HIP_TRY(h, hipStreamSynchronize(h->stream));
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, h->cal_ev[0], h->cal_ev[1]) == hipSuccess && ms > 0.f) single_ms = ms;
    }
    std::vector<hipStream_t> rejected;
    for (int c = 0; c < 12 && (int)h->owned.size() < need; c++) {
        hipStream_t st = nullptr;
        HIP_TRY(h, hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
        bool ok = streams_overlap(h, h->stream, st, ticks, single_ms);
        for (size_t i = 0; ok && i < h->owned.size(); i++) ok = streams_overlap(h, h->owned[i], st, ticks, single_ms);
        (ok ? h->owned : rejected).push_back(st);   // a rejected stream stays alive until the search ends: it keeps its queue busy
    }
    while ((int)h->owned.size() < need && !rejected.empty()) { h->owned.push_back(rejected.back()); rejected.pop_back(); }
    for (hipStream_t st : rejected) hipStreamDestroy(st);
    while ((int)h->owned.size() < need) {
        hipStream_t st = nullptr;
        HIP_TRY(h, hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
        h->owned.push_back(st);
    }
    h->owned_for = h->stream;
    h->owned_valid = true;
    // hand them out: the parts first, then (two parts only) the side streams in use
    int k = 0;
    // the cheap tail of the order rides on the caller's stream: that stream also carries the order-table kernels the other
    // streams wait for, and behind the most expensive part they would come a whole step late (measured: 520 us per step
    // instead of 440, doors, full Dict)
    for (int q = 0; q <= h->n_cuts; q++) h->part_stream[q] = q == 0 ? h->stream : h->owned[k++];
    for (int i = 0; i < 2; i++)
        for (int q = 0; q < 2; q++) {
            const bool used = h->n_cuts == 1 && (i ? (h->side_mask & 14u) : (h->side_mask & 1u));
            h->side[i][q] = used ? h->owned[k++] : nullptr;
        }
    return NPP_OK;
}
int streams_needed(npp_handle h) {
    return h->n_cuts + (h->n_cuts == 1 ? 2 * (((h->side_mask & 14u) ? 1 : 0) + ((h->side_mask & 1u) ? 1 : 0)) : 0);
}

// One observation kernel: as it is on the caller's stream (overlap off), or once per part of the last split step, the most
// expensive part first, each launch told which part's envs are its own.
template <class F> int obs_launch(npp_handle h, KernelArgs a, int kind, bool tables, F &&launch) {
    if (h->live_parts <= 1) {   // overlap off, or the last step was not split
        HIP_TRY(h, launch(a, h->stream));
        return NPP_OK;
    }
    hipStream_t st = h->stream;
    a.phase = h->d_phase;
    for (int q = h->live_parts - 1; q >= 0; q--) {
        HIP_TRY(h, obs_stream(h, kind, q, tables, &st));
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
int pull_levels(npp_handle h);

void plan_geometry(npp_handle h, bool keep_tuning = false) {
    (void)pull_levels(h);   // (a failure leaves the mirror as it was and is reported by the next call that syncs)
    const int zoo_before = h->zoo_active;
    int g = h->lanes_per_env;
    if (const char *ev = std::getenv("NPP_LANES_PER_ENV")) g = std::atoi(ev);
    if (g <= 0) {
        // measured on MI355X (tools/sweep_geometry.py, tools/big_batch_probe.py): 16 lanes per env up to 16 384 envs, 8 at
        // 32 768, 4 from 65 536 on (95.8 M env-steps/s there; 2 lanes per env is 2.5x slower at any size)
        g = 16;
        while (g > 4 && (long long)h->n * g / 64 > 4096) g >>= 1;
    }
    int gg = 1;
    while (gg * 2 <= g && gg < 64) gg *= 2;
    g = gg;
    int wpb = h->waves_per_block;
    if (const char *ev = std::getenv("NPP_WAVES_PER_BLOCK")) wpb = std::atoi(ev);
    if (wpb <= 0) wpb = 4;
    if (wpb > 4) wpb = 4;
    while (wpb > 1 && (64 / g) * wpb > h->n) wpb >>= 1;
    h->zoo_active = h->n_ovr > 0 ? 1 : 0;   // repositioned switches / doors are handled by the zoo kernel's merged walk
    if (h->d_zoo)
        for (int e = 0; e < h->n && !h->zoo_active; e++) h->zoo_active = h->levels[h->env_level[e]].has_zoo ? 1 : 0;
    if (h->pool_on)   // (level pool) any level an env may draw
        for (size_t l = 0; l < h->pool_w.size() && !h->zoo_active; l++) h->zoo_active = h->pool_w[l] > 0.0 && h->levels[l].has_zoo ? 1 : 0;
    const int zw = h->zoo_active ? h->zoo_words : 0;
    // LDS plan: staged level + entity words + observation staging (+ zoo blocks) must fit the per-workgroup budget
    for (;;) {
        int epb = (64 / g) * wpb;
        uint32_t fixed = (uint32_t)lds_bytes(0, h->n_words_max, epb, zw);
        if (fixed > LDS_BUDGET) {
            if (wpb > 1) { wpb >>= 1; continue; }
            if (g < 64) { g *= 2; continue; }   // zoo blocks are big: fewer envs per wavefront
        }
        uint32_t cap = h->hot_max;
        if (zw && fixed + cap > LDS_BUDGET && wpb > 1) { wpb >>= 1; continue; }   // zoo: staging the level beats a bigger workgroup
        if (fixed + cap > LDS_BUDGET) cap = fixed < LDS_BUDGET ? ((LDS_BUDGET - fixed) / 16) * 16 : 0;
        h->lds_hot_cap = cap;
        break;
    }
    // a new plan (level set, assignment, geometry, zoo kernels on / off) restarts npp_step's variant autotuner; a plan that comes
    // out the same (npp_restore of a snapshot with the same overrides) keeps the decision
    const bool same_plan = keep_tuning && g == h->geo_g && wpb == h->geo_wpb && zoo_before == h->zoo_active;
    h->geo_g = g;
    h->geo_wpb = wpb;
    if (!same_plan) {
        h->tune_state = 0; h->tune_count = 0; h->tuned = h->variant_pin >= 0;
        h->variant = h->variant_pin >= 0 ? h->variant_pin : 0;
    }
    // can every workgroup stage ONE level?  (the host owns the env -> level assignment)
    int epb = (64 / g) * wpb;
    int ok = !h->hdrs.empty() && !h->pool_on;   // (level pool: levels change on the device, workgroups no longer share one)
    for (int b0 = 0; b0 < h->n && ok; b0 += epb) {
        int lvl = h->env_level[b0];
        if (h->hdrs[lvl].hot_bytes > h->lds_hot_cap) ok = 0;
        for (int e = b0 + 1; e < b0 + epb && e < h->n && ok; e++)
            if (h->env_level[e] != lvl) ok = 0;
    }
    h->lds_level = ok;
}

KernelArgs base_args(npp_handle h) {
    KernelArgs a;
    std::memset(&a, 0, sizeof(a));
    a.f64 = h->d_f64;
    a.u32 = h->d_u32;
    a.ent_bits = h->d_ent;
    a.sc_cache = h->d_sc_cache;
    a.env_level = h->d_env_level;
    a.trunc_limit = h->d_trunc;
    a.hdr = h->d_hdr;
    a.blob = h->d_blob;
    a.tile_canvas = h->d_canvas;
    a.n = h->n;
    a.autoreset = (h->flags & NPP_FLAG_AUTORESET) ? 1 : 0;
    a.fast_reset = (h->flags & NPP_FLAG_FAST_RESET) ? 1 : 0;   // in-kernel auto-resets
    a.n_words_max = h->n_words_max;
    a.lds_hot_cap = h->lds_hot_cap;
    a.lanes_per_env = h->geo_g;
    a.waves_per_block = h->geo_wpb;
    a.lds_level = h->lds_level;
    a.zoo = h->d_zoo;
    a.zoo_words = h->zoo_words;
    a.zoo_doors = h->zoo_doors;
    a.zoo_movers = h->zoo_movers;
    a.zoo_active = h->zoo_active;
    a.variant = (h->geo_g == 16 && !h->zoo_active) ? h->variant : 0;   // npp_step's autotuner (or the pinned build)
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

// The render kernels read the tile layer from a per-level coverage canvas (npp_render.hip); it is built the first time a
// frame is asked for, so handles that never render pay neither the memory (633 600 B per level) nor the kernel.
int ensure_canvas(npp_handle h) {
    if (h->d_canvas) return NPP_OK;
    const size_t bytes = (size_t)h->levels.size() * 600 * 1056 + 16;   // + 16: rows are read as aligned dword pairs
    HIP_TRY(h, hipMalloc((void **)&h->d_canvas, bytes));
    HIP_TRY(h, launch_tile_tables(h->stream));   // idempotent: every handle of a device writes the same bytes
    HIP_TRY(h, launch_tile_canvas(h->d_hdr, h->d_blob, h->d_canvas, (int)h->levels.size(), h->stream));
    return NPP_OK;
}

int ensure_gv_tables(npp_handle h, float **gh) {
    const size_t nl = h->levels.size();
    HIP_TRY(h, hipMalloc((void **)&h->d_gv_v, nl * 176 * 100));
    HIP_TRY(h, hipMalloc((void **)&h->d_gv_p, nl * 600 * 1056 + 16));   // + 16: row slices are read as four aligned dwords
    HIP_TRY(h, hipMalloc((void **)gh, nl * 600 * 100 * sizeof(float)));
    KernelArgs a = base_args(h);
    HIP_TRY(h, launch_gv_static(a, (int)nl, h->d_gv_p, *gh, h->d_gv_v, h->stream));
    return NPP_OK;
}

int ensure_gv(npp_handle h) {
    if (int rc = ensure_canvas(h)) return rc;
    if (h->d_gv_h) return NPP_OK;
    float *gh = nullptr;
    if (int rc = ensure_gv_tables(h, &gh)) {   // nothing half-built stays behind: the next call starts over (d_gv_h is the marker)
        hipFree(h->d_gv_v); hipFree(h->d_gv_p); hipFree(gh);
        h->d_gv_v = nullptr; h->d_gv_p = nullptr;
        return rc;
    }
    h->d_gv_h = gh;
    if (!h->d_gv_order) {
        HIP_TRY(h, hipMalloc((void **)&h->d_gv_order, (size_t)h->n * sizeof(uint32_t)));
        HIP_TRY(h, hipMalloc((void **)&h->d_gv_cost, (size_t)h->n * sizeof(uint32_t)));
        HIP_TRY(h, hipMemsetAsync(h->d_gv_cost, 0, (size_t)h->n * sizeof(uint32_t), h->stream));
        h->gv_launches = 0;   // the first launch builds an order (any permutation) from the zero costs
    }
#ifdef NPP_GV_SPLIT
    if (!h->d_gv_x) {   // (A/B builds of the split cell pass) sized by the number of envs, not by the level set: kept across npp_load_levels
        HIP_TRY(h, hipMalloc((void **)&h->d_gv_x, (size_t)h->n * GV_XSTRIDE));
    }
#endif
    return NPP_OK;
}

void free_reach(npp_handle h) {
    hipFree(h->d_rhdr); hipFree(h->d_rblob); hipFree(h->d_rkey); hipFree(h->d_rcache); hipFree(h->s_rkey); hipFree(h->s_rcache);
    hipFree(h->rmiss.stamp); hipFree(h->rmiss.raw); hipFree(h->rmiss.epoch); hipFree(h->rmiss.last_episode);
    h->d_rhdr = nullptr; h->d_rblob = nullptr; h->d_rkey = nullptr; h->d_rcache = nullptr; h->s_rkey = nullptr; h->s_rcache = nullptr;
    h->rmiss = {nullptr, nullptr, nullptr, nullptr};
    h->s_reach = 0;
}

// The reachability tables (npp_reach.cpp) are built the first time the observation is asked for: ~1 ms of host work and
// ~260 KB of HBM per level, which handles that never ask for it do not pay.
int ensure_reach_alloc(npp_handle h, const std::vector<ReachHdr> &hdrs, const std::vector<unsigned char> &blob, bool any_miss) {
    const size_t N = (size_t)h->n, nl = hdrs.size();
    HIP_TRY(h, hipMalloc((void **)&h->d_rblob, blob.size() + 16));
    HIP_TRY(h, hipMemcpy(h->d_rblob, blob.data(), blob.size(), hipMemcpyHostToDevice));
    HIP_TRY(h, hipMalloc((void **)&h->d_rkey, sizeof(uint32_t) * N));
    HIP_TRY(h, hipMemset(h->d_rkey, 0, sizeof(uint32_t) * N));
    HIP_TRY(h, hipMalloc((void **)&h->d_rcache, sizeof(float) * (REACH_DIM + 1) * N));
    HIP_TRY(h, hipMemset(h->d_rcache, 0, sizeof(float) * (REACH_DIM + 1) * N));
    if (any_miss) {   // 13.2 KB per env: 108 MB at 8192 envs
        HIP_TRY(h, hipMalloc((void **)&h->rmiss.stamp, sizeof(uint32_t) * REACH_CELLS * N));
        HIP_TRY(h, hipMemset(h->rmiss.stamp, 0, sizeof(uint32_t) * REACH_CELLS * N));
        HIP_TRY(h, hipMalloc((void **)&h->rmiss.raw, sizeof(double) * REACH_CELLS * N));
        HIP_TRY(h, hipMalloc((void **)&h->rmiss.epoch, sizeof(uint32_t) * N));
        HIP_TRY(h, hipMemset(h->rmiss.epoch, 0, sizeof(uint32_t) * N));
        HIP_TRY(h, hipMalloc((void **)&h->rmiss.last_episode, sizeof(uint32_t) * N));
        HIP_TRY(h, hipMemset(h->rmiss.last_episode, 0xff, sizeof(uint32_t) * N));
    }
    ReachHdr *d = nullptr;
    HIP_TRY(h, hipMalloc((void **)&d, sizeof(ReachHdr) * nl));
    h->d_rhdr = d;
    HIP_TRY(h, hipMemcpy(d, hdrs.data(), sizeof(ReachHdr) * nl, hipMemcpyHostToDevice));
    return NPP_OK;
}

int ensure_reach(npp_handle h) {
    if (h->d_rhdr) return NPP_OK;
    const size_t nl = h->levels.size();
    std::vector<ReachHdr> hdrs(nl);
    std::vector<unsigned char> blob;
    bool any_miss = false;
    for (size_t i = 0; i < nl; i++) {
        ReachBuilt R;
        build_reach(h->levels[i], R);
        if (!R.hdr.supported)
            return fail(h, NPP_ERR_UNSUPPORTED, "npp_reachability: level " + std::to_string(i) + ": " + R.note +
                                                    " (outside the restated part of the reference's reachability code, see DESIGN.md)");
        any_miss = any_miss || R.hdr.miss_exit;
        pack_reach(R, hdrs[i], blob);
    }
    const int rc = ensure_reach_alloc(h, hdrs, blob, any_miss);
    if (rc != NPP_OK) {   // a failed allocation / copy must not leave half a table set behind (d_rhdr is the "complete" marker)
        const std::string msg = h->err;
        free_reach(h);
        h->err = msg;
    }
    return rc;
}

// level pool: read the device's env_level / d_trunc back into the host mirrors (synchronises; only after a draw)
int pull_levels(npp_handle h) {
    if (!h->pool_dirty) return NPP_OK;
    HIP_TRY(h, join_streams(h));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    HIP_TRY(h, hipMemcpy(h->env_level.data(), h->d_env_level, sizeof(int32_t) * (size_t)h->n, hipMemcpyDeviceToHost));
    HIP_TRY(h, hipMemcpy(h->trunc.data(), h->d_trunc, sizeof(int32_t) * (size_t)h->n, hipMemcpyDeviceToHost));
    h->pool_dirty = false;
    return NPP_OK;
}

void level_trunc_table(npp_handle h) {
    if (h->level_trunc.size() == h->levels.size()) return;
    h->level_trunc.resize(h->levels.size());
    for (size_t i = 0; i < h->levels.size(); i++) {
        ReachBuilt R;
        build_reach(h->levels[i], R);
        h->level_trunc[i] = truncation_limit_for_area(R.spawn_area);
    }
}

// level pool + dynamic truncation: the per-level limits on the device, for the draw kernel
int upload_level_trunc(npp_handle h) {
    level_trunc_table(h);
    if (!h->d_level_trunc) HIP_TRY(h, hipMalloc((void **)&h->d_level_trunc, sizeof(int32_t) * h->levels.size()));
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    HIP_TRY(h, hipMemcpy(h->d_level_trunc, h->level_trunc.data(), sizeof(int32_t) * h->levels.size(), hipMemcpyHostToDevice));
    return NPP_OK;
}

// envs selected by mask (NULL = all) take their level's dynamic limit
int apply_dynamic_truncation(npp_handle h, const uint8_t *mask) {
    if (int rc = pull_levels(h)) return rc;
    level_trunc_table(h);
    for (int e = 0; e < h->n; e++)
        if (!mask || mask[e]) h->trunc[e] = h->level_trunc[h->env_level[e]];
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    HIP_TRY(h, hipMemcpy(h->d_trunc, h->trunc.data(), sizeof(int32_t) * (size_t)h->n, hipMemcpyHostToDevice));
    return NPP_OK;
}

// `fresh` = the entities are created for the first time since the level was assigned (the state a replay starts from);
// any later reset is a Simulator.reset(), after which Entity.index no longer starts at 0 (see ZOO_HEAD in npp_internal.hpp)
int reset_impl(npp_handle h, const uint8_t *env_mask, int fresh, int fast = 0, int automatic = 0) {
    if (!h) return NPP_ERR_INVALID;
    if (h->levels.empty()) return fail(h, NPP_ERR_STATE, "npp_reset: no levels loaded");
    ON_DEVICE_JOINED(h);
    KernelArgs a = base_args(h);
    a.reset_fresh = fresh;
    a.fast_reset = fresh ? 0 : fast;
    a.reset_auto = automatic;
    if (env_mask) {
        HIP_TRY(h, hipMemcpyAsync(h->d_mask, env_mask, (size_t)h->n, hipMemcpyHostToDevice, h->stream));
        a.reset_mask = h->d_mask;
    }
    HIP_TRY(h, launch_reset(a, h->stream));
    if (env_mask) HIP_TRY(h, hipStreamSynchronize(h->stream));  // env_mask is caller memory: finish the copy
    return NPP_OK;
}

// Level pool: the envs with (flags[e] & bits) draw a level (npp_pool.hip); those that drew another one are reset as after
// npp_assign_levels -- fresh Simulator.reset, reachability cache row and per-episode dictionary dropped -- by the existing kernels
// under the draw's device mask, and, when `out` is given, their observation rows are rewritten by a masked observe launch.
// The caller has joined the streams.
int pool_redraw(npp_handle h, const uint8_t *d_flags, int bits, const npp_step_out *out) {
    PoolArgs p;
    p.n = h->n;
    p.flags = d_flags;
    p.bits = bits;
    p.cdf = h->d_pool_cdf;
    p.n_levels = (int)h->levels.size();
    p.last = h->pool_last;
    p.seed = h->pool_seed;
    p.count = h->d_pool_count;
    p.env_level = h->d_env_level;
    p.trunc = h->d_trunc;
    p.level_trunc = h->dyn_trunc ? h->d_level_trunc : nullptr;
    p.changed = h->d_pool_changed;
    HIP_TRY(h, launch_pool_draw(p, h->stream));
    h->pool_dirty = true;
    KernelArgs a = base_args(h);
    a.reset_mask = h->d_pool_changed;
    a.reset_fresh = 1;
    a.fast_reset = 0;   // (base_args carries the auto-reset's NPP_FLAG_FAST_RESET) a new level is a Simulator.reset
    HIP_TRY(h, launch_reset(a, h->stream));
    if (h->d_rkey) HIP_TRY(h, launch_reach_restore(a, nullptr, nullptr, h->d_rkey, h->d_rcache, h->rmiss, h->stream));
    if (out) {
        KernelArgs o = base_args(h);
        o.n_ticks = 0;
        o.mode = 0;
        o.autoreset = 0;
        fill_out(o, out);
        o.out.flags = nullptr; o.out.reward = nullptr; o.out.frames = nullptr; o.out.terminal_state = nullptr; o.out.work = nullptr;
        o.obs_mask = h->d_pool_changed;
        HIP_TRY(h, launch_step(o, h->stream));
    }
    return NPP_OK;
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
    hipError_t e1 = hipMalloc((void **)&h->d_f64, sizeof(double) * NF64 * N);
    hipError_t e2 = hipMalloc((void **)&h->d_u32, sizeof(uint32_t) * NU32 * N);
    hipError_t e3 = hipMalloc((void **)&h->d_env_level, sizeof(int32_t) * N);
    hipError_t e4 = hipMalloc((void **)&h->d_trunc, sizeof(int32_t) * N);
    hipError_t e5 = hipMalloc((void **)&h->d_mask, N);
    hipError_t e6 = hipMalloc((void **)&h->d_sc_cache, sizeof(float) * 48 * N);
    hipError_t e7 = hipMalloc((void **)&h->d_pool_count, sizeof(uint32_t) * N);
    if (e1 != hipSuccess || e2 != hipSuccess || e3 != hipSuccess || e4 != hipSuccess || e5 != hipSuccess || e6 != hipSuccess ||
        e7 != hipSuccess) {
        npp_destroy(h);
        return fail(nullptr, NPP_ERR_HIP, "npp_create: hipMalloc failed");
    }
    h->env_level.assign(N, 0);
    h->trunc.assign(N, 10000);  // MAX_TIME_IN_FRAMES fallback (gym_environment/constants.py:8)
    hipMemcpy(h->d_trunc, h->trunc.data(), sizeof(int32_t) * N, hipMemcpyHostToDevice);
    hipMemset(h->d_env_level, 0, sizeof(int32_t) * N);
    hipMemset(h->d_pool_count, 0, sizeof(uint32_t) * N);
    *out = h;
    return NPP_OK;
}

int npp_destroy(npp_handle h) {
    if (!h) return NPP_OK;
    DeviceGuard dg(h->device);
    hipDeviceSynchronize();
    hipFree(h->d_f64); hipFree(h->d_u32); hipFree(h->d_ent); hipFree(h->d_env_level); hipFree(h->d_trunc);
    hipFree(h->d_mask); hipFree(h->d_blob); hipFree(h->d_hdr); hipFree(h->d_sc_cache); hipFree(h->d_canvas);
    hipFree(h->d_gv_h); hipFree(h->d_gv_v); hipFree(h->d_gv_p);
    hipFree(h->d_gv_x); hipFree(h->d_gv_order); hipFree(h->d_gv_cost); hipFree(h->d_wg_order); hipFree(h->d_wg_cost); hipFree(h->d_pf_order); hipFree(h->d_pf_cost);
    for (auto &e : h->tune_ev)
        if (e) hipEventDestroy(e);
    if (h->split_stream) { hipStreamDestroy(h->split_stream); hipEventDestroy(h->split_ev[0]); hipEventDestroy(h->split_ev[1]); }
    for (auto &e : h->ov_ev)
        if (e) hipEventDestroy(e);
    for (hipStream_t st : h->owned) hipStreamDestroy(st);
    for (auto &e : h->cal_ev)
        if (e) hipEventDestroy(e);
    for (int q = 0; q < 4; q++)
        if (h->part_ev[q]) hipEventDestroy(h->part_ev[q]);
    for (int k = 0; k < 2; k++)
        for (int p = 0; p < 2; p++)
            if (h->side_ev[k][p]) hipEventDestroy(h->side_ev[k][p]);
    hipFree(h->d_phase);
    hipFree(h->d_fs_frames); hipFree(h->d_fs_state);
    hipFree(h->d_pool_cdf); hipFree(h->d_pool_count); hipFree(h->d_pool_flags); hipFree(h->d_pool_changed); hipFree(h->d_level_trunc);
    hipFree(h->s_level); hipFree(h->s_count); hipFree(h->s_trunc);
    free_reach(h);
    hipFree(h->s_f64); hipFree(h->s_u32); hipFree(h->s_ent); hipFree(h->s_sc); hipFree(h->d_zoo); hipFree(h->s_zoo);
    delete h;
    return NPP_OK;
}

int npp_set_stream(npp_handle h, void *hip_stream) {
    if (!h) return NPP_ERR_INVALID;
    if (h->stream != (hipStream_t)hip_stream) {   // the autotuner's window events live on the old stream: start its cycle over
        h->tune_state = 0; h->tune_count = 0; h->tuned = h->variant_pin >= 0;
        h->variant = h->variant_pin >= 0 ? h->variant_pin : 0;
    }
    if (h->live_parts > 1 || h->n_cuts) {   // a split step may still be in flight: its other streams join the OLD stream
        ON_DEVICE_JOINED(h);
    }
    if (h->stream != (hipStream_t)hip_stream) h->owned_valid = false;   // (observation overlap) streams are chosen again at the next split step
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
    if (h->levels.empty()) return fail(h, NPP_ERR_STATE, "npp_snapshot: no levels loaded");
    ON_DEVICE_JOINED(h);
    size_t N = (size_t)h->n;
    if (!h->s_f64) {
        HIP_TRY(h, hipMalloc((void **)&h->s_f64, sizeof(double) * NF64 * N));
        HIP_TRY(h, hipMalloc((void **)&h->s_u32, sizeof(uint32_t) * NU32 * N));
        HIP_TRY(h, hipMalloc((void **)&h->s_sc, sizeof(float) * 48 * N));
        HIP_TRY(h, hipMalloc((void **)&h->s_level, sizeof(int32_t) * N));
        HIP_TRY(h, hipMalloc((void **)&h->s_count, sizeof(uint32_t) * N));
        HIP_TRY(h, hipMalloc((void **)&h->s_trunc, sizeof(int32_t) * N));
    }
    if (h->s_words != h->n_words_max) {
        hipFree(h->s_ent);
        h->s_ent = nullptr;
        HIP_TRY(h, hipMalloc((void **)&h->s_ent, sizeof(uint32_t) * (size_t)h->n_words_max * N));
        h->s_words = h->n_words_max;
    }
    HIP_TRY(h, hipMemcpyAsync(h->s_f64, h->d_f64, sizeof(double) * NF64 * N, hipMemcpyDeviceToDevice, h->stream));
    HIP_TRY(h, hipMemcpyAsync(h->s_u32, h->d_u32, sizeof(uint32_t) * NU32 * N, hipMemcpyDeviceToDevice, h->stream));
    HIP_TRY(h, hipMemcpyAsync(h->s_ent, h->d_ent, sizeof(uint32_t) * (size_t)h->n_words_max * N, hipMemcpyDeviceToDevice, h->stream));
    HIP_TRY(h, hipMemcpyAsync(h->s_sc, h->d_sc_cache, sizeof(float) * 48 * N, hipMemcpyDeviceToDevice, h->stream));
    // (level pool) each env's level, draw count and truncation limit go with its state
    HIP_TRY(h, hipMemcpyAsync(h->s_level, h->d_env_level, sizeof(int32_t) * N, hipMemcpyDeviceToDevice, h->stream));
    HIP_TRY(h, hipMemcpyAsync(h->s_count, h->d_pool_count, sizeof(uint32_t) * N, hipMemcpyDeviceToDevice, h->stream));
    HIP_TRY(h, hipMemcpyAsync(h->s_trunc, h->d_trunc, sizeof(int32_t) * N, hipMemcpyDeviceToDevice, h->stream));
    if (h->d_zoo) {
        if (!h->s_zoo) HIP_TRY(h, hipMalloc((void **)&h->s_zoo, sizeof(double) * (size_t)h->zoo_words * N));
        HIP_TRY(h, hipMemcpyAsync(h->s_zoo, h->d_zoo, sizeof(double) * (size_t)h->zoo_words * N, hipMemcpyDeviceToDevice, h->stream));
    }
    h->s_reach = 0;
    if (h->d_rkey) {   // the cached reachability vector is part of what the next observation returns
        if (!h->s_rkey) {
            HIP_TRY(h, hipMalloc((void **)&h->s_rkey, sizeof(uint32_t) * N));
            HIP_TRY(h, hipMalloc((void **)&h->s_rcache, sizeof(float) * (REACH_DIM + 1) * N));
        }
        HIP_TRY(h, hipMemcpyAsync(h->s_rkey, h->d_rkey, sizeof(uint32_t) * N, hipMemcpyDeviceToDevice, h->stream));
        HIP_TRY(h, hipMemcpyAsync(h->s_rcache, h->d_rcache, sizeof(float) * (REACH_DIM + 1) * N, hipMemcpyDeviceToDevice, h->stream));
        h->s_reach = 1;
    }
    h->s_ovr = h->ovr;
    h->s_gen = h->assign_gen;
    return NPP_OK;
}

int npp_restore(npp_handle h, const uint8_t *env_mask) {
    if (!h) return NPP_ERR_INVALID;
    if (!h->s_f64 || h->s_gen != h->assign_gen)
        return fail(h, NPP_ERR_STATE, "npp_restore: no snapshot for the current level assignment");
    ON_DEVICE_JOINED(h);
    KernelArgs a = base_args(h);
    if (env_mask) {
        HIP_TRY(h, hipMemcpyAsync(h->d_mask, env_mask, (size_t)h->n, hipMemcpyHostToDevice, h->stream));
        a.reset_mask = h->d_mask;
    }
    HIP_TRY(h, launch_restore(a, h->s_f64, h->s_u32, h->s_ent, h->s_sc, h->d_zoo ? h->s_zoo : nullptr, h->stream));
    if (h->d_rkey)   // no cache in the snapshot (taken before the first npp_reachability): the restored envs start without one
        HIP_TRY(h, launch_reach_restore(a, h->s_reach ? h->s_rkey : nullptr, h->s_rcache, h->d_rkey, h->d_rcache, h->rmiss, h->stream));
    if (h->pool_ever) {   // the pool changed levels since npp_load_levels: the snapshot's levels come back with the state
        HIP_TRY(h, launch_pool_restore(h->n, a.reset_mask, h->s_level, h->s_count, h->s_trunc, h->d_env_level, h->d_pool_count, h->d_trunc,
                                       h->stream));
        h->pool_dirty = true;
    }
    if (env_mask) HIP_TRY(h, hipStreamSynchronize(h->stream));
    // the restored zoo blocks carry the repositioning flags / coordinates of the snapshot (head words 3..7): the host's
    // view of them (which decides whether the zoo kernels run) is restored with them
    if (h->s_ovr.size() == h->ovr.size()) {
        for (int e = 0; e < h->n; e++)
            if (!env_mask || env_mask[e]) h->ovr[e] = h->s_ovr[e];
        h->n_ovr = 0;
        for (int e = 0; e < h->n; e++) h->n_ovr += h->ovr[e] != 0;
        plan_geometry(h, true);   // restoring a checkpoint every few hundred steps must not keep the autotuner in its warm-up
    } else if (h->pool_ever) {
        plan_geometry(h, true);
    }
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
    if (lanes_per_env) *lanes_per_env = h->geo_g;
    if (waves_per_block) *waves_per_block = h->geo_wpb;
    return NPP_OK;
}

int npp_num_envs(npp_handle h) { return h ? h->n : 0; }
int npp_num_levels(npp_handle h) { return h ? (int)h->levels.size() : 0; }

int npp_load_levels(npp_handle h, const double *blob, const int64_t *offsets, int n_levels) {
    if (!h || !blob || !offsets || n_levels <= 0) return fail(h, NPP_ERR_INVALID, "npp_load_levels: bad arguments");
    ON_DEVICE_JOINED(h);
    std::vector<CompiledLevel> lv(n_levels);
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
    // ---- pack the blob
    std::vector<unsigned char> host;
    std::vector<LevelHdr> hdrs(n_levels);
    int words_max = 1;
    uint32_t hot_max = 0;
    bool any_zoo = false;
    int zoo_doors = 0, zoo_movers = 0;
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
        if (L.has_zoo) any_zoo = true;
        // every level's block is initialised by the reset kernel (locked doors have an edge counter too)
        zoo_doors = std::max(zoo_doors, (int)H.n_zdoor);
        zoo_movers = std::max(zoo_movers, (int)H.n_mov);
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
        words_max = std::max(words_max, (int)H.n_words);
        H.fits_lds = 1;
        hot_max = std::max(hot_max, hot_bytes);
    }
    // ---- upload (replaces the previous set)
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    hipFree(h->d_blob); h->d_blob = nullptr;
    hipFree(h->d_canvas); h->d_canvas = nullptr;
    hipFree(h->d_gv_h); h->d_gv_h = nullptr;
    hipFree(h->d_gv_v); h->d_gv_v = nullptr;
    hipFree(h->d_gv_p); h->d_gv_p = nullptr;
    free_reach(h);
    hipFree(h->d_hdr); h->d_hdr = nullptr;
    hipFree(h->d_ent); h->d_ent = nullptr;
    hipFree(h->d_zoo); h->d_zoo = nullptr;
    hipFree(h->s_zoo); h->s_zoo = nullptr;
    // a new level set turns the level pool off (its weights were per level of the old set); draw counts restart
    hipFree(h->d_pool_cdf); h->d_pool_cdf = nullptr;
    hipFree(h->d_level_trunc); h->d_level_trunc = nullptr;
    h->pool_on = h->pool_ever = h->pool_dirty = false;
    h->pool_w.clear();
    HIP_TRY(h, hipMemset(h->d_pool_count, 0, sizeof(uint32_t) * (size_t)h->n));
    (void)any_zoo;
    zoo_block_plan(lv, zoo_doors, zoo_movers);
    for (int i = 0; i < n_levels; i++)   // round-1 fault: a block sized over zoo levels only was overrun
        if ((int)hdrs[i].n_zdoor > zoo_doors || (int)hdrs[i].n_mov > zoo_movers)
            return fail(h, NPP_ERR_STATE, "npp_load_levels: zoo block plan does not cover level " + std::to_string(i));
    h->zoo_words = zoo_words_for(zoo_doors, zoo_movers);
    h->zoo_doors = zoo_doors;
    h->zoo_movers = zoo_movers;
    HIP_TRY(h, hipMalloc((void **)&h->d_zoo, sizeof(double) * (size_t)h->zoo_words * h->n));
    HIP_TRY(h, hipMemset(h->d_zoo, 0, sizeof(double) * (size_t)h->zoo_words * h->n));
    h->ovr.assign(h->n, 0);
    h->n_ovr = 0;
    HIP_TRY(h, hipMalloc((void **)&h->d_blob, host.size() + 16));
    HIP_TRY(h, hipMemcpy(h->d_blob, host.data(), host.size(), hipMemcpyHostToDevice));
    HIP_TRY(h, hipMalloc((void **)&h->d_hdr, sizeof(LevelHdr) * n_levels));
    HIP_TRY(h, hipMemcpy(h->d_hdr, hdrs.data(), sizeof(LevelHdr) * n_levels, hipMemcpyHostToDevice));
    HIP_TRY(h, hipMalloc((void **)&h->d_ent, sizeof(uint32_t) * (size_t)words_max * h->n));
    HIP_TRY(h, hipMemset(h->d_ent, 0, sizeof(uint32_t) * (size_t)words_max * h->n));
    h->levels.swap(lv);
    h->hdrs.swap(hdrs);
    h->assign_gen++;
    h->n_words_max = words_max;
    h->hot_max = hot_max;
    std::fill(h->env_level.begin(), h->env_level.end(), 0);
    plan_geometry(h);
    if (lds_bytes(h->lds_hot_cap, h->n_words_max, (64 / h->geo_g) * h->geo_wpb, h->zoo_active ? h->zoo_words : 0) > LDS_BUDGET)
        return fail(h, NPP_ERR_INVALID, "npp_load_levels: entity tables exceed LDS");
    std::fill(h->env_level.begin(), h->env_level.end(), 0);
    HIP_TRY(h, hipMemset(h->d_env_level, 0, sizeof(int32_t) * (size_t)h->n));
    h->level_trunc.clear();
    if (h->dyn_trunc)
        if (int rc = apply_dynamic_truncation(h, nullptr)) return rc;
    return reset_impl(h, nullptr, 1);
}

int npp_assign_levels(npp_handle h, const int32_t *env_ids, const int32_t *level_ids, int n) {
    if (!h || !level_ids || n <= 0) return fail(h, NPP_ERR_INVALID, "npp_assign_levels: bad arguments");
    if (h->levels.empty()) return fail(h, NPP_ERR_STATE, "npp_assign_levels: no levels loaded");
    if (!env_ids && n != h->n) return fail(h, NPP_ERR_INVALID, "npp_assign_levels: env_ids == NULL needs n == n_envs");
    ON_DEVICE_JOINED(h);
    if (int rc = pull_levels(h)) return rc;   // (level pool) the whole mirror is uploaded below
    std::vector<uint8_t> mask(h->n, 0);
    for (int i = 0; i < n; i++) {   // validate everything before touching the assignment: an error must leave host and device in step
        int e = env_ids ? env_ids[i] : i;
        if (e < 0 || e >= h->n || level_ids[i] < 0 || level_ids[i] >= (int)h->levels.size())
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
    HIP_TRY(h, hipMemcpy(h->d_env_level, h->env_level.data(), sizeof(int32_t) * (size_t)h->n, hipMemcpyHostToDevice));
    if (h->d_rkey) {   // a new level: the env's cached reachability vector belongs to the old one
        KernelArgs a = base_args(h);
        HIP_TRY(h, hipMemcpy(h->d_mask, mask.data(), (size_t)h->n, hipMemcpyHostToDevice));
        a.reset_mask = h->d_mask;
        HIP_TRY(h, launch_reach_restore(a, nullptr, nullptr, h->d_rkey, h->d_rcache, h->rmiss, h->stream));
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
    const int fast = mode == 2 || (mode == 0 && (h->flags & NPP_FLAG_FAST_RESET));
    // mode 0 follows NppEnvironment.reset: the first reset after a level assignment reloads the map (Simulator.reset), later ones
    // are fast resets; the per-env "no reset yet" bit lives in the state planes (npp_kernels.hip: Nj::fastord bit 1)
    return reset_impl(h, env_mask, 0, fast ? 1 : 0, mode == 0 ? 1 : 0);
}

int npp_set_truncation_limit(npp_handle h, const int32_t *limits, int32_t all) {
    if (!h) return NPP_ERR_INVALID;
    ON_DEVICE_JOINED(h);
    if (limits) h->trunc.assign(limits, limits + h->n);
    else h->trunc.assign(h->n, all);
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    HIP_TRY(h, hipMemcpy(h->d_trunc, h->trunc.data(), sizeof(int32_t) * (size_t)h->n, hipMemcpyHostToDevice));
    return NPP_OK;
}

int npp_set_dynamic_truncation(npp_handle h, int enable) {
    if (!h) return NPP_ERR_INVALID;
    h->dyn_trunc = enable != 0;
    if (!h->dyn_trunc || h->levels.empty()) return NPP_OK;
    ON_DEVICE_JOINED(h);
    if (h->pool_on)
        if (int rc = upload_level_trunc(h)) return rc;
    return apply_dynamic_truncation(h, nullptr);
}

int npp_set_level_pool(npp_handle h, const double *weights, int n_levels, uint64_t seed) {
    if (!h) return NPP_ERR_INVALID;
    if (!weights) {   // off: every env keeps the level it plays now
        if (!h->pool_on) return NPP_OK;
        ON_DEVICE_JOINED(h);
        if (int rc = pull_levels(h)) return rc;
        h->pool_on = false;
        plan_geometry(h);
        return NPP_OK;
    }
    if (h->levels.empty()) return fail(h, NPP_ERR_STATE, "npp_set_level_pool: no levels loaded");
    std::vector<double> cdf;
    int last = 0;
    std::string err;
    if (!pool_cdf(weights, n_levels, (int)h->levels.size(), cdf, last, err)) return fail(h, NPP_ERR_INVALID, "npp_set_level_pool: " + err);
    if (h->n_ovr) return fail(h, NPP_ERR_STATE, "npp_set_level_pool: an exit switch / door is repositioned (npp_set_entity_pos)");
    ON_DEVICE_JOINED(h);
    const size_t N = (size_t)h->n;
    HIP_TRY(h, hipStreamSynchronize(h->stream));   // the previous CDF may still be read by queued draws
    if (!h->d_pool_cdf) HIP_TRY(h, hipMalloc((void **)&h->d_pool_cdf, sizeof(double) * cdf.size()));
    if (!h->d_pool_changed) {
        HIP_TRY(h, hipMalloc((void **)&h->d_pool_changed, N));
        HIP_TRY(h, hipMalloc((void **)&h->d_pool_flags, N));
        HIP_TRY(h, hipMemset(h->d_pool_flags, 0, N));
    }
    HIP_TRY(h, hipMemcpy(h->d_pool_cdf, cdf.data(), sizeof(double) * cdf.size(), hipMemcpyHostToDevice));
    if (!h->pool_on || seed != h->pool_seed) HIP_TRY(h, hipMemset(h->d_pool_count, 0, sizeof(uint32_t) * N));   // a new stream of draws
    if (h->dyn_trunc)
        if (int rc = upload_level_trunc(h)) return rc;
    const bool was_on = h->pool_on;
    h->pool_w.assign(weights, weights + n_levels);
    h->pool_seed = seed;
    h->pool_last = last;
    h->pool_on = h->pool_ever = true;
    // the step-variant autotuner decides once for the pool: a weight update keeps its decision unless it switches the zoo kernels
    plan_geometry(h, was_on);
    return NPP_OK;
}

int npp_draw_levels(npp_handle h, const uint8_t *env_mask) {
    if (!h) return NPP_ERR_INVALID;
    if (!h->pool_on) return fail(h, NPP_ERR_STATE, "npp_draw_levels: the level pool is off (npp_set_level_pool)");
    ON_DEVICE_JOINED(h);
    if (env_mask) HIP_TRY(h, hipMemcpyAsync(h->d_mask, env_mask, (size_t)h->n, hipMemcpyHostToDevice, h->stream));
    else HIP_TRY(h, hipMemsetAsync(h->d_mask, 1, (size_t)h->n, h->stream));
    if (int rc = pool_redraw(h, h->d_mask, 0xff, nullptr)) return rc;
    if (env_mask) HIP_TRY(h, hipStreamSynchronize(h->stream));   // env_mask is caller memory: finish the copy
    return NPP_OK;
}

int npp_env_level_view(npp_handle h, const int32_t **d_levels) {
    if (!h || !d_levels) return fail(h, NPP_ERR_INVALID, "npp_env_level_view: bad arguments");
    *d_levels = h->d_env_level;
    return NPP_OK;
}

int npp_get_env_levels(npp_handle h, int32_t *host_out) {
    if (!h || !host_out) return fail(h, NPP_ERR_INVALID, "npp_get_env_levels: bad arguments");
    ON_DEVICE_JOINED(h);
    if (int rc = pull_levels(h)) return rc;
    std::memcpy(host_out, h->env_level.data(), sizeof(int32_t) * (size_t)h->n);
    return NPP_OK;
}


#ifndef NPP_STEP_FOLD
#define NPP_STEP_FOLD 0
#endif
namespace {
// 256 launches of warm-up (episodes desynchronise: right after a reset every env sits at its spawn and the launches are dominated by
// the levels with a crease under the spawn, which favours variant 2 -- a first cut that tuned on launches 48 .. 288 picked it for the
// mixed set and lost 10 %), then 9 interleaved windows of 48 launches; the decision is re-examined every 16 384 launches
constexpr int TUNE_WARM = 256, TUNE_WINDOW = 48, TUNE_ROUNDS = 3, TUNE_AGAIN = 16384;
// restart the tuner (new level set / assignment / geometry): the warm-up also lets the heavy-first order settle
void tune_reset(npp_handle h) {
    h->tune_state = 0; h->tune_count = 0; h->tuned = h->variant_pin >= 0;
    h->variant = h->variant_pin >= 0 ? h->variant_pin : 0;
}
// called by npp_step before every launch; returns the variant to launch.  *pair >= 0: a measured launch -- npp_step records
// tune_ev[2 * pair] right before and tune_ev[2 * pair + 1] right after the step kernel, so that only the kernel itself is timed
// (observation kernels and the caller's own work on the stream, whose cost varies with the state, stay outside: ADVICE r2)
int tune_next(npp_handle h, int *pair) {
    *pair = -1;
    if (h->variant_pin >= 0) return h->variant_pin;
    if (h->geo_g != 16 || h->zoo_active) return 0;   // only the plain G = 16 kernels have variants
    if (h->tuned) {
        static const long again = [] { const char *ev = std::getenv("NPP_TUNE_AGAIN"); return ev ? std::atol(ev) : (long)TUNE_AGAIN; }();   // tests shorten it
        if (++h->tune_since < again) return h->variant;
        h->tuned = false; h->tune_state = 0; h->tune_count = TUNE_WARM; h->tune_since = 0;   // measure again, no warm-up needed
    }
    const int n_win = 3 * TUNE_ROUNDS;
    if (h->tune_state == 0) {   // warm-up on variant 0
        if (++h->tune_count <= TUNE_WARM) return h->variant;
        if (h->tune_ev.empty()) {
            h->tune_ev.assign((size_t)2 * TUNE_WINDOW * n_win, nullptr);
            for (auto &e : h->tune_ev)
                if (hipEventCreate(&e) != hipSuccess) {   // no events: stay on variant 0
                    for (auto &d : h->tune_ev)
                        if (d) hipEventDestroy(d);
                    h->tune_ev.clear();
                    h->tuned = true; h->variant = 0;
                    return 0;
                }
        }
        h->tune_state = 1; h->tune_count = 0;
    }
    if (h->tune_state <= n_win) {   // window w measures variant (w - 1) % 3
        const int w = h->tune_state;
        *pair = (w - 1) * TUNE_WINDOW + h->tune_count;
        if (++h->tune_count == TUNE_WINDOW) { h->tune_state++; h->tune_count = 0; }
        return (w - 1) % 3;
    }
    // all windows recorded: decide as soon as the last launch has been reached by the GPU (no waiting)
    if (hipEventQuery(h->tune_ev.back()) == hipSuccess) {
        float t[3] = {0.f, 0.f, 0.f};
        bool ok = true;
        for (int w = 0; w < n_win && ok; w++)
            for (int k = 0; k < TUNE_WINDOW && ok; k++) {
                float ms = 0.f;
                const size_t p = (size_t)w * TUNE_WINDOW + k;
                ok = hipEventElapsedTime(&ms, h->tune_ev[2 * p], h->tune_ev[2 * p + 1]) == hipSuccess;
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
        h->variant = best; h->tuned = true; h->tune_since = 0;
        return best;
    }
    return h->variant;
}
}  // namespace

int npp_set_obs_overlap_parts(npp_handle h, const int *cuts, int n_cuts) {
    if (!h || n_cuts < 0 || n_cuts > 3 || (n_cuts && !cuts)) return fail(h, NPP_ERR_INVALID, "npp_set_obs_overlap_parts: at most three cuts");
    for (int i = 0; i < n_cuts; i++)
        if (cuts[i] <= (i ? cuts[i - 1] : 0) || cuts[i] >= 100)
            return fail(h, NPP_ERR_INVALID, "npp_set_obs_overlap_parts: cuts must be ascending percentages in (0, 100)");
    ON_DEVICE_JOINED(h);
    if (n_cuts > 0 && !h->d_phase) {
        HIP_TRY(h, hipMalloc((void **)&h->d_phase, (size_t)h->n));
        HIP_TRY(h, hipMemsetAsync(h->d_phase, 0, (size_t)h->n, h->stream));
        for (auto &e : h->ov_ev) HIP_TRY(h, hipEventCreateWithFlags(&e, hipEventDisableTiming));
        // player_frame beside the rest.  Measured (doors, full Dict, two parts cut at 40 %): no side stream 471 us per step,
        // global_view aside 485, player_frame aside 436, both 555 -- HIP feeds a process through four hardware queues, so more
        // streams than that share queues and serialise again
        h->side_mask = 2;
        if (const char *ev = std::getenv("NPP_OBS_SIDE")) h->side_mask = (unsigned)std::atoi(ev) & 15u;
    }
    for (int q = 0; q < 4; q++)
        if (!h->part_ev[q]) HIP_TRY(h, hipEventCreateWithFlags(&h->part_ev[q], hipEventDisableTiming));
    for (int k = 0; k < 2; k++)
        for (int q = 0; q < 2; q++)
            if (!h->side_ev[k][q]) HIP_TRY(h, hipEventCreateWithFlags(&h->side_ev[k][q], hipEventDisableTiming));
    if (n_cuts != h->n_cuts) h->owned_valid = false;
    h->phase_dirty = true;
    h->n_cuts = n_cuts;
    for (int i = 0; i < n_cuts; i++) h->cut_pct[i] = cuts[i];
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
    h->variant_pin = variant;
    tune_reset(h);
    return NPP_OK;
}

int npp_get_step_variant(npp_handle h, int *variant, int *tuned) {
    if (!h) return NPP_ERR_INVALID;
    if (variant) *variant = (h->geo_g == 16 && !h->zoo_active) ? h->variant : 0;
    if (tuned) *tuned = (h->tuned || h->variant_pin >= 0 || h->geo_g != 16 || h->zoo_active) ? 1 : 0;
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
    fill_out(a, out);
    {   // heavy-first workgroup order: rebuilt from the per-block costs every 16th launch (and whenever the launch geometry changes)
        const int epb = (64 / (h->geo_g > 0 ? h->geo_g : 1)) * (h->geo_wpb > 0 ? h->geo_wpb : 1);
        const int blocks = (h->n + epb - 1) / epb;
        if (!h->d_wg_order) {
            HIP_TRY(h, hipMalloc((void **)&h->d_wg_order, (size_t)h->n * sizeof(uint32_t)));
            HIP_TRY(h, hipMalloc((void **)&h->d_wg_cost, (size_t)h->n * sizeof(uint32_t)));
            h->wg_blocks = 0;
        }
        const bool fresh = blocks != h->wg_blocks;
        if (fresh) tune_reset(h);
        if (fresh || h->step_launches % 16 == 0) {
            h->phase_dirty = true;   // (observation overlap) the parts are pieces of this order
            if (fresh) HIP_TRY(h, hipMemsetAsync(h->d_wg_cost, 0, (size_t)h->n * sizeof(uint32_t), h->stream));
            HIP_TRY(h, launch_cost_order(h->d_wg_cost, h->d_wg_order, blocks, NPP_STEP_FOLD, h->stream));
            HIP_TRY(h, hipMemsetAsync(h->d_wg_cost, 0, (size_t)blocks * sizeof(uint32_t), h->stream));   // costs are maxima over the next 16 launches
            h->wg_blocks = blocks;
        }
        h->step_launches++;
        a.wg_order = h->d_wg_order;
        a.wg_cost = h->d_wg_cost;
    }
    {   // cost-split launch (VERDICT r2 #3b; off unless NPP_STEP_SPLIT is set -- measured, no gain: DESIGN.md 4.1)
        static const char *sp = std::getenv("NPP_STEP_SPLIT");
        int pct = 0, vh = 0, vl = 1;
        if (sp && std::sscanf(sp, "%d:%d:%d", &pct, &vh, &vl) == 3 && pct > 0 && pct < 100 && h->geo_g == 16 && !h->zoo_active && a.wg_order) {
            const int epb = (64 / h->geo_g) * h->geo_wpb, blocks = (h->n + epb - 1) / epb;
            const int heavy = std::max(1, blocks * pct / 100);
            if (!h->split_stream) {
                HIP_TRY(h, hipStreamCreateWithFlags(&h->split_stream, hipStreamNonBlocking));
                HIP_TRY(h, hipEventCreateWithFlags(&h->split_ev[0], hipEventDisableTiming));
                HIP_TRY(h, hipEventCreateWithFlags(&h->split_ev[1], hipEventDisableTiming));
            }
            HIP_TRY(h, hipEventRecord(h->split_ev[0], h->stream));
            HIP_TRY(h, hipStreamWaitEvent(h->split_stream, h->split_ev[0], 0));
            KernelArgs ah = a, al = a;
            ah.variant = vh; ah.wg_first = 0; ah.wg_count = heavy;
            al.variant = vl; al.wg_first = heavy; al.wg_count = blocks - heavy;
            HIP_TRY(h, launch_step(ah, h->split_stream));
            HIP_TRY(h, launch_step(al, h->stream));
            HIP_TRY(h, hipEventRecord(h->split_ev[1], h->split_stream));
            HIP_TRY(h, hipStreamWaitEvent(h->stream, h->split_ev[1], 0));
            return NPP_OK;
        }
    }
    int pair = -1;
    a.variant = tune_next(h, &pair);
    if (h->n_cuts > 0 && h->d_phase && pair < 0 && (h->tuned || h->variant_pin >= 0 || h->geo_g != 16 || h->zoo_active)) {
        // observation overlap: the pieces of the heavy-first order as launches of their own, the most expensive first; the
        // observation entry points called next launch one kernel per part.  Only with workgroups of whole reachability groups (16
        // envs) and never on a launch the autotuner is timing.
        const int epb = (64 / h->geo_g) * h->geo_wpb, blocks = (h->n + epb - 1) / epb;
        int edge[5] = {0, 0, 0, 0, 0};   // part q = n_cuts - i covers order entries [edge[i], edge[i + 1])
        bool ok = epb % 16 == 0;
        for (int i = 0; i < h->n_cuts; i++) {
            edge[i + 1] = (int)((long long)blocks * h->cut_pct[i] / 100);
            ok = ok && edge[i + 1] > edge[i];
        }
        edge[h->n_cuts + 1] = blocks;
        ok = ok && edge[h->n_cuts + 1] > edge[h->n_cuts];
        if (ok) {
            // the one-wavefront-per-SIMD build holds 310 registers: beside it neither another part nor an observation kernel finds
            // room on the SIMD, which is the point of the split (doors, full Dict: 502 us per step with it, 435-442 with build 0)
            if (a.variant == 2) a.variant = 0;
            if (!h->owned_valid || h->owned_for != h->stream)   // (first split step after npp_set_stream: one-off, synchronises)
                if (int rc = calibrate_streams(h, streams_needed(h))) return rc;
            if (h->phase_dirty) {   // the env -> part map, on the caller's stream ahead of the fork
                HIP_TRY(h, launch_phase_assign(h->d_wg_order, blocks, epb, h->n, edge, h->n_cuts + 1, h->d_phase, h->stream));
                h->phase_dirty = false;
            }
            HIP_TRY(h, hipEventRecord(h->ov_ev[0], h->stream));
            h->live_parts = h->n_cuts + 1;
            for (int i = 0; i <= h->n_cuts; i++) {
                const int q = h->n_cuts - i;
                KernelArgs ap = a;
                ap.wg_first = edge[i]; ap.wg_count = edge[i + 1] - edge[i];
                if (h->part_stream[q] != h->stream) HIP_TRY(h, hipStreamWaitEvent(h->part_stream[q], h->ov_ev[0], 0));
                HIP_TRY(h, launch_step(ap, h->part_stream[q]));
            }
            return NPP_OK;
        }
    }
    if (pair >= 0) hipEventRecord(h->tune_ev[2 * (size_t)pair], h->stream);
    const hipError_t le = launch_step(a, h->stream);
    if (pair >= 0) hipEventRecord(h->tune_ev[2 * (size_t)pair + 1], h->stream);
    HIP_TRY(h, le);
    return NPP_OK;
}
}  // namespace

extern "C" {

int npp_step(npp_handle h, const uint8_t *d_actions, int frame_skip, const npp_step_out *out) {
    if (!h || !d_actions || frame_skip <= 0) return fail(h, NPP_ERR_INVALID, "npp_step: bad arguments");
    if (h->levels.empty()) return fail(h, NPP_ERR_STATE, "npp_step: no levels loaded");
    if (!h->pool_on || !(h->flags & NPP_FLAG_AUTORESET)) return step_impl(h, d_actions, frame_skip, out);
    // level pool: the step as without it, then (joined) the draw for the envs whose episode ended -- read from the step's flags
    npp_step_out o;
    std::memset(&o, 0, sizeof(o));
    if (out) o = *out;
    if (!o.d_flags) o.d_flags = h->d_pool_flags;
    if (int rc = step_impl(h, d_actions, frame_skip, &o)) return rc;
    ON_DEVICE_JOINED(h);
    return pool_redraw(h, o.d_flags, NPP_F_WON | NPP_F_DEAD | NPP_F_TRUNCATED, &o);
}

int npp_step_many(npp_handle h, const uint8_t *d_actions, int n_steps, int frame_skip, const npp_step_out *out) {
    if (!h || !d_actions || frame_skip <= 0 || n_steps <= 0) return fail(h, NPP_ERR_INVALID, "npp_step_many: bad arguments");
    if (h->levels.empty()) return fail(h, NPP_ERR_STATE, "npp_step_many: no levels loaded");
    ON_DEVICE_JOINED(h);
    KernelArgs a = base_args(h);
    a.inputs = d_actions;
    a.n_ticks = frame_skip;
    a.n_steps = n_steps;
    a.mode = 0;
    fill_out(a, out);
    a.out.terminal_state = nullptr;   // pre-reset observations exist for single steps only
    HIP_TRY(h, launch_step(a, h->stream));
    return NPP_OK;
}

int npp_tick(npp_handle h, const uint8_t *d_inputs, int n_ticks) {
    if (!h || !d_inputs || n_ticks <= 0) return fail(h, NPP_ERR_INVALID, "npp_tick: bad arguments");
    if (h->levels.empty()) return fail(h, NPP_ERR_STATE, "npp_tick: no levels loaded");
    ON_DEVICE_JOINED(h);
    KernelArgs a = base_args(h);
    a.inputs = d_inputs;
    a.n_ticks = n_ticks;
    a.mode = 1;
    a.autoreset = 0;
    HIP_TRY(h, launch_step(a, h->stream));
    return NPP_OK;
}

int npp_observe(npp_handle h, const npp_step_out *out) {
    if (!h || !out) return fail(h, NPP_ERR_INVALID, "npp_observe: bad arguments");
    if (h->levels.empty()) return fail(h, NPP_ERR_STATE, "npp_observe: no levels loaded");
    ON_DEVICE_JOINED(h);
    KernelArgs a = base_args(h);
    a.n_ticks = 0;
    a.mode = 0;
    a.autoreset = 0;
    fill_out(a, out);
    HIP_TRY(h, launch_step(a, h->stream));
    return NPP_OK;
}

}  // extern "C"

namespace {
// player_frame of every env into d_out + env * stride (and, with mirror != 0, also mirror bytes further on)
int render_player_frame(npp_handle h, uint8_t *d_out, uint32_t stride, uint32_t mirror) {
    if (h->levels.empty()) return fail(h, NPP_ERR_STATE, "npp_render_player_frame: no levels loaded");
    ON_DEVICE(h);
    bool tables = !h->d_canvas;   // (observation overlap) something the second stream has to wait for was put on the caller's stream
    if (int rc = ensure_canvas(h)) return rc;
    KernelArgs a = base_args(h);
    {   // heavy-first env order, rebuilt from the last launch's per-env clocks on every 8th launch
        if (!h->d_pf_order) {
            HIP_TRY(h, hipMalloc((void **)&h->d_pf_order, (size_t)h->n * sizeof(uint32_t)));
            HIP_TRY(h, hipMalloc((void **)&h->d_pf_cost, (size_t)h->n * sizeof(uint32_t)));
            HIP_TRY(h, hipMemsetAsync(h->d_pf_cost, 0, (size_t)h->n * sizeof(uint32_t), h->stream));
            h->pf_launches = 0;
        }
        if (h->pf_launches % 8 < 2) {
            HIP_TRY(h, launch_cost_order(h->d_pf_cost, h->d_pf_order, h->n, 0, h->stream));
            tables = true;
        }
        h->pf_launches++;
        a.wg_order = h->d_pf_order;
        a.wg_cost = h->d_pf_cost;
    }
    const int centered = (h->flags & NPP_FLAG_FRAME_CENTERED) ? 1 : 0;
    return obs_launch(h, a, 1, tables,
                      [&](const KernelArgs &ka, hipStream_t st) { return launch_render(ka, d_out, centered, st, stride, mirror); });
}
}  // namespace

extern "C" {

int npp_render_player_frame(npp_handle h, uint8_t *d_out) {
    if (!h || !d_out) return fail(h, NPP_ERR_INVALID, "npp_render_player_frame: bad arguments");
    return render_player_frame(h, d_out, 84 * 84, 0);
}

int npp_set_frame_stack(npp_handle h, int visual_k, int state_k, int padding) {
    if (!h || visual_k < 0 || visual_k > 12 || state_k < 0 || state_k > 12 || padding < 0 || padding > 1)
        return fail(h, NPP_ERR_INVALID, "npp_set_frame_stack: stack sizes must be 0 (off) or 1..12 and padding 0 (zero) or 1 (repeat)");
    ON_DEVICE_JOINED(h);
    HIP_TRY(h, hipStreamSynchronize(h->stream));   // the old rings may still be read by queued work
    hipFree(h->d_fs_frames); hipFree(h->d_fs_state);
    h->d_fs_frames = nullptr; h->d_fs_state = nullptr;
    h->fs_vk = h->fs_sk = 0;
    const size_t N = (size_t)h->n;
    if (visual_k) {
        const size_t b = N * 2 * visual_k * 84 * 84;
        HIP_TRY(h, hipMalloc((void **)&h->d_fs_frames, b));
        HIP_TRY(h, hipMemsetAsync(h->d_fs_frames, 0, b, h->stream));
    }
    if (state_k) {
        const size_t b = N * 2 * state_k * NPP_GAME_STATE_DIM * sizeof(float);
        HIP_TRY(h, hipMalloc((void **)&h->d_fs_state, b));
        HIP_TRY(h, hipMemsetAsync(h->d_fs_state, 0, b, h->stream));
    }
    h->fs_vk = visual_k; h->fs_sk = state_k; h->fs_repeat = padding;
    h->fs_vhead = visual_k ? visual_k - 1 : 0;   // the first push completes position 0
    h->fs_shead = state_k ? state_k - 1 : 0;
    return NPP_OK;
}

int npp_frame_stack_render(npp_handle h) {
    if (!h) return NPP_ERR_INVALID;
    if (!h->fs_vk) return fail(h, NPP_ERR_STATE, "npp_frame_stack_render: visual stacking is off (npp_set_frame_stack)");
    const int K = h->fs_vk, q = (h->fs_vhead + 1) % K;
    const uint32_t slot = 84 * 84, stride = (uint32_t)(2 * K) * slot;
    // position q lives in slots q and q + K; slot 0 is never inside a window, so position 0 is written once
    uint8_t *dst = h->d_fs_frames + (size_t)(q ? q : K) * slot;
    return render_player_frame(h, dst, stride, q ? (uint32_t)K * slot : 0u);
}

int npp_frame_stack_push(npp_handle h, const float *d_game_state, const float *d_terminal_state, const uint8_t *d_flags,
                         int reset_bits, int reset_all, float *d_terminal_stack) {
    if (!h || !d_game_state || (!reset_all && reset_bits && !d_flags) || (d_terminal_stack && !d_terminal_state))
        return fail(h, NPP_ERR_INVALID, "npp_frame_stack_push: bad arguments");
    if (!h->fs_vk && !h->fs_sk) return fail(h, NPP_ERR_STATE, "npp_frame_stack_push: frame stacking is off (npp_set_frame_stack)");
    if (d_terminal_stack && !h->fs_sk) return fail(h, NPP_ERR_STATE, "npp_frame_stack_push: a terminal stack needs state stacking");
    ON_DEVICE_JOINED(h);
    if (h->fs_vk) h->fs_vhead = (h->fs_vhead + 1) % h->fs_vk;
    if (h->fs_sk) h->fs_shead = (h->fs_shead + 1) % h->fs_sk;
    StackArgs a;
    a.n = h->n;
    a.visual_k = h->fs_vk; a.state_k = h->fs_sk;
    a.vhead = h->fs_vhead; a.shead = h->fs_shead;
    a.repeat = h->fs_repeat;
    a.reset_bits = d_flags ? reset_bits : 0;
    a.reset_all = reset_all ? 1 : 0;
    a.flags = d_flags;
    a.game_state = d_game_state;
    a.terminal_state = d_terminal_state;
    a.frames = h->d_fs_frames;
    a.state = h->d_fs_state;
    a.terminal_stack = d_terminal_stack;
    HIP_TRY(h, launch_stack_push(a, h->stream));
    return NPP_OK;
}

int npp_frame_stack_view(npp_handle h, int which, void **base, int64_t *offset, int64_t *batch_stride) {
    if (!h || (which != 0 && which != 1) || !base || !offset || !batch_stride) return fail(h, NPP_ERR_INVALID, "npp_frame_stack_view: bad arguments");
    const int K = which == 0 ? h->fs_vk : h->fs_sk;
    if (!K) return fail(h, NPP_ERR_STATE, "npp_frame_stack_view: that stack is off (npp_set_frame_stack)");
    const int64_t E = which == 0 ? 84 * 84 : NPP_GAME_STATE_DIM;
    const int head = which == 0 ? h->fs_vhead : h->fs_shead;
    *base = which == 0 ? (void *)h->d_fs_frames : (void *)h->d_fs_state;
    *offset = (int64_t)(head + 1) * E;
    *batch_stride = (int64_t)2 * K * E;
    return NPP_OK;
}

int npp_set_entity_pos(npp_handle h, int env, int kind, double x, double y) {
    if (!h || env < 0 || env >= h->n || (kind != 0 && kind != 1)) return fail(h, NPP_ERR_INVALID, "npp_set_entity_pos: bad arguments");
    if (h->levels.empty()) return fail(h, NPP_ERR_STATE, "npp_set_entity_pos: no levels loaded");
    if (h->pool_on) return fail(h, NPP_ERR_STATE, "npp_set_entity_pos: the level pool is on (npp_set_level_pool)");
    {
        ON_DEVICE_JOINED(h);
        if (int rc = pull_levels(h)) return rc;
    }
    const CompiledLevel &L = h->levels[h->env_level[env]];
    if (L.obs_switch < 0) return fail(h, NPP_ERR_STATE, "npp_set_entity_pos: the env's level has no exit switch / door");
    ON_DEVICE_JOINED(h);
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    double *blk = h->d_zoo + (size_t)env * h->zoo_words;
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
    if (h->levels.empty()) return fail(h, NPP_ERR_STATE, "npp_switch_states: no levels loaded");
    ON_DEVICE(h);
    KernelArgs a = base_args(h);
    return obs_launch(h, a, 3, false, [&](const KernelArgs &ka, hipStream_t st) { return launch_switch_states(ka, d_out, st); });
}

int npp_reachability(npp_handle h, float *d_features, float *d_mine_sdf, int32_t *d_status) {
    return npp_reachability_ex(h, d_features, d_mine_sdf, d_status, nullptr);
}

int npp_reachability_ex(npp_handle h, float *d_features, float *d_mine_sdf, int32_t *d_status, float *d_switch_states) {
    if (!h || (!d_features && !d_mine_sdf)) return fail(h, NPP_ERR_INVALID, "npp_reachability: bad arguments");
    if (h->levels.empty()) return fail(h, NPP_ERR_STATE, "npp_reachability: no levels loaded");
    if (h->n_ovr) return fail(h, NPP_ERR_UNSUPPORTED, "npp_reachability: exit switch / door repositioned with npp_set_entity_pos");
    ON_DEVICE(h);
    const bool tables = !h->d_rhdr;
    if (int rc = ensure_reach(h)) return rc;
    KernelArgs a = base_args(h);
    return obs_launch(h, a, 2, tables, [&](const KernelArgs &ka, hipStream_t st) {   // (tables: ensure_reach has just built them)
        return launch_reach(ka, h->d_rhdr, h->d_rblob, h->d_rkey, h->d_rcache, h->rmiss, d_features, d_mine_sdf, d_status, d_switch_states, st);
    });
}

int npp_render_frame(npp_handle h, int env0, int count, uint8_t *d_out) {
    if (!h || !d_out || env0 < 0 || count <= 0 || env0 + count > h->n) return fail(h, NPP_ERR_INVALID, "npp_render_frame: bad arguments");
    if (h->levels.empty()) return fail(h, NPP_ERR_STATE, "npp_render_frame: no levels loaded");
    ON_DEVICE_JOINED(h);
    if (int rc = ensure_canvas(h)) return rc;
    KernelArgs a = base_args(h);
    HIP_TRY(h, launch_full_frame(a, env0, count, d_out, h->stream));
    return NPP_OK;
}

int npp_render_global_view(npp_handle h, uint8_t *d_out) {
    if (!h || !d_out) return fail(h, NPP_ERR_INVALID, "npp_render_global_view: bad arguments");
    if (h->levels.empty()) return fail(h, NPP_ERR_STATE, "npp_render_global_view: no levels loaded");
    ON_DEVICE(h);
    const bool tables = !h->d_gv_h || !h->d_canvas;
    if (int rc = ensure_gv(h)) return rc;
    KernelArgs a = base_args(h);
    int max_records = 0;
    for (const LevelHdr &lh : h->hdrs) max_records = std::max(max_records, (int)(lh.n_door + lh.n_ent + lh.n_mov));
    const int reorder = (h->gv_launches++ % 4) < 2;   // the order is rebuilt on launches 0, 1, 4, 5, 8, ... (costs exist from launch 1 on)
    if (h->live_parts > 1) {   // one kernel per part of a split step; the order table is rebuilt once, ahead of all of them
        if (reorder) HIP_TRY(h, launch_cost_order(h->d_gv_cost, h->d_gv_order, h->n, 0, h->stream));
        return obs_launch(h, a, 0, reorder || tables, [&](const KernelArgs &ka, hipStream_t st) {
            return launch_global_view(ka, max_records, h->d_gv_p, h->d_gv_h, h->d_gv_v, d_out, h->d_gv_x, h->d_gv_order, h->d_gv_cost, 0, st);
        });
    }
    HIP_TRY(h, launch_global_view(a, max_records, h->d_gv_p, h->d_gv_h, h->d_gv_v, d_out, h->d_gv_x, h->d_gv_order, h->d_gv_cost, reorder, h->stream));
    return NPP_OK;
}

int npp_dump_state(npp_handle h, int env0, int count, double *f64_out, int32_t *i32_out) {
    if (!h || env0 < 0 || count <= 0 || env0 + count > h->n) return fail(h, NPP_ERR_INVALID, "npp_dump_state: bad range");
    if (h->levels.empty()) return fail(h, NPP_ERR_STATE, "npp_dump_state: no levels loaded");
    ON_DEVICE_JOINED(h);
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (int rc = pull_levels(h)) return rc;
    size_t N = (size_t)h->n;
    std::vector<double> f((size_t)NF64 * count);
    std::vector<uint32_t> u((size_t)NU32 * count);
    std::vector<uint32_t> w((size_t)h->n_words_max * count);
    for (int k = 0; k < NF64; k++)
        HIP_TRY(h, hipMemcpy(f.data() + (size_t)k * count, h->d_f64 + k * N + env0, sizeof(double) * count, hipMemcpyDeviceToHost));
    for (int k = 0; k < NU32; k++)
        HIP_TRY(h, hipMemcpy(u.data() + (size_t)k * count, h->d_u32 + k * N + env0, sizeof(uint32_t) * count, hipMemcpyDeviceToHost));
    for (int k = 0; k < h->n_words_max; k++)
        HIP_TRY(h, hipMemcpy(w.data() + (size_t)k * count, h->d_ent + k * N + env0, sizeof(uint32_t) * count, hipMemcpyDeviceToHost));
    for (int i = 0; i < count; i++) {
        auto F = [&](int k) { return f[(size_t)k * count + i]; };
        uint32_t A = u[(size_t)U_A * count + i], B = u[(size_t)U_B * count + i], C = u[(size_t)U_C * count + i],
                 D = u[(size_t)U_D * count + i], E = u[(size_t)U_E * count + i];
        int gjump = (A >> 13) & 1, dslow = (A >> 14) & 1;
        if (f64_out) {
            double *o = f64_out + (size_t)i * NPP_DUMP_F64;
            o[0] = F(F_X); o[1] = F(F_Y); o[2] = F(F_VX); o[3] = F(F_VY);
            o[4] = F(F_FNX); o[5] = F(F_FNY); o[6] = F(F_CNX); o[7] = F(F_CNY);
            o[8] = F(F_VXO); o[9] = F(F_VYO);
            o[10] = gjump ? 0.01111111111111111 : 0.06666666666666665;
            o[11] = dslow ? 0.8617738760127536 : 0.9933221725495059;
        }
        if (i32_out) {
            int32_t *o = i32_out + (size_t)i * NPP_DUMP_I32;
            std::memset(o, 0, sizeof(int32_t) * NPP_DUMP_I32);
            int lvl = h->env_level[env0 + i];
            const CompiledLevel &L = h->levels[lvl];
            int sw_active = 2;
            if (L.obs_switch >= 0) sw_active = (w[(size_t)(L.obs_switch >> 4) * count + i] >> ((L.obs_switch & 15) * 2)) & 3;
            o[0] = A & 15; o[1] = (A >> 4) & 1; o[2] = (A >> 6) & 1; o[3] = (A >> 7) & 3;
            o[4] = (A >> 15) & 7; o[5] = (A >> 18) & 7; o[6] = (A >> 21) & 7; o[7] = (A >> 24) & 7;
            o[8] = (B >> 6) & 255; o[9] = (B >> 14) & 255; o[10] = B & 63;
            o[11] = !gjump; o[12] = !dslow; o[13] = sw_active;
            o[14] = (D >> 16) & 255; o[15] = D >> 24; o[16] = C & 0xffff; o[17] = C >> 16;
            o[18] = (A >> 5) & 1; o[19] = (A >> 9) & 1; o[20] = (A >> 27) & 3; o[21] = (A >> 29) & 1;
            o[22] = D & 0xffff; o[23] = (int)((A >> 10) & 3) - 1; o[24] = (A >> 12) & 1; o[25] = (B >> 22) & 15;
            o[26] = E & 0xffff; o[27] = lvl;
        }
    }
    return NPP_OK;
}

int npp_dump_entities(npp_handle h, int env, int32_t *out, int max, int *n_out) {
    if (!h || env < 0 || env >= h->n || !out || !n_out) return fail(h, NPP_ERR_INVALID, "npp_dump_entities: bad arguments");
    if (h->levels.empty()) return fail(h, NPP_ERR_STATE, "npp_dump_entities: no levels loaded");
    ON_DEVICE_JOINED(h);
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (int rc = pull_levels(h)) return rc;
    const CompiledLevel &L = h->levels[h->env_level[env]];
    std::vector<uint32_t> w(h->n_words_max);
    for (int k = 0; k < h->n_words_max; k++)
        HIP_TRY(h, hipMemcpy(&w[k], h->d_ent + (size_t)k * h->n + env, sizeof(uint32_t), hipMemcpyDeviceToHost));
    int n = (int)L.ent_map_order.size();
    if (n > max) n = max;
    for (int i = 0; i < n; i++) {
        int slot = L.ent_map_order[i];
        out[i] = (w[slot >> 4] >> ((slot & 15) * 2)) & 3;
    }
    *n_out = n;
    return NPP_OK;
}

int npp_entity_checksum(npp_handle h, int env0, int count, double *out) {
    if (!h || env0 < 0 || count <= 0 || env0 + count > h->n || !out) return fail(h, NPP_ERR_INVALID, "npp_entity_checksum: bad arguments");
    if (h->levels.empty()) return fail(h, NPP_ERR_STATE, "npp_entity_checksum: no levels loaded");
    ON_DEVICE_JOINED(h);
    HIP_TRY(h, hipStreamSynchronize(h->stream));
    if (int rc = pull_levels(h)) return rc;
    size_t N = (size_t)h->n;
    std::vector<uint32_t> w((size_t)h->n_words_max * count);
    for (int k = 0; k < h->n_words_max; k++)
        HIP_TRY(h, hipMemcpy(w.data() + (size_t)k * count, h->d_ent + k * N + env0, sizeof(uint32_t) * count, hipMemcpyDeviceToHost));
    std::vector<double> zb;
    if (h->d_zoo) {
        zb.resize((size_t)h->zoo_words * count);
        HIP_TRY(h, hipMemcpy(zb.data(), h->d_zoo + (size_t)env0 * h->zoo_words, sizeof(double) * zb.size(), hipMemcpyDeviceToHost));
    }
    const int door_words = (h->zoo_doors + 1) / 2;
    for (int i = 0; i < count; i++) {
        const CompiledLevel &L = h->levels[h->env_level[env0 + i]];
        const double *blk = h->d_zoo ? zb.data() + (size_t)i * h->zoo_words : nullptr;
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
                uint32_t st = (w[(size_t)(s >> 4) * count + i] >> ((s & 15) * 2)) & 3u;
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
    if (!h || level < 0 || level >= (int)h->levels.size() || !out || !n_out)
        return fail(h, NPP_ERR_INVALID, "npp_dump_level_segments: bad arguments");
    int r = dump_segments(h->levels[level], out, max_rows);
    if (r < 0) return fail(h, NPP_ERR_INVALID, "npp_dump_level_segments: buffer too small");
    *n_out = r;
    return NPP_OK;
}

}  // extern "C"
