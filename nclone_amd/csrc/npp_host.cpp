// npp_host.cpp -- the host-only entry points of include/npp_amd.h (no GPU, no handle): the level compiler's views for the CPU
// test-suite, the zoo block plan, the dynamic truncation limit.  No HIP header is included, so this file, npp_level.cpp and
// npp_reach.cpp also build with plain g++ (tools/build_sanitized.sh: -fsanitize=address,undefined).
#include "npp_host.hpp"

#include <cstring>

#include "../../include/npp_amd.h"
#include "npp_augment.hpp"
#include "npp_cells.hpp"
#include "npp_demo.hpp"
#include "npp_episode.hpp"
#include "npp_minimal.hpp"
#include "npp_pathmask.hpp"
#include "npp_pool.hpp"
#include "npp_reach_build.hpp"
#include "npp_route.hpp"
#include "npp_seed.hpp"
#include "npp_sweep.hpp"

using namespace npp;

namespace npp {
std::string &host_error() {
    static thread_local std::string e;
    return e;
}
}  // namespace npp

namespace {
int fail(std::nullptr_t, int code, const std::string &msg) {
    host_error() = msg;
    return code;
}
}  // namespace

extern "C" {

int npp_minimal_encode_host(const uint32_t *state_a, const double *planes, int count, float *out) {
    if (count < 0 || (count > 0 && (!state_a || !planes || !out))) return fail(nullptr, NPP_ERR_INVALID, "npp_minimal_encode_host: bad arguments");
    for (int i = 0; i < count; i++)
        minobs_encode_state(state_a[i], planes[4 * i], planes[4 * i + 1], planes[4 * i + 2], planes[4 * i + 3], out + (size_t)i * MINOBS_DIM);
    return NPP_OK;
}

int npp_state_decode_host(const uint32_t words[5], int32_t *out) {
    static_assert(STATE_DUMP_I32 == NPP_DUMP_I32 && NU32 == 5, "the row npp_dump_state documents");
    if (!words || !out) return fail(nullptr, NPP_ERR_INVALID, "npp_state_decode_host: bad arguments");
    state_decode_row(words, EXIT_SWITCH_NONE, 0, out);
    return NPP_OK;
}

int npp_level_pool_draw_host(const double *weights, int n_levels, uint64_t seed, const int32_t *envs, const uint32_t *counts, int count,
                             int32_t *out) {
    if (count < 0 || (count > 0 && (!envs || !counts || !out))) return fail(nullptr, NPP_ERR_INVALID, "npp_level_pool_draw_host: bad arguments");
    std::vector<double> cdf;
    int last = 0;
    std::string err;
    if (!pool_cdf(weights, n_levels, n_levels, cdf, last, err)) return fail(nullptr, NPP_ERR_INVALID, err);
    for (int i = 0; i < count; i++) out[i] = pool_pick(cdf.data(), n_levels, last, seed, (uint32_t)envs[i], counts[i]);
    return NPP_OK;
}

int npp_frame_augment_params_host(uint64_t seed, double p, double scale, const int32_t *envs, const uint32_t *counts, const int32_t *targets,
                                  int count, int32_t *out) {
    if (count < 0 || (count > 0 && (!envs || !counts || !targets || !out)))
        return fail(nullptr, NPP_ERR_INVALID, "npp_frame_augment_params_host: bad arguments");
    if (!(p >= 0.0 && p <= 1.0)) return fail(nullptr, NPP_ERR_INVALID, "npp_frame_augment_params_host: p must be between 0.0 and 1.0");
    const int s10 = scale == 0.7 ? 7 : scale == 1.0 ? 10 : scale == 1.3 ? 13 : 0;
    if (!s10) return fail(nullptr, NPP_ERR_INVALID, "npp_frame_augment_params_host: scale must be 0.7 (light), 1.0 (medium) or 1.3 (strong)");
    for (int i = 0; i < count; i++) {
        if (targets[i] != 0 && targets[i] != 1) return fail(nullptr, NPP_ERR_INVALID, "npp_frame_augment_params_host: target must be 0 or 1");
        const AugParams P = aug_draw(seed, (uint32_t)envs[i], counts[i], targets[i], p, s10);
        std::memcpy(out + (size_t)i * AUG_WORDS, &P, sizeof(P));
    }
    return NPP_OK;
}

int npp_frame_augment_apply_host(const uint8_t *frames, int count, int height, int width, const int32_t *params, uint8_t *out) {
    if (count < 0 || height <= 0 || width <= 0 || height > 1024 || width > 1024 || (count > 0 && (!frames || !params || !out)))
        return fail(nullptr, NPP_ERR_INVALID, "npp_frame_augment_apply_host: bad arguments");
    const size_t E = (size_t)height * width;
    for (int i = 0; i < count; i++) {
        AugParams P;
        std::memcpy(&P, params + (size_t)i * AUG_WORDS, sizeof(P));
        if (!aug_params_ok(P, height, width)) return fail(nullptr, NPP_ERR_INVALID, "npp_frame_augment_apply_host: parameters outside the image");
        for (int y = 0; y < height; y++)
            for (int x = 0; x < width; x++) out[i * E + (size_t)y * width + x] = aug_pixel(frames + i * E, height, width, P, y, x);
    }
    return NPP_OK;
}

int npp_archive_cell_keys_host(const double *map, int64_t n, int level, const double *xy, const int32_t *state, const int32_t *switch_state,
                                int count, int32_t *keys_out) {
    if (!map || level < 0 || count < 0 || (count > 0 && (!xy || !state || !switch_state || !keys_out)))
        return fail(nullptr, NPP_ERR_INVALID, "npp_archive_cell_keys_host: bad arguments");
    CompiledLevel L;
    std::string err;
    if (!compile_level(map, n, L, err)) return fail(nullptr, NPP_ERR_INVALID, "npp_archive_cell_keys_host: " + err);
    const bool has_door = L.obs_switch >= 0 && L.obs_door >= 0;
    const double door_x = has_door ? L.ent_x[L.obs_door] : 0.0, door_y = has_door ? L.ent_y[L.obs_door] : 0.0;
    for (int i = 0; i < count; i++) {
        const int k = cell_key_in_level(state[i], switch_state[i], xy[2 * i], xy[2 * i + 1], has_door, door_x, door_y);
        keys_out[i] = k < 0 ? -1 : level * NPP_CELLS_PER_LEVEL + k;
    }
    return NPP_OK;
}

int npp_archive_cell_pick_host(const int32_t *cell_slot, const uint32_t *visits, const uint32_t *chosen, uint64_t seed, uint32_t call,
                                const int32_t *envs, int count, int32_t *slots_out) {
    if (!cell_slot || !visits || !chosen || count < 0 || (count > 0 && (!envs || !slots_out)))
        return fail(nullptr, NPP_ERR_INVALID, "npp_archive_cell_pick_host: bad arguments");
    std::vector<uint64_t> cdf(NPP_CELLS_PER_LEVEL);
    uint64_t run = 0;
    for (int k = 0; k < NPP_CELLS_PER_LEVEL; k++) {
        if (cell_slot[k] >= 0) run += cell_weight(visits[k], chosen[k]);
        cdf[k] = run;
    }
    for (int i = 0; i < count; i++) slots_out[i] = run ? cell_slot[cell_pick(cdf.data(), seed, (uint32_t)envs[i], call)] : -1;
    return NPP_OK;
}

int npp_route_apply_host(int32_t *hdr, uint8_t *actions, int capacity, int autoreset, const int32_t *events, int count,
                         const uint8_t *restore_bytes) {
    if (!hdr || !actions || capacity <= 0 || capacity % 16 || count < 0 || (count > 0 && !events))
        return fail(nullptr, NPP_ERR_INVALID, "npp_route_apply_host: bad arguments (capacity must be a positive multiple of 16)");
    if ((hdr[ROUTE_CUR] != 0 && hdr[ROUTE_CUR] != 1) || hdr[R_LEN] < 0 || hdr[R_LEN] > capacity)
        return fail(nullptr, NPP_ERR_INVALID, "npp_route_apply_host: header word 12 must be 0 or 1 and word 0 within the capacity");
    for (int i = 0; i < count; i++) {
        const int32_t *ev = events + (size_t)i * 8;
        switch (ev[0]) {
        case 0: route_step(hdr, actions, capacity, ev[1], ev[2], ev[3], ev[4], ev[5], autoreset != 0); break;
        case 1: route_flip(hdr); break;
        case 2: route_tick(hdr); break;
        case 3:
            if (ev[1 + R_LEN] < 0 || ev[1 + R_LEN] > capacity || (ev[1 + R_LEN] > 0 && (!restore_bytes || ev[7] < 0)))
                return fail(nullptr, NPP_ERR_INVALID, "npp_route_apply_host: event " + std::to_string(i) + ": bad route to restore from");
            route_restore(hdr, actions, capacity, ev + 1, restore_bytes ? restore_bytes + ev[7] : nullptr);
            break;
        default: return fail(nullptr, NPP_ERR_INVALID, "npp_route_apply_host: event " + std::to_string(i) + ": unknown kind");
        }
    }
    return NPP_OK;
}

int npp_path_direction_host(const double *map, int64_t n, const double *pos, const uint8_t *switch_activated, int count,
                            int8_t *direction_out, uint8_t *from_graph_out, int32_t *status) {
    return npp_path_direction_goal_host(map, n, nullptr, pos, switch_activated, count, direction_out, from_graph_out, status);
}

int npp_path_direction_goal_host(const double *map, int64_t n, const double *goal_xy, const double *pos, const uint8_t *switch_activated, int count,
                                 int8_t *direction_out, uint8_t *from_graph_out, int32_t *status) {
    if (!map || count < 0 || (count > 0 && (!pos || !switch_activated || !direction_out)))
        return fail(nullptr, NPP_ERR_INVALID, "npp_path_direction_host: bad arguments");
    ReachBuilt R;
    std::string err;
    if (!build_reach_variant(map, n, goal_xy, R, err)) return fail(nullptr, NPP_ERR_INVALID, "npp_path_direction_host: " + err);
    ReachHdr H;
    std::vector<unsigned char> blob;
    pack_reach(R, H, blob);
    const ReachTabs T{&H, blob.data() + H.base};
    for (int k = 0; k < count; k++) {
        int from_graph = 0;
        direction_out[k] = (int8_t)reach_path_direction(T, pos[2 * k], pos[2 * k + 1], switch_activated[k] != 0, &from_graph);
        if (from_graph_out) from_graph_out[k] = (uint8_t)from_graph;
    }
    if (status) *status = H.supported ? 0 : 2;
    return NPP_OK;
}

int npp_compile_level_segments(const double *map, int64_t n, int16_t *out, int max_rows, int *n_out, uint32_t *unsupported_mask) {
    return npp_compile_level_segments_goal(map, n, nullptr, out, max_rows, n_out, unsupported_mask);
}

int npp_compile_level_segments_goal(const double *map, int64_t n, const double *goal_xy, int16_t *out, int max_rows, int *n_out,
                                    uint32_t *unsupported_mask) {
    if (!map || !out || !n_out) return fail(nullptr, NPP_ERR_INVALID, "npp_compile_level_segments: bad arguments");
    CompiledLevel L;
    std::string err;
    if (!compile_level_variant(map, n, goal_xy, L, err)) return fail(nullptr, NPP_ERR_INVALID, "npp_compile_level_segments: " + err);
    int r = dump_segments(L, out, max_rows);
    if (r < 0) return fail(nullptr, NPP_ERR_INVALID, "npp_compile_level_segments: buffer too small");
    *n_out = r;
    if (unsupported_mask) *unsupported_mask = L.unsupported_mask;
    return NPP_OK;
}

int npp_compile_level_zoo(const double *map, int64_t n, int32_t *edges_out, double *movers_out, int max_movers, int *n_movers) {
    if (!map || !edges_out || !n_movers) return fail(nullptr, NPP_ERR_INVALID, "npp_compile_level_zoo: bad arguments");
    CompiledLevel L;
    std::string err;
    if (!compile_level(map, n, L, err)) return fail(nullptr, NPP_ERR_INVALID, "npp_compile_level_zoo: " + err);
    const int NK = EDGE_W * EDGE_H;
    for (int k = 0; k < NK; k++) {
        edges_out[k] = (int32_t)((L.edges[k >> 5] >> (k & 31)) & 1u);
        edges_out[NK + k] = (int32_t)((L.edges[EDGE_WORDS + (k >> 5)] >> (k & 31)) & 1u);
    }
    for (size_t d = 0; d + 1 < L.door_tab.size(); d += 2) {
        uint32_t keys[2] = {L.door_tab[d] & 0xffffu, L.door_tab[d] >> 16};
        for (uint32_t k : keys) edges_out[((k & 0x8000u) ? NK : 0) + (int)(k & 0x7fffu)] += (int32_t)(L.door_tab[d + 1] & 0xffu);
    }
    int nm = (int)L.mov_meta.size();
    if (movers_out) {
        if (nm > max_movers) return fail(nullptr, NPP_ERR_INVALID, "npp_compile_level_zoo: buffer too small");
        static const double type_of[7] = {0, 14, 17, 20, 25, 26, 28};
        for (int m = 0; m < nm; m++) {
            movers_out[4 * m] = type_of[L.mov_meta[m] & 7u];
            movers_out[4 * m + 1] = L.mov_x0[m];
            movers_out[4 * m + 2] = L.mov_y0[m];
            movers_out[4 * m + 3] = (double)(L.mov_meta[m] >> 8);
        }
    }
    *n_movers = nm;
    return NPP_OK;
}

int npp_plan_zoo_block(const double *blob, const int64_t *offsets, int n_levels, int *doors, int *movers, int *words) {
    if (!blob || !offsets || n_levels <= 0) return fail(nullptr, NPP_ERR_INVALID, "npp_plan_zoo_block: bad arguments");
    std::vector<CompiledLevel> lv(n_levels);
    for (int i = 0; i < n_levels; i++) {
        std::string err;
        if (offsets[i + 1] < offsets[i] || !compile_level(blob + offsets[i], offsets[i + 1] - offsets[i], lv[i], err))
            return fail(nullptr, NPP_ERR_INVALID, "npp_plan_zoo_block: level " + std::to_string(i) + ": " + err);
    }
    int d = 0, m = 0;
    zoo_block_plan(lv, d, m);
    if (doors) *doors = d;
    if (movers) *movers = m;
    if (words) *words = zoo_words_for(d, m);
    return NPP_OK;
}

int npp_compile_level_entities(const double *map, int64_t n, double *out, int max_rows, int *n_out) {
    return npp_compile_level_entities_goal(map, n, nullptr, out, max_rows, n_out, nullptr);
}

int npp_compile_level_entities_goal(const double *map, int64_t n, const double *goal_xy, double *out, int max_rows, int *n_out, int32_t *order) {
    if (!map || !out || !n_out) return fail(nullptr, NPP_ERR_INVALID, "npp_compile_level_entities: bad arguments");
    CompiledLevel L;
    std::string err;
    if (!compile_level_variant(map, n, goal_xy, L, err)) return fail(nullptr, NPP_ERR_INVALID, "npp_compile_level_entities: " + err);
    for (size_t i = 0; order && i < L.ent_map_order.size() && (int)i < max_rows; i++) {   // per entity in map order: CSR slot, list-order
        const int s = L.ent_map_order[i];                                                   // numbers after reset / fast reset, fast walk place
        int walk = 0;
        while (L.ent_perm[walk] != s) walk++;
        order[4 * i] = s; order[4 * i + 1] = L.ent_seq[s]; order[4 * i + 2] = L.ent_rank[s]; order[4 * i + 3] = walk;
    }
    int ne = (int)L.ent_map_order.size();
    if (ne > max_rows) return fail(nullptr, NPP_ERR_INVALID, "npp_compile_level_entities: buffer too small");
    // cell of a slot from the CSR
    std::vector<int> cell_of_slot(ne, 0);
    for (int c = 0; c < N_CELLS; c++)
        for (int s = L.ent_start[c]; s < L.ent_start[c + 1]; s++) cell_of_slot[s] = c;
    for (int i = 0; i < ne; i++) {
        int s = L.ent_map_order[i];
        double *o = out + (size_t)i * 6;
        o[0] = L.ent_meta[s] & 15u;
        o[1] = L.ent_x[s];
        o[2] = L.ent_y[s];
        o[3] = cell_of_slot[s] / GRID_H;
        o[4] = cell_of_slot[s] % GRID_H;
        o[5] = (L.ent_meta[s] >> 4) & 3u;
    }
    *n_out = ne;
    return NPP_OK;
}


int npp_level_truncation_limit(const double *map, int64_t n, int32_t *limit, int32_t *surface_area) {
    if (!map) return NPP_ERR_INVALID;
    ReachBuilt R;
    std::string err;
    if (!build_reach(map, n, R, err)) return NPP_ERR_INVALID;
    if (limit) *limit = truncation_limit_for_area(R.spawn_area);
    if (surface_area) *surface_area = R.spawn_area;
    return NPP_OK;
}

int npp_demo_plan_host(const int64_t *lengths, int n_replays, int frame_skip, int64_t max_transitions, int n_envs, int32_t *rows,
                       int64_t *row_base, int32_t *order, int32_t *round_ticks, int32_t *counts, int64_t *rows_total) {
    DemoPlan p;
    const char *why = nullptr;
    if (!demo_plan(lengths, n_replays, frame_skip, max_transitions, n_envs, p, &why))   // a refusal writes nothing
        return fail(nullptr, NPP_ERR_INVALID, std::string("npp_demo_plan_host: ") + why);
    for (int r = 0; r < n_replays; r++) {
        if (rows) rows[r] = p.rows[r];
        if (row_base) row_base[r] = p.row_base[r];
        if (order) order[r] = (size_t)r < p.order.size() ? p.order[r] : -1;
        if (round_ticks) round_ticks[r] = (size_t)r < p.round_ticks.size() ? p.round_ticks[r] : 0;
    }
    if (counts) { counts[0] = (int32_t)p.order.size(); counts[1] = (int32_t)p.round_ticks.size(); }
    if (rows_total) *rows_total = p.rows_total;
    return NPP_OK;
}

int npp_episode_apply_host(int32_t *rec_i32, double *rec_f64, uint64_t *table, int n_levels, int autoreset, const int32_t *events,
                           const float *rows, int count, uint8_t *ended) {
    static_assert(EP_NI == NPP_EP_NI && EP_ND == NPP_EP_ND && EP_FIN == NPP_EP_FIN && EP_DFIN == NPP_EP_DFIN && EP_COLS == NPP_EP_COLS &&
                      EP_FIN_FLAGS == NPP_EP_FIN_FLAGS && EP_N_FINISHED == NPP_EP_N_FINISHED && EP_COMP == NPP_EP_COMP &&
                      (int)EPC_ABANDONED == (int)NPP_EPC_ABANDONED && (int)EP_BITS == (int)NPP_EP_BITS,
                  "the planes and columns include/npp_amd.h documents");
    if (!rec_i32 || !rec_f64 || n_levels < 0 || (n_levels > 0 && !table) || count < 0 || (count > 0 && !events))
        return fail(nullptr, NPP_ERR_INVALID, "npp_episode_apply_host: bad arguments");
    EpRecord r;
    for (int k = 0; k < EP_NI; k++) r.i[k] = rec_i32[k];
    for (int k = 0; k < EP_ND; k++) r.d[k] = rec_f64[k];
    bool any = false;
    for (int i = 0; i < count; i++) {
        const int32_t *ev = events + (size_t)i * 8;
        if (ev[0] == 0) {
            if (ev[1] < 0 || ev[1] > 255 || ev[2] < 0 || ev[2] > 65535 || !rows)
                return fail(nullptr, NPP_ERR_INVALID, "npp_episode_apply_host: event " + std::to_string(i) + ": bad step row");
            const float *row = rows + (size_t)i * 8;
            const bool end = ev[4] ? ep_row<true>(r, ev[1], ev[2], row[0], row + 1, ev[3], autoreset != 0)
                                   : ep_row<false>(r, ev[1], ev[2], row[0], nullptr, ev[3], autoreset != 0);
            if (end) {
                any = true;
                const int level = r.i[EP_FIN + EP_LEVEL];
                if (level >= 0 && level < n_levels) {
                    uint64_t d[EP_COLS];
                    ep_deltas(r, d);
                    for (int k = 0; k < EP_COLS; k++) table[(size_t)level * EP_COLS + k] += d[k];
                }
            }
        } else if (ev[0] >= 1 && ev[0] <= 5) {
            static const int kind[6] = {0, EP_EV_RESET, EP_EV_RESTORE, EP_EV_TICK, EP_EV_INIT, EP_EV_CLEAR};
            const int charged = ep_event(r, kind[ev[0]], ev[1]);
            if (charged >= 0 && charged < n_levels) table[(size_t)charged * EP_COLS + EPC_ABANDONED] += 1;
        } else {
            return fail(nullptr, NPP_ERR_INVALID, "npp_episode_apply_host: event " + std::to_string(i) + ": unknown kind");
        }
    }
    for (int k = 0; k < EP_NI; k++) rec_i32[k] = r.i[k];
    for (int k = 0; k < EP_ND; k++) rec_f64[k] = r.d[k];
    if (ended) *ended = any ? 1 : 0;
    return NPP_OK;
}

int npp_sweep_assign_host(const uint8_t *flags, int end_bits, int n_envs, const int32_t *jobs, int n_jobs, int32_t *counters, int32_t *env_job,
                          int32_t *prev_job, int32_t *env_level, int32_t *trunc, const int32_t *level_trunc, int n_levels, uint8_t *changed) {
    static_assert(SWEEP_RI == NPP_SWEEP_RI && SWEEP_RD == NPP_SWEEP_RD && SWEEP_R_FLAGS == NPP_SWEEP_R_FLAGS && SWEEP_R_ENV == NPP_SWEEP_R_ENV &&
                      SWEEP_R_STATUS == NPP_SWEEP_R_STATUS,
                  "the result planes include/npp_amd.h documents");
    if (n_envs < 0 || n_jobs < 0 || n_levels < 0 || !counters || (n_jobs > 0 && !jobs) ||
        (n_envs > 0 && (!flags || !env_job || !prev_job || !env_level || !changed || (level_trunc && !trunc))))
        return fail(nullptr, NPP_ERR_INVALID, "npp_sweep_assign_host: bad arguments");
    if (counters[SWEEP_NEXT] < 0 || counters[SWEEP_NEXT] > n_jobs + n_envs)
        return fail(nullptr, NPP_ERR_INVALID, "npp_sweep_assign_host: next outside 0 .. n_jobs + n_envs");
    for (int j = 0; j < n_jobs; j++)
        if (jobs[j] < 0 || (level_trunc && jobs[j] >= n_levels))
            return fail(nullptr, NPP_ERR_INVALID, "npp_sweep_assign_host: job " + std::to_string(j) + ": level id out of range");
    for (int e = 0; e < n_envs; e++)
        if (env_job[e] < -1 || env_job[e] >= n_jobs)
            return fail(nullptr, NPP_ERR_INVALID, "npp_sweep_assign_host: env " + std::to_string(e) + ": job out of range");
    counters[SWEEP_NEXT] += sweep_assign_row(flags, end_bits, n_envs, jobs, n_jobs, counters[SWEEP_NEXT], env_job, prev_job, env_level, trunc,
                                             level_trunc, changed);
    return NPP_OK;
}

int npp_archive_seed_rows_host(const uint8_t *in, int64_t len, int score_mode, uint8_t *actions, uint8_t *route_bits, float *scores) {
    if (len < 0 || (len > 0 && !in)) return fail(nullptr, NPP_ERR_INVALID, "npp_archive_seed_rows_host: bad arguments");
    if (score_mode != SEED_PROGRESS && score_mode != SEED_FRAMES)
        return fail(nullptr, NPP_ERR_INVALID, "npp_archive_seed_rows_host: score_mode must be 0 (progress) or 1 (frames)");
    bool latch = false;
    for (int64_t f = 0; f < len; f++) {
        latch = latch || seed_byte_mismatch(in[f]);
        if (actions) actions[f] = demo_action_of_byte(in[f]);
        if (route_bits) route_bits[f] = latch ? (uint8_t)ROUTE_BROKEN : (uint8_t)0;
        if (scores) scores[f] = seed_score(score_mode, f, len);
    }
    return NPP_OK;
}

}  // extern "C"
