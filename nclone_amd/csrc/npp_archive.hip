// npp_archive.hip -- the two kernels that move one env's state between the live planes and a record (npp_archive.hpp): entry i
// moves env envs[i] into record slots[i] (store) or back (restore); without lists entry i is env i and record i, under an optional
// env mask (the snapshot slot).  One wavefront per entry: the strided [plane][n] planes go one plane per lane, the contiguous
// rows (zoo block, spatial-context cache, reachability row, route bytes) and the record go over consecutive lanes, so the record side of an
// entry is one contiguous stream.  Everything that decides an entry (the two list values or the mask byte, the slot's "stored"
// word and level) is wave-uniform; lane 0 writes the status and the meta row.  An entry whose status is not 0 reads only the list
// values (and, restore, the slot's meta and level words once both indices are known to be in range) and writes only its status.
#include <hip/hip_runtime.h>

#include "npp_archive.hpp"

namespace npp {
namespace {

constexpr int ENTRIES_PER_BLOCK = 4;   // 256 threads

template <bool STORE> __global__ __launch_bounds__(256) void npp_archive_kernel(ArchiveArgs a) {
    const int lane = threadIdx.x & (WAVE - 1);
    const int i = blockIdx.x * ENTRIES_PER_BLOCK + (threadIdx.x >> 6);
    if (i >= a.count) return;
    const ArchiveLayout &L = a.lay;
    int env = i, slot = i;
    if (a.envs) { env = a.envs[i]; slot = a.slots[i]; }
    else if (a.mask && a.mask[i] == 0) env = -1;
    uint32_t *rec = nullptr;
    int st = ARCHIVE_DONE;
    if (env < 0 || slot < 0) {
        st = ARCHIVE_SKIPPED;
    } else if (env >= a.n || slot >= a.n_slots) {
        st = ARCHIVE_RANGE;
    } else {
        rec = a.rec + (size_t)slot * L.words;
        if (!STORE) {
            if (a.meta_i32 && a.meta_i32[(size_t)slot * ARCHIVE_META_I32] == 0) st = ARCHIVE_EMPTY;
            else if (!a.level_out && (int32_t)rec[L.off_tail + 1] != a.env_level[env]) st = ARCHIVE_LEVEL_MISMATCH;
        }
    }
    if (lane == 0 && a.status) a.status[i] = st;
    if (st != ARCHIVE_DONE) return;

    const size_t N = (size_t)a.n, e = (size_t)env;
    double *rec64 = reinterpret_cast<double *>(rec);   // the f64 planes and the zoo block: words [0, off_u32)
    // strided planes, one per lane
    for (int k = lane; k < NF64; k += WAVE) {
        if (STORE) rec64[k] = a.f64[k * N + e];
        else a.f64[k * N + e] = rec64[k];
    }
    for (int k = lane; k < NU32 + L.n_words_max; k += WAVE) {   // (off_ent == off_u32 + NU32: one run of the record)
        uint32_t *live = k < NU32 ? a.u32 + k * N + e : a.ent + (size_t)(k - NU32) * N + e;
        if (STORE) rec[L.off_u32 + k] = *live;
        else *live = rec[L.off_u32 + k];
    }
    // contiguous rows, consecutive lanes
    if (a.zoo) {
        double *live = a.zoo + e * L.zoo_words;
        for (int k = lane; k < L.zoo_words; k += WAVE) {
            if (STORE) rec64[NF64 + k] = live[k];
            else live[k] = rec64[NF64 + k];
        }
    }
    if (lane < ARCHIVE_SC) {
        float *live = a.sc + e * ARCHIVE_SC + lane;
        if (STORE) rec[L.off_sc + lane] = __float_as_uint(*live);
        else *live = __uint_as_float(rec[L.off_sc + lane]);
    }
    if (L.route_cap) {
        // the env's current route (npp_route.hpp): header words by the first lanes, then the first `len` bytes, rounded up to 16,
        // 16 per lane (cap is a multiple of 16 and both sides are 16-byte aligned).  A restore leaves the env's finished route and
        // its buffer choice (word 12) alone.
        int32_t *hdr = a.route_hdr + e * ROUTE_HDR_WORDS;
        const int cur = hdr[ROUTE_CUR] & 1;
        uint4 *live = reinterpret_cast<uint4 *>(a.route_act + (e * 2 + cur) * L.route_cap);
        uint4 *recb = reinterpret_cast<uint4 *>(rec + L.off_route + ROUTE_REC_HDR_WORDS);
        int len = STORE ? hdr[R_LEN] : (int32_t)rec[L.off_route + R_LEN];
        len = len < 0 ? 0 : (len > L.route_cap ? L.route_cap : len);
        if (lane < ROUTE_REC_HDR_WORDS) {
            if (STORE) rec[L.off_route + lane] = lane < ROUTE_WORDS ? (uint32_t)hdr[lane] : 0u;
            else if (lane < ROUTE_WORDS) hdr[lane] = (int32_t)rec[L.off_route + lane];
        }
        for (int k = lane; k < (len + 15) / 16; k += WAVE) {
            if (STORE) recb[k] = live[k];
            else live[k] = recb[k];
        }
    }
    if (STORE) {
        const bool reach = a.reach_key != nullptr;
        if (lane < ARCHIVE_REACH_ROW) rec[L.off_reach + 1 + lane] = reach ? __float_as_uint(a.reach_cache[e * ARCHIVE_REACH_ROW + lane]) : 0u;
        if (lane == 0) {
            const int level = a.env_level[env];
            rec[L.off_reach] = reach ? a.reach_key[env] : 0u;
            rec[L.off_tail] = (uint32_t)a.trunc[env];
            rec[L.off_tail + 1] = (uint32_t)level;
            rec[L.off_tail + 2] = reach ? 1u : 0u;
            rec[L.off_tail + 3] = a.draws[env];
            if (a.meta_i32) {   // the meta row, with npp_dump_state's decode
                const double x = a.f64[F_X * N + e], y = a.f64[F_Y * N + e];
                double *mf = a.meta_f64 + (size_t)slot * ARCHIVE_META_F64;
                mf[0] = x; mf[1] = y; mf[2] = a.f64[F_VX * N + e]; mf[3] = a.f64[F_VY * N + e];
                const int sw_state = exit_switch_state(a.ent, N, e, a.hdr[level].obs_switch);
                int32_t *mi = a.meta_i32 + (size_t)slot * ARCHIVE_META_I32;
                mi[1] = level;
                mi[2] = state_load(a.u32, N, e, S_FRAME);
                mi[3] = (int32_t)floor(x / 24.0);
                mi[4] = (int32_t)floor(y / 24.0);
                mi[5] = exit_switch_activated(sw_state);
                mi[0] = 1;
            }
        }
    } else {
        if (lane == 0) {
            if (a.trunc) a.trunc[env] = (int32_t)rec[L.off_tail];
            if (a.level_out) a.level_out[env] = (int32_t)rec[L.off_tail + 1];
            if (a.draws) a.draws[env] = rec[L.off_tail + 3];
        }
        if (a.reach_key) {
            // "reset + replay" (base_environment.py:1769-1789): the path calculator's per-episode dictionary is empty afterwards
            if (lane == 0 && a.reach_last_episode) a.reach_last_episode[env] = 0xffffffffu;
            if (rec[L.off_tail + 2]) {
                if (lane == 0) a.reach_key[env] = rec[L.off_reach];
                if (lane < ARCHIVE_REACH_ROW) a.reach_cache[e * ARCHIVE_REACH_ROW + lane] = __uint_as_float(rec[L.off_reach + 1 + lane]);
            } else if (lane == 0) {
                a.reach_key[env] = 0u;   // stored before the first npp_reachability: no cached vector
            }
        }
    }
}

template <bool STORE> hipError_t launch(const ArchiveArgs &a, hipStream_t s) {
    if (a.count <= 0) return hipSuccess;
    hipLaunchKernelGGL(npp_archive_kernel<STORE>, dim3((a.count + ENTRIES_PER_BLOCK - 1) / ENTRIES_PER_BLOCK), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_archive_store(const ArchiveArgs &a, hipStream_t s) { return launch<true>(a, s); }
hipError_t launch_archive_restore(const ArchiveArgs &a, hipStream_t s) { return launch<false>(a, s); }

}  // namespace npp
