// npp_archive.hpp -- the record of one env's state and the two kernels that move it between the live planes and a record
// (npp_archive.hip).  The checkpoint archive (include/npp_amd.h, npp_archive_create) is n_slots such records addressed by device
// lists; the snapshot slot (npp_snapshot / npp_restore) is n of them, record e for env e.
#pragma once
#include <hip/hip_runtime_api.h>

#include <cstdint>

#include "npp_internal.hpp"
#include "npp_reach.hpp"
#include "npp_route.hpp"

namespace npp {

// One contiguous record of 4-byte words, all the per-env state there is: a feature that adds some adds it HERE and to the kernel
// (offsets in words; the two f64 sections come first, so they are 8-byte aligned in a record whose size is a multiple of 16 bytes):
//   f64   [2 NF64]          the double planes, plane order
//   zoo   [2 zoo_words]     the zoo block (absent when the level set has none)
//   u32   [NU32]            the word planes
//   ent   [n_words_max]     entity words
//   sc    [48]              spatial-context cache row (floats)
//   reach [1 + REACH_DIM+1] key, then the cache row (floats); meaningful only when tail word 2 is set
//   tail  [4]               truncation limit, level, 1 = the record holds a reachability key / row, level pool draw count
//   route [8 + cap / 4]     (only with action routes on, npp_set_routes) the env's CURRENT route: its six header words
//                           (npp_route.hpp), two zero words, then the action bytes -- of which store and restore move only the
//                           first `len`, rounded up to 16, so a record's traffic follows its route and not the capacity
struct ArchiveLayout {
    int zoo_words = 0, n_words_max = 0;
    int off_zoo = 0, off_u32 = 0, off_ent = 0, off_sc = 0, off_reach = 0, off_tail = 0;
    int route_cap = 0, off_route = 0;   // route_cap: bytes per route buffer, a multiple of 16; 0 = the record has no route section
    int words = 0;   // record size, a multiple of 4
};
constexpr int ARCHIVE_SC = 48, ARCHIVE_REACH_ROW = REACH_DIM + 1;
inline ArchiveLayout archive_layout(int n_words_max, int zoo_words, int route_cap = 0) {
    ArchiveLayout L;
    L.zoo_words = zoo_words;
    L.n_words_max = n_words_max;
    L.off_zoo = 2 * NF64;
    L.off_u32 = L.off_zoo + 2 * zoo_words;
    L.off_ent = L.off_u32 + NU32;
    L.off_sc = L.off_ent + n_words_max;
    L.off_reach = L.off_sc + ARCHIVE_SC;
    L.off_tail = L.off_reach + 1 + ARCHIVE_REACH_ROW;
    L.words = (L.off_tail + 4 + 3) / 4 * 4;
    if (route_cap > 0) {   // (words is a multiple of 4 and so is the section: the bytes start 16-byte aligned)
        L.route_cap = route_cap;
        L.off_route = L.words;
        L.words += ROUTE_REC_HDR_WORDS + route_cap / 4;
    }
    return L;
}

constexpr int ARCHIVE_META_F64 = 4, ARCHIVE_META_I32 = 6;   // x, y, vx, vy | stored, level, frame, cell_x, cell_y, switch_activated
enum ArchiveStatus { ARCHIVE_DONE = 0, ARCHIVE_SKIPPED = 1, ARCHIVE_LEVEL_MISMATCH = 2, ARCHIVE_EMPTY = 3, ARCHIVE_RANGE = 4 };

// Entry i moves env envs[i] <-> record slots[i].  Identity mode, envs == slots == null (with count == n == n_slots): entry i is
// env i <-> record i, and an entry whose `mask` byte is 0 is skipped.
struct ArchiveArgs {
    ArchiveLayout lay;
    int n, n_slots, count;
    const int32_t *envs, *slots;   // [count] device lists; both null = identity mode
    const uint8_t *mask;           // [n] identity mode only; null = all
    int32_t *status;               // [count] or null
    uint32_t *rec;                 // [n_slots][lay.words]
    double *meta_f64;              // [n_slots][ARCHIVE_META_F64]; the two meta pointers null = no meta row is written (store), no
    int32_t *meta_i32;             // [n_slots][ARCHIVE_META_I32]  "slot empty" test is made (restore)
    // the live state
    double *f64;                   // [NF64][n]
    uint32_t *u32;                 // [NU32][n]
    uint32_t *ent;                 // [n_words_max][n]
    float *sc;                     // [n][48]
    double *zoo;                   // [n][zoo_words]; null = none
    int32_t *trunc;                // [n]; restore: null = the env keeps its limit
    uint32_t *draws;               // [n] level pool draw counts; restore: null = the env keeps its count
    const int32_t *env_level;      // [n]
    int32_t *level_out;            // restore: [n] receives the record's level, and no level-mismatch test is made; null = test
    const LevelHdr *hdr;           // [n_levels] (store: the exit switch's entity slot, for the meta row)
    uint32_t *reach_key;           // [n]; null = the reachability buffers do not exist (yet)
    float *reach_cache;            // [n][REACH_DIM + 1]
    uint32_t *reach_last_episode;  // [n]; null = no level of the set takes the miss branch
    int32_t *route_hdr;            // [n][ROUTE_HDR_WORDS]; with lay.route_cap only
    uint8_t *route_act;            // [n][2][lay.route_cap]
};
hipError_t launch_archive_store(const ArchiveArgs &a, hipStream_t s);
hipError_t launch_archive_restore(const ArchiveArgs &a, hipStream_t s);

}  // namespace npp
