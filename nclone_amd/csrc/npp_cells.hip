// npp_cells.hip -- the cell index over the checkpoint archive (include/npp_amd.h, npp_archive_cells_create; the rule:
// npp_cells.hpp): Go-Explore's "best state per cell" and its count-weighted pick, decided on the device.
//   explore = propose (one thread per env: visit count -- not under CellArgs::no_count, the seeding of npp_archive_seed -- + a
//                      64-bit atomic max of (ordered score, 0xfffffffe - env) per key)
//           + assign  (ONE workgroup walks the envs in ascending order: the winners of new keys take consecutive slots)
//           + the archive's own store kernel over (env e -> slot_of_env[e]).
//   select  = cdf     (one workgroup per level: inclusive prefix sums of the integer weights)
//           + pick    (one thread per env: binary search of its level's prefix sums).
// Launch boundaries are the only ordering between the kernels.  No atomic's return value is used and every atomic is an integer
// add or max, so no result depends on the order in which lanes, wavefronts or workgroups arrive; slot numbers come from a ballot
// rank in env order, never from a counter.
#include <hip/hip_runtime.h>

#include "npp_archive.hpp"
#include "npp_cells.hpp"
#include "npp_internal.hpp"

namespace npp {
namespace {

constexpr int ASSIGN_THREADS = 1024, ASSIGN_WAVES = ASSIGN_THREADS / WAVE;
constexpr int CDF_THREADS = 256, CDF_WAVES = CDF_THREADS / WAVE;
constexpr int CDF_KEYS = (NPP_CELLS_PER_LEVEL + CDF_THREADS - 1) / CDF_THREADS;   // 9 consecutive keys per thread

__global__ __launch_bounds__(256) void npp_cells_propose_kernel(CellArgs a) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= a.n) return;
    int key = -1, st = ARCHIVE_SKIPPED;
    if (!a.mask || a.mask[e]) {
        st = CELL_NOT_ELIGIBLE;
        const size_t N = (size_t)a.n;
        const int level = a.env_level[e];
        const LevelHdr &H = a.hdr[level];
        const int sw_state = exit_switch_state(a.ent, N, e, H.obs_switch);
        const int k = cell_key_in_level(state_load(a.u32, N, e, S_STATE), sw_state, a.f64[F_X * N + e], a.f64[F_Y * N + e],
                                        H.obs_door >= 0, H.door_x, H.door_y);
        const uint32_t bits = __float_as_uint(a.score ? a.score[e] : -(float)state_load(a.u32, N, e, S_FRAME));
        if (k >= 0 && !cell_bits_nan(bits)) {
            key = level * NPP_CELLS_PER_LEVEL + k;
            st = CELL_LOST;
            if (!a.no_count)   // (npp_archive_seed adds cells, not visits)
                (void)__hip_atomic_fetch_add(&a.visits[key], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            const unsigned long long prop = ((unsigned long long)cell_ordered_bits(bits) << 32) | cell_proposal_word((uint32_t)e);
            (void)__hip_atomic_fetch_max(&a.best[key], prop, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    a.env_key[e] = key;
    if (a.status) a.status[e] = st;
}

// One workgroup.  Chunk c holds envs [1024 c, 1024 c + 1024); a key has exactly one winner (the env whose proposal word the
// propose kernel's max left in the low word), so every table entry is written by one thread only.
__global__ __launch_bounds__(ASSIGN_THREADS) void npp_cells_assign_kernel(CellArgs a) {
    __shared__ int wave_new[ASSIGN_WAVES];
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid >> 6;
    int base = a.n_used[0];   // (one workgroup: everybody reads it before the only write, behind the last barrier)
    for (int c = 0; c < a.n; c += ASSIGN_THREADS) {
        const int e = c + tid;
        const int key = e < a.n ? a.env_key[e] : -1;
        unsigned long long b = 0;
        bool winner = false;
        if (key >= 0) {
            b = a.best[key];
            winner = (uint32_t)b == cell_proposal_word((uint32_t)e);
        }
        int slot = winner ? a.cell_slot[key] : -1;
        const bool is_new = winner && slot < 0;
        const unsigned long long m = __ballot(is_new);
        if (lane == 0) wave_new[wave] = __popcll(m);
        __syncthreads();
        int before = 0, total = 0;
        for (int w = 0; w < ASSIGN_WAVES; w++) {
            const int v = wave_new[w];
            before += w < wave ? v : 0;
            total += v;
        }
        __syncthreads();   // wave_new is rewritten by the next chunk
        if (is_new) {
            slot = base + before + __popcll(m & ((1ull << lane) - 1ull));
            if (slot < a.n_slots) {
                a.cell_slot[key] = slot;
                a.slot_key[slot] = key;
            } else {   // archive full: the key stays empty, only its visit count remains
                slot = -1;
                a.best[key] = 0ull;
                if (a.status) a.status[e] = CELL_FULL;
            }
        }
        if (slot >= 0) {   // the winner of a new or a better cell
            a.best[key] = b | 0xffffffffull;
            a.cell_score[key] = __uint_as_float(cell_float_bits((uint32_t)(b >> 32)));
            if (a.status) a.status[e] = ARCHIVE_DONE;
        }
        if (e < a.n) a.slot_of_env[e] = slot;
        base += total;
    }
    if (tid == 0) a.n_used[0] = base < a.n_slots ? base : a.n_slots;
}

__global__ __launch_bounds__(CDF_THREADS) void npp_cells_cdf_kernel(CellArgs a) {
    __shared__ unsigned long long wave_sum[CDF_WAVES];
    const int tid = threadIdx.x, lane = tid & (WAVE - 1), wave = tid >> 6;
    const size_t base = (size_t)blockIdx.x * NPP_CELLS_PER_LEVEL;
    const int k0 = tid * CDF_KEYS;
    uint32_t w[CDF_KEYS];
    unsigned long long local = 0;
#pragma unroll
    for (int j = 0; j < CDF_KEYS; j++) {
        const int k = k0 + j;
        w[j] = 0;
        if (k < NPP_CELLS_PER_LEVEL && a.cell_slot[base + k] >= 0) w[j] = cell_weight(a.visits[base + k], a.chosen[base + k]);
        local += w[j];
    }
    unsigned long long incl = local;   // inclusive scan over the wavefront (integer sums: exact in any association)
#pragma unroll
    for (int d = 1; d < WAVE; d <<= 1) {
        const unsigned long long up = __shfl_up(incl, d);
        if (lane >= d) incl += up;
    }
    if (lane == WAVE - 1) wave_sum[wave] = incl;
    __syncthreads();
    unsigned long long run = incl - local;
    for (int v = 0; v < wave; v++) run += wave_sum[v];
#pragma unroll
    for (int j = 0; j < CDF_KEYS; j++) {
        const int k = k0 + j;
        run += w[j];
        if (k < NPP_CELLS_PER_LEVEL) a.cdf[base + k] = run;
    }
}

__global__ __launch_bounds__(256) void npp_cells_pick_kernel(CellArgs a) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= a.n) return;
    int slot = -1;
    if (!a.mask || a.mask[e]) {
        const size_t base = (size_t)a.env_level[e] * NPP_CELLS_PER_LEVEL;
        const uint64_t *cdf = reinterpret_cast<const uint64_t *>(a.cdf + base);
        if (cdf[NPP_CELLS_PER_LEVEL - 1] != 0) {
            const int k = cell_pick(cdf, a.seed, (uint32_t)e, a.call);
            slot = a.cell_slot[base + k];
            (void)__hip_atomic_fetch_add(&a.chosen[base + k], 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    }
    a.slots_out[e] = slot;
}

}  // namespace

hipError_t launch_cells_propose(const CellArgs &a, hipStream_t s) {
    hipLaunchKernelGGL(npp_cells_propose_kernel, dim3((a.n + 255) / 256), dim3(256), 0, s, a);
    return hipGetLastError();
}
hipError_t launch_cells_assign(const CellArgs &a, hipStream_t s) {
    hipLaunchKernelGGL(npp_cells_assign_kernel, dim3(1), dim3(ASSIGN_THREADS), 0, s, a);
    return hipGetLastError();
}
hipError_t launch_cells_cdf(const CellArgs &a, hipStream_t s) {
    hipLaunchKernelGGL(npp_cells_cdf_kernel, dim3(a.n_levels), dim3(CDF_THREADS), 0, s, a);
    return hipGetLastError();
}
hipError_t launch_cells_pick(const CellArgs &a, hipStream_t s) {
    hipLaunchKernelGGL(npp_cells_pick_kernel, dim3((a.n + 255) / 256), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace npp
