// npp_graph.hip -- graph observation rows (include/npp_amd.h: npp_graph_observation; tables: npp_graph.hpp).
//
// The graph is a constant of the level, so a row is only ever rewritten when its env plays another level than the one the row
// holds (row_level; -1 = nothing).  One launch of a fixed grid walks the envs (env e -> workgroup e mod grid): in the steady state
// every workgroup reads two ints per env and returns, and a changed env's four rows -- 162 500 bytes -- are written whole, padding
// included, by one workgroup of 512 lanes with 16-byte stores (the node-mask row, 2 500 bytes, is not a 16-byte multiple: its
// ends are written bytewise).  The compact per-level tables are read from the blob, zero padded to 16 bytes, so the partial word
// at the end of a table is also the start of the row's zero tail.  Each lane loads its words of the feature row, then of the edge
// rows, before it stores them: a first cut that copied word by word (load -> store loop) waited one memory latency per word, 35
// per env.
#include <hip/hip_runtime.h>

#include "npp_graph.hpp"
#include "npp_internal.hpp"

namespace npp {
namespace {

constexpr int BLOCK = 512;
constexpr int MAX_GRID = 1024;   // four workgroups per CU: a full rewrite keeps enough stores in flight, an idle call stays short
constexpr int FEAT_Q = GRAPH_FEAT_ROW / 16, EDGE_Q = GRAPH_EDGE_ROW / 32;       // 16-byte words of a feature row / an edge-index half
static_assert((FEAT_Q + BLOCK - 1) / BLOCK == 8 && (EDGE_Q + BLOCK - 1) / BLOCK == 5, "words per lane: 8 and 5 (named below)");

// bytes k0 .. k0 + 3 of a mask row: 1 where k < n
__device__ inline uint32_t mask_word(int k0, int n) {
    const int c = n - k0;
    return c <= 0 ? 0u : (c >= 4 ? 0x01010101u : (0x01010101u & ((1u << (8 * c)) - 1u)));
}
__device__ inline uint4 mask_quad(int k0, int n) { return make_uint4(mask_word(k0, n), mask_word(k0 + 4, n), mask_word(k0 + 8, n), mask_word(k0 + 12, n)); }

// word q of a table of `lim` words, zero past its end (a value, not a conditional lvalue: `c ? p[q] : z` selects between two
// addresses and put z in scratch memory)
__device__ inline uint4 table_word(const uint4 *p, int q, int lim) {
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (q < lim) v = p[q];
    return v;
}

__global__ __launch_bounds__(BLOCK) void npp_graph_kernel(GraphArgs a) {
    const int t = threadIdx.x;
    for (int e = blockIdx.x; e < a.n; e += gridDim.x) {
        const int lvl = a.env_level[e];
        if (lvl < 0 || lvl >= a.n_levels || (!a.all && a.row_level[e] == lvl)) continue;   // (uniform in the workgroup)
        const GraphHdr *h = a.hdr + lvl;
        const int nn = (int)h->n_nodes, ne = (int)h->n_edges;
        // the table words of a lane are loaded before its stores: two memory latencies per changed env, not one per word
        const uint4 *fs = reinterpret_cast<const uint4 *>(a.blob + h->off_feats), *ss = reinterpret_cast<const uint4 *>(a.blob + h->off_src),
                    *ds = reinterpret_cast<const uint4 *>(a.blob + h->off_dst);
        const int fq = (nn * GRAPH_FEAT * 4 + 15) / 16, eq = (ne * 2 + 15) / 16;
        // (named registers: a kernel with scratch memory pays for it at every dispatch)
#define NPP_LD(v, src, k, lim) const uint4 v = table_word(src, t + (k) * BLOCK, lim)
#define NPP_ST(dst, k, lim, v) if (t + (k) * BLOCK < (lim)) (dst)[t + (k) * BLOCK] = v
        uint4 *fr = reinterpret_cast<uint4 *>(a.feats + (size_t)e * GRAPH_NODES * GRAPH_FEAT);
        uint4 *er = reinterpret_cast<uint4 *>(a.edges + (size_t)e * 2 * GRAPH_EDGES);
        {   // features: 8 words per lane
            NPP_LD(f0, fs, 0, fq); NPP_LD(f1, fs, 1, fq); NPP_LD(f2, fs, 2, fq); NPP_LD(f3, fs, 3, fq);
            NPP_LD(f4, fs, 4, fq); NPP_LD(f5, fs, 5, fq); NPP_LD(f6, fs, 6, fq); NPP_LD(f7, fs, 7, fq);
            NPP_ST(fr, 0, FEAT_Q, f0); NPP_ST(fr, 1, FEAT_Q, f1); NPP_ST(fr, 2, FEAT_Q, f2); NPP_ST(fr, 3, FEAT_Q, f3);
            NPP_ST(fr, 4, FEAT_Q, f4); NPP_ST(fr, 5, FEAT_Q, f5); NPP_ST(fr, 6, FEAT_Q, f6); NPP_ST(fr, 7, FEAT_Q, f7);
        }
        {   // edge index: 5 words of each half per lane
            NPP_LD(s0, ss, 0, eq); NPP_LD(s1, ss, 1, eq); NPP_LD(s2, ss, 2, eq); NPP_LD(s3, ss, 3, eq); NPP_LD(s4, ss, 4, eq);
            NPP_LD(d0, ds, 0, eq); NPP_LD(d1, ds, 1, eq); NPP_LD(d2, ds, 2, eq); NPP_LD(d3, ds, 3, eq); NPP_LD(d4, ds, 4, eq);
            NPP_ST(er, 0, EDGE_Q, s0); NPP_ST(er, 1, EDGE_Q, s1); NPP_ST(er, 2, EDGE_Q, s2); NPP_ST(er, 3, EDGE_Q, s3); NPP_ST(er, 4, EDGE_Q, s4);
            NPP_ST(er + EDGE_Q, 0, EDGE_Q, d0); NPP_ST(er + EDGE_Q, 1, EDGE_Q, d1); NPP_ST(er + EDGE_Q, 2, EDGE_Q, d2);
            NPP_ST(er + EDGE_Q, 3, EDGE_Q, d3); NPP_ST(er + EDGE_Q, 4, EDGE_Q, d4);
        }
#undef NPP_LD
#undef NPP_ST
        uint4 *em = reinterpret_cast<uint4 *>(a.edge_mask + (size_t)e * GRAPH_EMASK_ROW);
        for (int q = t; q < (int)GRAPH_EMASK_ROW / 16; q += BLOCK) em[q] = mask_quad(16 * q, ne);
        // node mask: bytes up to the first 16-byte boundary (lanes 0..15) and after the last (lanes 16..31), 16-byte words between
        uint8_t *nm = a.node_mask + (size_t)e * GRAPH_NMASK_ROW;
        const int head = (int)((16 - ((uintptr_t)nm & 15)) & 15);
        const int body = ((int)GRAPH_NMASK_ROW - head) / 16, tail = head + 16 * body;
        if (t < head) nm[t] = t < nn ? 1 : 0;
        else if (t >= 16 && t < 32 && tail + t - 16 < (int)GRAPH_NMASK_ROW) nm[tail + t - 16] = tail + t - 16 < nn ? 1 : 0;
        for (int q = t; q < body; q += BLOCK) reinterpret_cast<uint4 *>(nm + head)[q] = mask_quad(head + 16 * q, nn);
        __syncthreads();   // every lane has read row_level[e]
        if (t == 0) a.row_level[e] = lvl;
    }
}

}  // namespace

hipError_t launch_graph_rows(const GraphArgs &a, hipStream_t s) {
    const int grid = a.n < MAX_GRID ? a.n : MAX_GRID;
    hipLaunchKernelGGL(npp_graph_kernel, dim3(grid), dim3(BLOCK), 0, s, a);
    return hipGetLastError();
}

}  // namespace npp
