// npp_tilequery.hpp -- the tile queries of the step kernel, device side.  Included by npp_kernels.hip (it uses that
// file's Lv / TileRefs, the scalar helpers and the time-of-intersection primitives).
//
// A body (the ninja, radius 10; a death ball of the zoo kernels, radius 8) asks three questions about the tile
// segments around it:
//   sweep          sweep_circle_vs_tiles (physics.py:104-128): the earliest time of impact along a displacement
//   closest point  get_single_closest_point (physics.py:131-180): the nearest segment point, first wins on ties
//   wall probe     the tile terms of Ninja.post_collision (ninja.py:424-441), summed in query order
// Each is answered in two forms that give the same bits:
//   register form  from the per-tick candidate registers (Cand<K>, cand_gather): tile_sweep, cand_closest_query and
//                  the fast loops of collide_vs_tiles / post_collision
//   table form     a walk over the level's CSR table in LDS or L2 (region_walk), taken when a query leaves the
//                  gathered cells or they hold more than G * K segments: sweep_generic, region_closest
//                  (closest_generic, depen_generic), wall_probe_generic -- out of line, TileRefs by value
// Both forms share one decode of the packed 16-bit segment (seg_decode; besides it only npp_level.cpp, which packs
// the tables, knows the bit layout of the end points) and one geometry on the decoded values (cand_toi,
// cand_closest_lin, cand_closest_arc, seg_box), so a rule about a segment is written once.
#pragma once

// ---- cooperative groups of G lanes per environment -------------------------------------------------------------
// All G lanes of a group hold the same ninja state and execute the same scalar code redundantly; they split up only
// the per-segment work of a region query (lane r takes segments r, r+G, ... of the query's flat order) and combine
// with DPP butterflies.  Order-dependent semantics of the reference are preserved exactly: minima are
// order-independent, "first wins" ties (physics.py:176 strict <) are broken by the flat query index, and the wall
// probe's sum (ninja.py:441) is accumulated in query order.
// The butterfly partner always lies in the same lane group, whose lanes execute together, so it is always active:
// bound_ctrl lets the compiler fold the move into the consuming instruction instead of keeping a copy for `old`.
template <int CTRL> DEV int dpp_i(int v) { return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xf, 0xf, true); }
template <int CTRL> DEV double dpp_d(double v) {
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = dpp_i<CTRL>(lo);
    hi = dpp_i<CTRL>(hi);
    return __hiloint2double(hi, lo);
}
// value held by the butterfly partner at distance STEP (1,2: quad_perm; 4: row_half_mirror; 8: row_mirror)
template <int STEP> DEV int partner_i(int v) {
    if constexpr (STEP == 1) return dpp_i<0xB1>(v);
    else if constexpr (STEP == 2) return dpp_i<0x4E>(v);
    else if constexpr (STEP == 4) return dpp_i<0x141>(v);
    else if constexpr (STEP == 8) return dpp_i<0x140>(v);
    else return __shfl_xor(v, STEP, 64);
}
template <int STEP> DEV double partner_d(double v) {
    if constexpr (STEP == 1) return dpp_d<0xB1>(v);
    else if constexpr (STEP == 2) return dpp_d<0x4E>(v);
    else if constexpr (STEP == 4) return dpp_d<0x141>(v);
    else if constexpr (STEP == 8) return dpp_d<0x140>(v);
    else return __shfl_xor(v, STEP, 64);
}

// v_min_f64 without the canonicalising v_max_f64 x, x, x that llvm.minnum puts in front of every operand it cannot prove
// quiet (anything that went through a select or a DPP move): the operands here are never NaN (+inf / 1 mark "none"), and each
// such instruction is ~7 cycles of the single wavefront's issue cadence inside the depenetration loop (five per iteration).
DEV double min_nonan(double a, double b) {
    double r;
    asm("v_min_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
template <int G, int STEP = 1> DEV double group_min(double t) {
    if constexpr (STEP < G) {
        t = min_nonan(t, partner_d<STEP>(t));
        return group_min<G, STEP * 2>(t);
    } else {
        return t;
    }
}

struct Best {
    double key;   // biased squared distance (physics.py:171-176)
    int idx;      // flat query index << 8 | evaluating lane's rank in its group << 1 | is_back_facing
    double a, b;  // closest point
};

template <int G, int STEP = 1> DEV int group_min_i(int v) {
    if constexpr (STEP < G) {
        int o = partner_i<STEP>(v);
        v = o < v ? o : v;
        return group_min_i<G, STEP * 2>(v);
    } else {
        return v;
    }
}

// Group-wide "first wins" argmin (physics.py:176 strict <): smallest key, ties broken by the smallest flat query
// index.  Two cheap butterflies (key, then index among the lanes holding the minimum key) and one cross-lane fetch
// of the winner's closest point; every lane of the group ends up with the same m.
template <int G> DEV void group_argmin(Best &m) {
    if constexpr (G > 1) {
        const double kmin = group_min<G>(m.key);
        const int cand = (m.idx != 0x7fffffff && m.key == kmin) ? m.idx : 0x7fffffff;
        const int imin = group_min_i<G>(cand);
        const int src = (((threadIdx.x & 63) & ~(G - 1)) + ((imin >> 1) & 63)) << 2;   // winner lane, byte address
        int alo = __builtin_amdgcn_ds_bpermute(src, __double2loint(m.a)), ahi = __builtin_amdgcn_ds_bpermute(src, __double2hiint(m.a));
        int blo = __builtin_amdgcn_ds_bpermute(src, __double2loint(m.b)), bhi = __builtin_amdgcn_ds_bpermute(src, __double2hiint(m.b));
        m.key = kmin;
        m.idx = imin;
        m.a = __hiloint2double(ahi, alo);
        m.b = __hiloint2double(bhi, blo);
    }
}

// the wavefront ballot of the calling lane's group: bit k belongs to the group's lane of rank k
template <int G> DEV unsigned long long group_ballot(bool v) {
    unsigned long long bal = __ballot(v) >> ((threadIdx.x & 63) & ~(G - 1));
    if constexpr (G < 64) bal &= (1ull << G) - 1;
    return bal;
}
template <int G> DEV bool group_any(bool v) {
    if constexpr (G == 1) return v;
    else return group_ballot<G>(v) != 0;
}

// sum the wall-probe terms of one pass in lane (= query) order (ninja.py:441)
template <int G> DEV void ordered_add(double &acc, double term) {
    if constexpr (G == 1) {
        acc += term;
    } else {
        const int glane0 = (threadIdx.x & 63) & ~(G - 1);
        unsigned long long bal = group_ballot<G>(term != 0);
        while (bal) {
            int k = __builtin_ctzll(bal);
            bal &= bal - 1;
            acc += __shfl(term, glane0 + k, 64);
        }
    }
}

// ---- one segment geometry ----------------------------------------------------------------------------------------
// A packed segment of cell (xc, yc), decoded.  Linear: (x1, y1), (x2, y2) are the end points; arc: (x1, y1) is the
// centre, x2 = p_hor.x and y2 = p_ver.y (entities.py:113-114).  u* are the same four values in units of 12 px (exact:
// every tile coordinate is a multiple of 12), the integers behind the segment's AABB.  Bits of s that survive the
// decode: 0 arc, and for an arc 6 hor > 0, 7 ver > 0, 8 convex.
struct Seg {
    uint32_t s;
    double x1, y1, x2, y2;
    int ux1, uy1, ux2, uy2;
};
DEV Seg seg_decode(uint32_t s, int xc, int yc) {
    Seg g;
    g.s = s;
    g.ux1 = 2 * xc + (int)((s >> 2) & 3); g.uy1 = 2 * yc + (int)((s >> 4) & 3);
    if ((s & 1u) == 0) { g.ux2 = 2 * xc + (int)((s >> 6) & 3); g.uy2 = 2 * yc + (int)((s >> 8) & 3); }
    else { g.ux2 = g.ux1 + (((s >> 6) & 1) ? 2 : -2); g.uy2 = g.uy1 + (((s >> 7) & 1) ? 2 : -2); }
    g.x1 = 12.0 * g.ux1; g.y1 = 12.0 * g.uy1; g.x2 = 12.0 * g.ux2; g.y2 = 12.0 * g.uy2;
    return g;
}
// |w|^2 / 144 of a linear segment: 1 (axis aligned), 8 (45 degrees) or 5 (the 1:2 slopes) for every shape the tile tables produce
DEV int seg_aw(const Seg &g) { return (g.ux2 - g.ux1) * (g.ux2 - g.ux1) + (g.uy2 - g.uy1) * (g.uy2 - g.uy1); }

// the segment's AABB (entities.py:36-41,119-125): min / max of (x1, x2) and of (y1, y2), for arcs too
DEV void seg_box(double x1, double y1, double x2, double y2, double &bx0, double &by0, double &bx1, double &by1) {
    bx0 = __builtin_fmin(x1, x2); bx1 = __builtin_fmax(x1, x2);
    by0 = __builtin_fmin(y1, y2); by1 = __builtin_fmax(y1, y2);
}

// GridSegment*.intersect_with_ray on a decoded segment (entities.py:82-96,180-203)
DEV double cand_toi(uint32_t s, double x1, double y1, double x2, double y2, double px, double py, double dx, double dy,
                    double vel_sq, double radius) {
    double t1, t2, t3;
    if ((s & 1u) == 0) {
        int wxu = (int)((s >> 6) & 3) - (int)((s >> 2) & 3), wyu = (int)((s >> 8) & 3) - (int)((s >> 4) & 3);
        t1 = toi_circle_point(px, py, dx, dy, vel_sq, x1, y1, radius);
        t2 = toi_circle_point(px, py, dx, dy, vel_sq, x2, y2, radius);
        t3 = toi_circle_lineseg(px, py, dx, dy, x1, y1, wxu, wyu, radius);
    } else {
        double hor = ((s >> 6) & 1) ? 1.0 : -1.0, ver = ((s >> 7) & 1) ? 1.0 : -1.0;
        t1 = toi_circle_point(px, py, dx, dy, vel_sq, x2, y1, radius);
        t2 = toi_circle_point(px, py, dx, dy, vel_sq, x1, y2, radius);
        t3 = toi_circle_arc(px, py, dx, dy, vel_sq, x1, y1, hor, ver, radius);
    }
    double t = t1;
    if (t2 < t) t = t2;
    if (t3 < t) t = t3;
    return t;
}

// GridSegmentCircular.get_closest_point on a decoded segment (entities.py:127-157); returns is_back_facing
DEV bool cand_closest_arc(uint32_t s, double x1, double y1, double x2, double y2, double px, double py,
                                              double &a, double &b) {
    double hor = ((s >> 6) & 1) ? 1.0 : -1.0, ver = ((s >> 7) & 1) ? 1.0 : -1.0;
    bool convex = (s >> 8) & 1;
    double dx = px - x1, dy = py - y1;
    bool back = false;
    if (dx * hor > 0 && dy * ver > 0) {
        double dist = dsqrt(sq(dx) + sq(dy));
        if (dist == 0) {
            if (dx * hor > dy * ver) { a = x2; b = y1; }
            else { a = x1; b = y2; }
            return false;
        }
        a = x1 + 24.0 * dx / dist;
        b = y1 + 24.0 * dy / dist;
        back = convex ? (dist < 24.0) : (dist > 24.0);
    } else {
        if (dx * hor > dy * ver) { a = x2; b = y1; }
        else { a = x1; b = y2; }
    }
    return back;
}

// GridSegmentLinear.get_closest_point (entities.py:43-59) on a decoded segment with vector (wx, wy), l2 = |w|^2 in
// {144, 720, 1152} and rl2 = RN(1 / l2), branch-free; returns is_back_facing (tile segments are always oriented).
// max/min are the hardware ones: they differ from Python's max(u, 0) / min(u, 1) only in the sign of a zero u, which
// cannot reach a or b (x1 + (+-0) * w == x1).
DEV bool cand_closest_lin(double x1, double y1, double wx, double wy, double l2, double rl2, double px, double py,
                          double &a, double &b) {
    double dx = px - x1, dy = py - y1;
    double num = dx * wx + dy * wy;
    double u = div_const(num, l2, rl2);
    u = __builtin_fmax(u, 0.0);
    u = __builtin_fmin(u, 1.0);
    a = x1 + u * wx;
    b = y1 + u * wy;
    return dy * wx - dx * wy < 0;
}

// get_closest_point of a segment decoded from the table
DEV bool seg_closest(const Seg &g, double px, double py, double &a, double &b) {
    if (g.s & 1u) return cand_closest_arc(g.s, g.x1, g.y1, g.x2, g.y2, px, py, a, b);
    const double wx = g.x2 - g.x1, wy = g.y2 - g.y1;
    switch (seg_aw(g)) {   // |w|^2 and its reciprocal as literals: as selected values they cost the callers' kernels scratch
    case 1: return cand_closest_lin(g.x1, g.y1, wx, wy, 144.0, 1.0 / 144.0, px, py, a, b);
    case 8: return cand_closest_lin(g.x1, g.y1, wx, wy, 1152.0, 1.0 / 1152.0, px, py, a, b);
    case 5: return cand_closest_lin(g.x1, g.y1, wx, wy, 720.0, 1.0 / 720.0, px, py, a, b);
    }
    // a shape the tile tables never produce (cand_gather vetoes the register form for it): the reference's own division
    const double dx = px - g.x1, dy = py - g.y1, u = pymin(pymax((dx * wx + dy * wy) / (sq(wx) + sq(wy)), 0.0), 1.0);
    a = g.x1 + u * wx; b = g.y1 + u * wy;
    return dy * wx - dx * wy < 0;
}

// SpatialSegmentIndex.query_region cell filter (utils/spatial_segment_index.py:140-156, inclusive test :186-188)
DEV bool cell_passes(uint32_t cb, int xc, int yc, double qx0, double qy0, double qx1, double qy1) {
    double bx0 = 24.0 * xc + 12.0 * (cb & 3), by0 = 24.0 * yc + 12.0 * ((cb >> 2) & 3);
    double bx1 = 24.0 * xc + 12.0 * ((cb >> 4) & 3), by1 = 24.0 * yc + 12.0 * ((cb >> 6) & 3);
    return !(qx1 < bx0 || qx0 > bx1 || qy1 < by0 || qy0 > by1);
}

// ---- per-tick candidate registers (register form) ----------------------------------------------------------------
// Once per tick every lane group gathers ALL segments of the cells around the ninja's path (old position -> new
// position, inflated by the largest query radius) and keeps them decoded in registers: lane r holds candidates
// r, r + G, ... of the region's x-major order (K slots per lane).  A region query of the reference (sweep box,
// depenetration gather box, wall-probe box) whose clamped cell range lies inside the gathered range is then
// answered from registers by applying the reference's own filters per candidate (cell range, inclusive cell-bounds
// test, per-segment AABB test) -- the surviving candidates in flat order are exactly the reference's list.  A query
// that leaves the region (or a region with more segments than lanes x slots) takes the table form below.
// All filters are evaluated in doubles on exact quantities (multiples of 12 px), so no integer cell arithmetic is
// needed on the fast path.

DEV double clampd(double v, double lo, double hi) { return v < lo ? lo : (v > hi ? hi : v); }

// A query box plus copies clamped to the map: clamp(floor(q / 24), 0, 43) == floor(clamp(q, 0, 1032) / 24) and
// likewise with 576 for y (utils/spatial_segment_index.py:131-134), so "cell xc is inside the query's clamped cell
// range" is 24 xc <= clamp(qx1) && 24 (xc + 1) > clamp(qx0).
struct QBox {
    double x0, y0, x1, y1;
    double cx0, cy0, cx1, cy1;
};
DEV QBox make_qbox(double x0, double y0, double x1, double y1) {
    QBox q;
    q.x0 = x0; q.y0 = y0; q.x1 = x1; q.y1 = y1;
    q.cx0 = clampd(x0, 0.0, 1032.0); q.cx1 = clampd(x1, 0.0, 1032.0);
    q.cy0 = clampd(y0, 0.0, 576.0); q.cy1 = clampd(y1, 0.0, 576.0);
    return q;
}

// The per-segment AABB test of get_single_closest_point (physics.py:150-167) against the ninja's box [x - 10, x + 10] x [y - 10, y + 10],
// as exact thresholds on x and y: segment bounds are multiples of 12 in [0, 1056], the reference rounds x - 10 and x + 10 before it
// compares, and rounding is monotone, so "not (b1 < fl(x - 10))" is "x <= b1 + 10" (b1 + 10 is exact and its ulp is at least b1's) and
// "not (b0 > fl(x + 10))" is "x >= AABB_LO[b0 / 12]", the smallest double whose rounded sum reaches b0 (it lies below b0 - 10 where b0 - 10
// sits in a lower binade than b0: 8 of the 89 entries).  Generated and checked against the rounded sums on 40 doubles either side of every
// threshold (tests/test_host_cpu.py repeats the check on the table below); saves the four fp64 additions per candidate and iteration.
__constant__ double AABB_LO[89] = {
    -0x1.4000000000000p+3 /* 0: fl(x + 10) >= 0 */,
    0x1.ffffffffffffcp+0 /* 1: fl(x + 10) >= 12 */,
    0x1.bffffffffffffp+3 /* 2: fl(x + 10) >= 24 */,
    0x1.9ffffffffffffp+4 /* 3: fl(x + 10) >= 36 */,
    0x1.3000000000000p+5 /* 4: fl(x + 10) >= 48 */,
    0x1.9000000000000p+5 /* 5: fl(x + 10) >= 60 */,
    0x1.effffffffffffp+5 /* 6: fl(x + 10) >= 72 */,
    0x1.2800000000000p+6 /* 7: fl(x + 10) >= 84 */,
    0x1.5800000000000p+6 /* 8: fl(x + 10) >= 96 */,
    0x1.8800000000000p+6 /* 9: fl(x + 10) >= 108 */,
    0x1.b800000000000p+6 /* 10: fl(x + 10) >= 120 */,
    0x1.e7fffffffffffp+6 /* 11: fl(x + 10) >= 132 */,
    0x1.0c00000000000p+7 /* 12: fl(x + 10) >= 144 */,
    0x1.2400000000000p+7 /* 13: fl(x + 10) >= 156 */,
    0x1.3c00000000000p+7 /* 14: fl(x + 10) >= 168 */,
    0x1.5400000000000p+7 /* 15: fl(x + 10) >= 180 */,
    0x1.6c00000000000p+7 /* 16: fl(x + 10) >= 192 */,
    0x1.8400000000000p+7 /* 17: fl(x + 10) >= 204 */,
    0x1.9c00000000000p+7 /* 18: fl(x + 10) >= 216 */,
    0x1.b400000000000p+7 /* 19: fl(x + 10) >= 228 */,
    0x1.cc00000000000p+7 /* 20: fl(x + 10) >= 240 */,
    0x1.e400000000000p+7 /* 21: fl(x + 10) >= 252 */,
    0x1.fbfffffffffffp+7 /* 22: fl(x + 10) >= 264 */,
    0x1.0a00000000000p+8 /* 23: fl(x + 10) >= 276 */,
    0x1.1600000000000p+8 /* 24: fl(x + 10) >= 288 */,
    0x1.2200000000000p+8 /* 25: fl(x + 10) >= 300 */,
    0x1.2e00000000000p+8 /* 26: fl(x + 10) >= 312 */,
    0x1.3a00000000000p+8 /* 27: fl(x + 10) >= 324 */,
    0x1.4600000000000p+8 /* 28: fl(x + 10) >= 336 */,
    0x1.5200000000000p+8 /* 29: fl(x + 10) >= 348 */,
    0x1.5e00000000000p+8 /* 30: fl(x + 10) >= 360 */,
    0x1.6a00000000000p+8 /* 31: fl(x + 10) >= 372 */,
    0x1.7600000000000p+8 /* 32: fl(x + 10) >= 384 */,
    0x1.8200000000000p+8 /* 33: fl(x + 10) >= 396 */,
    0x1.8e00000000000p+8 /* 34: fl(x + 10) >= 408 */,
    0x1.9a00000000000p+8 /* 35: fl(x + 10) >= 420 */,
    0x1.a600000000000p+8 /* 36: fl(x + 10) >= 432 */,
    0x1.b200000000000p+8 /* 37: fl(x + 10) >= 444 */,
    0x1.be00000000000p+8 /* 38: fl(x + 10) >= 456 */,
    0x1.ca00000000000p+8 /* 39: fl(x + 10) >= 468 */,
    0x1.d600000000000p+8 /* 40: fl(x + 10) >= 480 */,
    0x1.e200000000000p+8 /* 41: fl(x + 10) >= 492 */,
    0x1.ee00000000000p+8 /* 42: fl(x + 10) >= 504 */,
    0x1.f9fffffffffffp+8 /* 43: fl(x + 10) >= 516 */,
    0x1.0300000000000p+9 /* 44: fl(x + 10) >= 528 */,
    0x1.0900000000000p+9 /* 45: fl(x + 10) >= 540 */,
    0x1.0f00000000000p+9 /* 46: fl(x + 10) >= 552 */,
    0x1.1500000000000p+9 /* 47: fl(x + 10) >= 564 */,
    0x1.1b00000000000p+9 /* 48: fl(x + 10) >= 576 */,
    0x1.2100000000000p+9 /* 49: fl(x + 10) >= 588 */,
    0x1.2700000000000p+9 /* 50: fl(x + 10) >= 600 */,
    0x1.2d00000000000p+9 /* 51: fl(x + 10) >= 612 */,
    0x1.3300000000000p+9 /* 52: fl(x + 10) >= 624 */,
    0x1.3900000000000p+9 /* 53: fl(x + 10) >= 636 */,
    0x1.3f00000000000p+9 /* 54: fl(x + 10) >= 648 */,
    0x1.4500000000000p+9 /* 55: fl(x + 10) >= 660 */,
    0x1.4b00000000000p+9 /* 56: fl(x + 10) >= 672 */,
    0x1.5100000000000p+9 /* 57: fl(x + 10) >= 684 */,
    0x1.5700000000000p+9 /* 58: fl(x + 10) >= 696 */,
    0x1.5d00000000000p+9 /* 59: fl(x + 10) >= 708 */,
    0x1.6300000000000p+9 /* 60: fl(x + 10) >= 720 */,
    0x1.6900000000000p+9 /* 61: fl(x + 10) >= 732 */,
    0x1.6f00000000000p+9 /* 62: fl(x + 10) >= 744 */,
    0x1.7500000000000p+9 /* 63: fl(x + 10) >= 756 */,
    0x1.7b00000000000p+9 /* 64: fl(x + 10) >= 768 */,
    0x1.8100000000000p+9 /* 65: fl(x + 10) >= 780 */,
    0x1.8700000000000p+9 /* 66: fl(x + 10) >= 792 */,
    0x1.8d00000000000p+9 /* 67: fl(x + 10) >= 804 */,
    0x1.9300000000000p+9 /* 68: fl(x + 10) >= 816 */,
    0x1.9900000000000p+9 /* 69: fl(x + 10) >= 828 */,
    0x1.9f00000000000p+9 /* 70: fl(x + 10) >= 840 */,
    0x1.a500000000000p+9 /* 71: fl(x + 10) >= 852 */,
    0x1.ab00000000000p+9 /* 72: fl(x + 10) >= 864 */,
    0x1.b100000000000p+9 /* 73: fl(x + 10) >= 876 */,
    0x1.b700000000000p+9 /* 74: fl(x + 10) >= 888 */,
    0x1.bd00000000000p+9 /* 75: fl(x + 10) >= 900 */,
    0x1.c300000000000p+9 /* 76: fl(x + 10) >= 912 */,
    0x1.c900000000000p+9 /* 77: fl(x + 10) >= 924 */,
    0x1.cf00000000000p+9 /* 78: fl(x + 10) >= 936 */,
    0x1.d500000000000p+9 /* 79: fl(x + 10) >= 948 */,
    0x1.db00000000000p+9 /* 80: fl(x + 10) >= 960 */,
    0x1.e100000000000p+9 /* 81: fl(x + 10) >= 972 */,
    0x1.e700000000000p+9 /* 82: fl(x + 10) >= 984 */,
    0x1.ed00000000000p+9 /* 83: fl(x + 10) >= 996 */,
    0x1.f300000000000p+9 /* 84: fl(x + 10) >= 1008 */,
    0x1.f900000000000p+9 /* 85: fl(x + 10) >= 1020 */,
    0x1.fefffffffffffp+9 /* 86: fl(x + 10) >= 1032 */,
    0x1.0280000000000p+10 /* 87: fl(x + 10) >= 1044 */,
    0x1.0580000000000p+10 /* 88: fl(x + 10) >= 1056 */
};

template <int K> struct Cand {
    double rx0, ry0, rx1, ry1;   // gathered cell range in pixels: [24 c0, 24 (c1 + 1))
    bool ok;
    uint32_t s[K];               // packed segment (bits 0-15, incl. cell y) | cell x << 16 | valid << 31
    double x1[K], y1[K], x2[K], y2[K];       // linear: end points; arc: centre, p_hor.x, p_ver.y (Seg)
    double wx[K], wy[K], l2[K], rl2[K];      // linear: segment vector, |w|^2 and RN(1 / |w|^2)
    double ox[K], oy[K];                     // origin of the owning cell
    double bx0[K], by0[K], bx1[K], by1[K];   // the owning cell's bounds over its segments (:86-105)
    double tx0[K], tx1[K], ty0[K], ty1[K];   // the segment's AABB as thresholds on the ninja position (AABB_LO above): tx0 <= x <= tx1, ...
};

template <int G, int K>
DEV void cand_gather(const Lv &lv, int r, double qx0, double qy0, double qx1, double qy1, Cand<K> &c) {
    const int c0x = cell_coord(qx0, 43), c1x = cell_coord(qx1, 43), c0y = cell_coord(qy0, 24), c1y = cell_coord(qy1, 24);
    c.rx0 = 24.0 * c0x; c.rx1 = 24.0 * (c1x + 1); c.ry0 = 24.0 * c0y; c.ry1 = 24.0 * (c1y + 1);
    const int ncol = c1x - c0x + 1;
    int a0 = lv.seg_start[c0x * 25 + c0y], n0 = lv.seg_start[c0x * 25 + c1y + 1] - a0;
    int a1 = 0, n1 = 0, a2 = 0, n2 = 0;
    if (ncol > 1) { a1 = lv.seg_start[(c0x + 1) * 25 + c0y]; n1 = lv.seg_start[(c0x + 1) * 25 + c1y + 1] - a1; }
    if (ncol > 2) { a2 = lv.seg_start[(c0x + 2) * 25 + c0y]; n2 = lv.seg_start[(c0x + 2) * 25 + c1y + 1] - a2; }
    const int total = n0 + n1 + n2;
    c.ok = ncol <= 3 && total <= G * K;
#pragma unroll
    for (int k = 0; k < K; k++) {
        int f = k * G + r;
        c.s[k] = 0;
        c.x1[k] = 0; c.y1[k] = 0; c.x2[k] = 0; c.y2[k] = 0; c.wx[k] = 0; c.wy[k] = 0; c.l2[k] = 1; c.rl2[k] = 1;
        c.ox[k] = 0; c.oy[k] = 0; c.bx0[k] = 0; c.by0[k] = 0; c.bx1[k] = 0; c.by1[k] = 0;
        c.tx0[k] = 0; c.tx1[k] = 0; c.ty0[k] = 0; c.ty1[k] = 0;
        if (c.ok && f < total) {
            int xc = c0x, i = a0 + f;
            if (f >= n0) { xc += 1; i = a1 + (f - n0); }
            if (f >= n0 + n1) { xc += 1; i = a2 + (f - n0 - n1); }
            uint32_t s = lv.segs[i];
            int yc = s >> 11;
            uint32_t cb = lv.bounds[xc * 25 + yc];
            c.s[k] = s | ((uint32_t)xc << 16) | 0x80000000u;
            double ox = 24.0 * xc, oy = 24.0 * yc;
            c.ox[k] = ox; c.oy[k] = oy;
            c.bx0[k] = ox + 12.0 * (cb & 3); c.by0[k] = oy + 12.0 * ((cb >> 2) & 3);
            c.bx1[k] = ox + 12.0 * ((cb >> 4) & 3); c.by1[k] = oy + 12.0 * ((cb >> 6) & 3);
            const Seg g = seg_decode(s, xc, yc);
            c.x1[k] = g.x1; c.y1[k] = g.y1; c.x2[k] = g.x2; c.y2[k] = g.y2;
            if ((s & 1u) == 0) {
                const int aw = seg_aw(g);
                c.wx[k] = g.x2 - g.x1; c.wy[k] = g.y2 - g.y1;
                c.l2[k] = aw == 1 ? 144.0 : (aw == 8 ? 1152.0 : 720.0);
                c.rl2[k] = aw == 1 ? 1.0 / 144.0 : (aw == 8 ? 1.0 / 1152.0 : 1.0 / 720.0);
                if (!(aw == 1 || aw == 8 || aw == 5)) c.ok = false;   // never produced by the tile tables
            }
            // the segment's AABB in units of 12 px, as thresholds on the ninja position
            const int ulo = g.ux1 < g.ux2 ? g.ux1 : g.ux2, uhi = g.ux1 < g.ux2 ? g.ux2 : g.ux1;
            const int vlo = g.uy1 < g.uy2 ? g.uy1 : g.uy2, vhi = g.uy1 < g.uy2 ? g.uy2 : g.uy1;
            if (ulo < 0 || uhi > 88 || vlo < 0 || vhi > 88) c.ok = false;   // never produced by the tile tables
            c.tx0[k] = AABB_LO[ulo < 0 ? 0 : (ulo > 88 ? 88 : ulo)]; c.tx1[k] = 12.0 * uhi + 10.0;
            c.ty0[k] = AABB_LO[vlo < 0 ? 0 : (vlo > 88 ? 88 : vlo)]; c.ty1[k] = 12.0 * vhi + 10.0;
        }
    }
    if constexpr (G > 1) c.ok = group_ballot<G>(!c.ok) == 0;   // the "unexpected segment length" veto must be group-wide
}

template <int K> DEV bool cand_covers(const Cand<K> &c, const QBox &q) {
    return c.ok & (q.cx0 >= c.rx0) & (q.cx1 < c.rx1) & (q.cy0 >= c.ry0) & (q.cy1 < c.ry1);
}

// would the reference's query have returned candidate k?  (its cell inside the query's clamped cell range and the
// inclusive cell-bounds test of utils/spatial_segment_index.py:186-188)
template <int K> DEV bool cand_in_box(const Cand<K> &c, int k, const QBox &q) {
    bool in_range = (c.ox[k] <= q.cx1) & (c.ox[k] + 24.0 > q.cx0) & (c.oy[k] <= q.cy1) & (c.oy[k] + 24.0 > q.cy0);
    bool reject = (q.x1 < c.bx0[k]) | (q.x0 > c.bx1[k]) | (q.y1 < c.by0[k]) | (q.y0 > c.by1[k]);
    return (c.s[k] >> 31) & in_range & !reject;
}

template <int K> DEV bool cand_closest_lin(const Cand<K> &c, int k, double px, double py, double &a, double &b) {
    return cand_closest_lin(c.x1[k], c.y1[k], c.wx[k], c.wy[k], c.l2[k], c.rl2[k], px, py, a, b);
}
template <int K> DEV bool cand_closest(const Cand<K> &c, int k, double px, double py, double &a, double &b) {
    if ((c.s[k] & 1u) == 0) return cand_closest_lin(c, k, px, py, a, b);
    return cand_closest_arc(c.s[k], c.x1[k], c.y1[k], c.x2[k], c.y2[k], px, py, a, b);
}

// ---- table form: one walk over the segments of a query's cells ---------------------------------------------------
// The reference's query_region for the box (qx0, qy0)-(qx1, qy1): columns c0x..c1x of the clamped cell range, in each
// the CSR entries seg_start[xc * 25 + c0y] .. seg_start[xc * 25 + c1y + 1] (the column's cells are contiguous), of
// which lane r takes every G-th; an entry counts when its cell passes the inclusive cell-bounds test.  `body(valid,
// s, xc, yc, flat)` gets the packed segment, its cell and its flat query index (the tie-break of group_argmin).
// Two modes.  UNIFORM: every lane of a group makes the same number of trips and body runs in each of them -- valid is
// false for a filtered entry and past the column's end -- so that body may hold a group collective (ordered_add, and
// the ninja's depenetration search, whose kernels have less scratch this way).  Otherwise body runs for the counting
// entries only (valid is always true): the sweep and the zoo's closest_generic, which time as at the parent this way.
template <int G, bool UNIFORM, typename F>
DEV void region_walk(TileRefs lv, int r, double qx0, double qy0, double qx1, double qy1, F body) {
    const int c0x = cell_coord(qx0, 43), c1x = cell_coord(qx1, 43), c0y = cell_coord(qy0, 24), c1y = cell_coord(qy1, 24);
    int base = 0;
    for (int xc = c0x; xc <= c1x; xc++) {
        const int i0 = lv.seg_start[xc * 25 + c0y], i1 = lv.seg_start[xc * 25 + c1y + 1];
        if constexpr (UNIFORM) {
            for (int ib = i0; ib < i1; ib += G) {
                const int i = ib + r;
                uint32_t s = 0;
                bool valid = false;
                if (i < i1) {
                    s = lv.segs[i];
                    valid = cell_passes(lv.bounds[xc * 25 + (s >> 11)], xc, s >> 11, qx0, qy0, qx1, qy1);
                }
                body(valid, s, xc, (int)(s >> 11), base + i - i0);
            }
        } else {
            for (int i = i0 + r; i < i1; i += G) {
                const uint32_t s = lv.segs[i];
                const int yc = s >> 11;
                if (cell_passes(lv.bounds[xc * 25 + yc], xc, yc, qx0, qy0, qx1, qy1)) body(true, s, xc, yc, base + i - i0);
            }
        }
        base += i1 - i0;
    }
}

// ---- sweep: sweep_circle_vs_tiles (physics.py:104-128).  The early `return 0` of the reference equals the minimum.
template <int G>
__device__ __noinline__ double sweep_generic(TileRefs lv, int r, double xo, double yo, double dx, double dy, double radius) {
    const double xn = xo + dx, yn = yo + dy, width = radius + 1;
    const double vel_sq = sq(dx) + sq(dy);
    double shortest = 1;
    region_walk<G, false>(lv, r, (xo < xn ? xo : xn) - width, (yo < yn ? yo : yn) - width, (xo > xn ? xo : xn) + width, (yo > yn ? yo : yn) + width,
                   [&](bool valid, uint32_t s, int xc, int yc, int) {
        if (!valid) return;
        const Seg g = seg_decode(s, xc, yc);
        const double t = cand_toi(g.s, g.x1, g.y1, g.x2, g.y2, xo, yo, dx, dy, vel_sq, radius);
        if (t < shortest) shortest = t;
    });
    return group_min<G>(shortest);
}

// cover test, per-candidate box test, cand_toi, group_min; else the table form
template <int G, int K>
DEV double tile_sweep(const Lv &lv, int r, const Cand<K> &cd, double xo, double yo, double dx, double dy, double radius) {
    const double xn = xo + dx, yn = yo + dy, width = radius + 1;
    const QBox q = make_qbox((xo < xn ? xo : xn) - width, (yo < yn ? yo : yn) - width, (xo > xn ? xo : xn) + width, (yo > yn ? yo : yn) + width);
    if (!cand_covers(cd, q)) return sweep_generic<G>(TileRefs{lv.seg_start, lv.segs, lv.bounds}, r, xo, yo, dx, dy, radius);
    bool in[K];
    bool any = false;
#pragma unroll
    for (int k = 0; k < K; k++) { in[k] = cand_in_box(cd, k, q); any |= in[k]; }
    if (!group_any<G>(any)) return 1;   // most sweeps touch no segment at all
    const double vel_sq = sq(dx) + sq(dy);
    double shortest = 1;
#pragma unroll
    for (int k = 0; k < K; k++)
        if (in[k]) {
            const double t = cand_toi(cd.s[k], cd.x1[k], cd.y1[k], cd.x2[k], cd.y2[k], xo, yo, dx, dy, vel_sq, radius);
            if (t < shortest) shortest = t;
        }
    return group_min<G>(shortest);
}

// ---- closest point: get_single_closest_point (physics.py:131-180), first-wins argmin in the reference's iteration order.
// The cell filter uses the box the segment list was gathered with (c*), the per-segment AABB test the box around the
// current position (q*): the ninja gathers once and then moves (ninja.py:282-285), a query with segments=None has
// both equal.
template <int G, bool UNIFORM = false>
DEV Best region_closest(TileRefs lv, int r, double px, double py, double cx0, double cy0, double cx1, double cy1,
                        double qx0, double qy0, double qx1, double qy1, double bias) {
    Best m;
    m.key = __builtin_inf(); m.idx = 0x7fffffff; m.a = 0; m.b = 0;
    region_walk<G, UNIFORM>(lv, r, cx0, cy0, cx1, cy1, [&](bool valid, uint32_t s, int xc, int yc, int flat) {
        if (!valid) return;
        const Seg g = seg_decode(s, xc, yc);
        double bx0, by0, bx1, by1;
        seg_box(g.x1, g.y1, g.x2, g.y2, bx0, by0, bx1, by1);
        if (bx1 < qx0 || bx0 > qx1 || by1 < qy0 || by0 > qy1) return;
        double a, b;
        const bool back = seg_closest(g, px, py, a, b);
        double distance_sq = sq(px - a) + sq(py - b);
        if (!back) distance_sq -= bias;
        if (distance_sq < m.key) { m.key = distance_sq; m.a = a; m.b = b; m.idx = (flat << 8) | (r << 1) | (back ? 1 : 0); }
    });
    group_argmin<G>(m);
    return m;
}
template <int G>
__device__ __noinline__ Best closest_generic(TileRefs lv, int r, double px, double py, double radius) {
    const double qx0 = px - radius, qy0 = py - radius, qx1 = px + radius, qy1 = py + radius;
    return region_closest<G>(lv, r, px, py, qx0, qy0, qx1, qy1, qx0, qy0, qx1, qy1, 0.1);
}

// the same from candidate registers, for the box q = position +- radius (cell filter and per-segment AABB); same
// per-candidate arithmetic as the ninja's depenetration loop.  (The death balls call this and closest_generic, and
// write their register sweep out, as ball_think always did: routed through tile_sweep and a tile_closest wrapper the
// zoo kernels spilled more and the zoo workload ran 0.27 % slower.)
template <int G, int K>
DEV Best cand_closest_query(const Cand<K> &cd, int r, double px, double py, const QBox &q) {
    Best m;
    m.key = __builtin_inf(); m.idx = 0x7fffffff; m.a = 0; m.b = 0;
#pragma unroll
    for (int k = 0; k < K; k++) {
        if (!cand_in_box(cd, k, q)) continue;
        double bx0, by0, bx1, by1;
        seg_box(cd.x1[k], cd.y1[k], cd.x2[k], cd.y2[k], bx0, by0, bx1, by1);
        if ((bx1 < q.x0) | (bx0 > q.x1) | (by1 < q.y0) | (by0 > q.y1)) continue;
        double a, b;
        const bool back = cand_closest(cd, k, px, py, a, b);
        const double distance_sq = sq(px - a) + sq(py - b);
        const double key = back ? distance_sq : distance_sq - 0.1;
        if (key < m.key) { m.key = key; m.a = a; m.b = b; m.idx = ((k * G + r) << 8) | (r << 1) | (back ? 1 : 0); }
    }
    group_argmin<G>(m);
    return m;
}
// ---- wall probe: the tile terms of Ninja.post_collision (ninja.py:424-441) -------------------------------------------
DEV double wall_term(double px, double py, double a, double b, double rad) {
    double dx = px - a, dy = py - b;
    if (dabs(dy) < 0.00001) {
        double dist = dsqrt(sq(dx) + sq(dy));
        if (0 < dist && dist <= rad) return dx / dist;
    }
    return 0;
}

template <int G>
__device__ __noinline__ double wall_probe_generic(TileRefs lv, int r, double px, double py, double qx0, double qy0,
                                                  double qx1, double qy1, double wall_normal) {
    const double rad = NINJA_RADIUS + 0.1;
    region_walk<G, true>(lv, r, qx0, qy0, qx1, qy1, [&](bool valid, uint32_t s, int xc, int yc, int) {
        double term = 0;
        if (valid) {
            double a, b;
            seg_closest(seg_decode(s, xc, yc), px, py, a, b);
            term = wall_term(px, py, a, b, rad);
        }
        ordered_add<G>(wall_normal, term);
    });
    return wall_normal;
}
