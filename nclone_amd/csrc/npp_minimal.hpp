// npp_minimal.hpp -- the columns of the minimal observation that are encodings of the ninja's state (the reference's
// compute_minimal_observation, gym_environment/observation_processor.py:505-567): compiled for the device (npp_reach_kernel.hip)
// and for the host (npp_minimal_encode_host in npp_host.cpp, which the CPU tests compare with numpy on every value of every field).
#pragma once
#include <cstdint>

#include "npp_state.hpp"

namespace npp {

constexpr int MINOBS_DIM = 40;
constexpr double MINOBS_MAX_HOR_SPEED = 3.333;   // nclone/constants MAX_HOR_SPEED (the step kernels keep their own copy)

// `buffer / span if buffer >= 0 else -1.0`: the quotient in f64, one rounding to f32 (the np.float32 array assignment).  The
// buffers hold -1 .. 6 (three state bits), so the quotients are constants the compiler folds with exactly that arithmetic instead
// of four f64 divisions per env on the device
NPP_HD inline float minobs_buffer(int b, double span) {
    return b < 0 ? -1.f : b == 0 ? 0.f : b == 1 ? (float)(1.0 / span) : b == 2 ? (float)(2.0 / span) : b == 3 ? (float)(3.0 / span)
         : b == 4 ? (float)(4.0 / span) : b == 5 ? (float)(5.0 / span) : (float)(6.0 / span);
}

// Columns 0-11 and 36-39 of the row `o` (40 floats) from state word A (npp_state.hpp: S_STATE, S_AIRBORN, S_WALLED, S_WN and the jump /
// floor / wall / launch pad buffers S_JBUF, S_FBUF, S_WBUF, S_LBUF) and the planes F_VX, F_VY, F_FNX, F_FNY.
NPP_HD inline void minobs_encode_state(uint32_t A, double vx, double vy, double fnx, double fny, float *o) {
    static_assert(S_STATE.plane == U_A && S_AIRBORN.plane == U_A && S_WALLED.plane == U_A && S_WN.plane == U_A && S_JBUF.plane == U_A &&
                  S_FBUF.plane == U_A && S_WBUF.plane == U_A && S_LBUF.plane == U_A, "every field read here is in word A");
    const uint32_t st = field_raw(A, S_STATE);
    const bool airborn = field_get(A, S_AIRBORN), walled = field_get(A, S_WALLED);
    const int wn = field_get(A, S_WN);
    o[0] = (float)(vx / MINOBS_MAX_HOR_SPEED);
    o[1] = (float)(vy / MINOBS_MAX_HOR_SPEED);
    const uint32_t hot = st < 4u ? st : 4u;   // min(state, 4): falling and every special state share the last slot
    for (uint32_t k = 0; k < 5; k++) o[2 + k] = k == hot ? 1.f : 0.f;
    o[7] = airborn ? 1.f : -1.f;
    o[8] = walled ? 1.f : -1.f;
    o[9] = walled ? (float)wn : 0.f;
    o[10] = (float)fnx;
    o[11] = (float)fny;
    o[36] = minobs_buffer(field_get(A, S_JBUF), 5.0);
    o[37] = minobs_buffer(field_get(A, S_FBUF), 5.0);
    o[38] = minobs_buffer(field_get(A, S_WBUF), 5.0);
    o[39] = minobs_buffer(field_get(A, S_LBUF), 4.0);
}

}  // namespace npp
