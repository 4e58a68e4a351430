// npp_minimal.hpp -- the columns of the minimal observation that are encodings of the ninja's state (the reference's
// compute_minimal_observation, gym_environment/observation_processor.py:505-567): compiled for the device (npp_reach_kernel.hip)
// and for the host (npp_minimal_encode_host in npp_host.cpp, which the CPU tests compare with numpy on every value of every field).
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__HIP__)
#define NPP_MIN_HD __host__ __device__
#else
#define NPP_MIN_HD
#endif

namespace npp {

constexpr int MINOBS_DIM = 40;
constexpr double MINOBS_MAX_HOR_SPEED = 3.333;   // nclone/constants MAX_HOR_SPEED (the step kernels keep their own copy)

// `buffer / span if buffer >= 0 else -1.0`: the quotient in f64, one rounding to f32 (the np.float32 array assignment).  The
// buffers hold -1 .. 6 (three state bits), so the quotients are constants the compiler folds with exactly that arithmetic instead
// of four f64 divisions per env on the device
NPP_MIN_HD inline float minobs_buffer(int b, double span) {
    return b < 0 ? -1.f : b == 0 ? 0.f : b == 1 ? (float)(1.0 / span) : b == 2 ? (float)(2.0 / span) : b == 3 ? (float)(3.0 / span)
         : b == 4 ? (float)(4.0 / span) : b == 5 ? (float)(5.0 / span) : (float)(6.0 / span);
}

// Columns 0-11 and 36-39 of the row `o` (40 floats) from state word A (bit layout: npp_kernels.hip pack_state / unpack_state: state
// bits 0-3, airborn 4, walled 6, wall normal + 1 bits 7-8, jump / floor / wall / launch pad buffer + 1 bits 15-17, 18-20, 21-23,
// 24-26) and the planes F_VX, F_VY, F_FNX, F_FNY.
NPP_MIN_HD inline void minobs_encode_state(uint32_t A, double vx, double vy, double fnx, double fny, float *o) {
    const uint32_t st = A & 15u;
    const bool airborn = (A >> 4) & 1u, walled = (A >> 6) & 1u;
    const int wn = (int)((A >> 7) & 3u) - 1;
    o[0] = (float)(vx / MINOBS_MAX_HOR_SPEED);
    o[1] = (float)(vy / MINOBS_MAX_HOR_SPEED);
    const uint32_t hot = st < 4u ? st : 4u;   // min(state, 4): falling and every special state share the last slot
    for (uint32_t k = 0; k < 5; k++) o[2 + k] = k == hot ? 1.f : 0.f;
    o[7] = airborn ? 1.f : -1.f;
    o[8] = walled ? 1.f : -1.f;
    o[9] = walled ? (float)wn : 0.f;
    o[10] = (float)fnx;
    o[11] = (float)fny;
    o[36] = minobs_buffer((int)((A >> 15) & 7u) - 1, 5.0);   // jump, floor, wall, launch pad
    o[37] = minobs_buffer((int)((A >> 18) & 7u) - 1, 5.0);
    o[38] = minobs_buffer((int)((A >> 21) & 7u) - 1, 5.0);
    o[39] = minobs_buffer((int)((A >> 24) & 7u) - 1, 4.0);
}

}  // namespace npp
