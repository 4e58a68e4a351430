// npp_episode.hpp -- episode statistics (include/npp_amd.h, npp_set_episode_stats): what the reference puts into `info` at every
// episode end (base_environment.py:1163-1242: "r" = current_ep_reward, created at :156, += reward at :676, zeroed at
// npp_environment.py:587 and :688; "l" = sim.frame; "is_success" / "switch_activated" / "switch_activation_frame" at :546-552;
// "level_id", "from_checkpoint"; episode_pbrs_metrics' pbrs_total and terminal_reward, main_reward_calculator.py:2825-2914), plus a
// per-level table of outcomes.  The rule lives here, shared by the device kernels (npp_episode.hip) and the host-only entry point
// (npp_host.cpp: npp_episode_apply_host).  No HIP header: the host side also builds with plain g++.  The arithmetic is integers
// plus f64 additions in step order, so the device, the host entry and the Python restatement of the tests (tests/episode_ref.py)
// agree bit for bit.
//
// Per env one record: EP_NI i32 words and EP_ND doubles, on the device as SoA planes [EP_NI][n] / [EP_ND][n].
//   i32 0-5    the CURRENT episode: steps | frames | switch_step (1-based step at which NPP_F_SWITCH was first seen, 0 = never) |
//              switch_frames (frames after that step) | level | bits
//   i32 6-11   the FINISHED episode (the one that ended last): the same six
//   i32 12     flags byte of the finished episode's ending step
//   i32 13     n_finished (u32): episodes this env has finished
//   f64 0-6    current: ret | comp[6]          f64 7-13   finished: ret | comp[6]
// The level table: u64[n_levels][16], one 128-byte row per level, columns EpColumn.
#pragma once
#include <cstdint>

#include "npp_state.hpp"   // NPP_HD

namespace npp {

enum EpWord { EP_STEPS = 0, EP_FRAMES, EP_SWITCH_STEP, EP_SWITCH_FRAMES, EP_LEVEL, EP_BITS };
constexpr int EP_WORDS = 6, EP_FIN = 6, EP_FIN_FLAGS = 12, EP_N_FINISHED = 13, EP_NI = 14;
constexpr int EP_RET = 0, EP_COMP = 1, EP_NCOMP = 6, EP_DWORDS = 7, EP_DFIN = 7, EP_ND = 14;
constexpr int EP_CLOSED = 1, EP_FROM_RESTORE = 2, EP_TICKED = 4;
constexpr int EP_F_WON = 1, EP_F_DEAD = 2, EP_F_SWITCH = 4, EP_F_TRUNCATED = 8, EP_F_MINE = 16, EP_F_IMPACT = 32;   // NPP_F_*
constexpr int EP_END_FLAGS = EP_F_WON | EP_F_DEAD | EP_F_TRUNCATED;
enum EpColumn {
    EPC_EPISODES = 0, EPC_WON, EPC_DEAD, EPC_TRUNCATED, EPC_DEAD_MINE, EPC_DEAD_IMPACT, EPC_SWITCH, EPC_STEPS, EPC_FRAMES,
    EPC_WON_FRAMES, EPC_RETURN_FIX, EPC_RESTORED, EPC_ABANDONED, EPC_USED, EP_COLS = 16
};
enum EpEvent { EP_EV_RESET = 0, EP_EV_RESTORE = 1, EP_EV_TICK = 2, EP_EV_INIT = 3, EP_EV_CLEAR = 4 };

struct EpRecord {
    int32_t i[EP_NI];
    double d[EP_ND];
};

// the return as the table adds it: floor(clamp(ret, +-2^42) * 2^20 + 0.5) as a two's-complement 64-bit word.  The product is exact
// (a power of two); NaN counts as 0.  Written without floor(): a truncating conversion, stepped down where it rounded up.
NPP_HD inline uint64_t ep_return_fix(double ret) {
    const double lim = 4398046511104.0;   // 2^42
    if (!(ret == ret)) ret = 0.0;
    if (ret > lim) ret = lim;
    if (ret < -lim) ret = -lim;
    const double t = ret * 1048576.0 + 0.5;
    int64_t q = (int64_t)t;
    if ((double)q > t) q--;
    return (uint64_t)q;
}

// current := empty, on `level`, with `bits`.  COMPS = false leaves the component doubles alone (see ep_row).
template <bool COMPS = true>
NPP_HD inline void ep_start(EpRecord &r, int level, int bits) {
    r.i[EP_STEPS] = 0; r.i[EP_FRAMES] = 0; r.i[EP_SWITCH_STEP] = 0; r.i[EP_SWITCH_FRAMES] = 0;
    r.i[EP_LEVEL] = level; r.i[EP_BITS] = bits;
    r.d[EP_RET] = 0.0;
    if (COMPS)
        for (int k = 0; k < EP_NCOMP; k++) r.d[EP_COMP + k] = 0.0;
}

// INIT: everything zero, both levels -1
NPP_HD inline void ep_init(EpRecord &r) {
    for (int k = 0; k < EP_NI; k++) r.i[k] = 0;
    for (int k = 0; k < EP_ND; k++) r.d[k] = 0.0;
    r.i[EP_LEVEL] = -1;
    r.i[EP_FIN + EP_LEVEL] = -1;
}

// The 16 table deltas of the FINISHED episode of r, to be added to row r.i[EP_FIN + EP_LEVEL].  An episode begun by a restore adds
// to `restored` and to nothing else: it did not start at the spawn, so its length and return say nothing about the level.
NPP_HD inline void ep_deltas(const EpRecord &r, uint64_t d[EP_COLS]) {
    for (int k = 0; k < EP_COLS; k++) d[k] = 0;
    const int32_t *e = r.i + EP_FIN;
    if (e[EP_BITS] & EP_FROM_RESTORE) { d[EPC_RESTORED] = 1; return; }
    const int f = r.i[EP_FIN_FLAGS];
    const bool won = (f & EP_F_WON) != 0, dead = (f & EP_F_DEAD) != 0;
    d[EPC_EPISODES] = 1;
    d[EPC_WON] = won;
    d[EPC_DEAD] = dead;
    d[EPC_TRUNCATED] = (f & EP_F_TRUNCATED) != 0;
    d[EPC_DEAD_MINE] = dead && (f & EP_F_MINE);
    d[EPC_DEAD_IMPACT] = dead && (f & EP_F_IMPACT);
    d[EPC_SWITCH] = e[EP_SWITCH_STEP] != 0;
    d[EPC_STEPS] = (uint64_t)(uint32_t)e[EP_STEPS];
    d[EPC_FRAMES] = (uint64_t)(uint32_t)e[EP_FRAMES];
    d[EPC_WON_FRAMES] = won ? (uint64_t)(uint32_t)e[EP_FRAMES] : 0;
    d[EPC_RETURN_FIX] = ep_return_fix(r.d[EP_DFIN + EP_RET]);
}

// One step row of the env: the step's flags byte f, frame count x, reward, the six reward components (COMPS), the level the env
// plays after the launch, whether the handle auto-resets.  Returns true when the row ended the episode: the finished half of r then
// holds it and the caller adds ep_deltas(r) to the table.  An env that is terminal and not auto-reset executes 0 frames
// (npp_kernels.hip: `live`); a TRUNCATED one keeps stepping there, and EP_CLOSED keeps it from being counted again.  An episode
// takes its level at its first row.  COMPS = false: the component doubles are neither read nor written, current or finished.
template <bool COMPS>
NPP_HD inline bool ep_row(EpRecord &r, int f, int x, float reward, const float *comps, int level_now, bool autoreset) {
    if (x == 0 || (r.i[EP_BITS] & EP_CLOSED)) return false;
    if (r.i[EP_STEPS] == 0) r.i[EP_LEVEL] = level_now;
    r.i[EP_STEPS]++;
    r.i[EP_FRAMES] += x;
    r.d[EP_RET] += (double)reward;
    if (COMPS)
        for (int k = 0; k < EP_NCOMP; k++) r.d[EP_COMP + k] += (double)comps[k];
    if ((f & EP_F_SWITCH) && r.i[EP_SWITCH_STEP] == 0) {
        r.i[EP_SWITCH_STEP] = r.i[EP_STEPS];
        r.i[EP_SWITCH_FRAMES] = r.i[EP_FRAMES];
    }
    if (!(f & EP_END_FLAGS)) return false;
    for (int k = 0; k < EP_WORDS; k++) r.i[EP_FIN + k] = r.i[k];
    r.i[EP_FIN_FLAGS] = f;
    r.i[EP_N_FINISHED] = (int32_t)((uint32_t)r.i[EP_N_FINISHED] + 1u);
    r.d[EP_DFIN + EP_RET] = r.d[EP_RET];
    if (COMPS)
        for (int k = 0; k < EP_NCOMP; k++) r.d[EP_DFIN + EP_COMP + k] = r.d[EP_COMP + k];
    if (autoreset) ep_start<COMPS>(r, level_now, 0);
    else r.i[EP_BITS] |= EP_CLOSED;
    return true;
}

// An event from outside the step.  RESET / RESTORE: the current episode is dropped and an empty one starts on `level_now` (RESTORE:
// marked EP_FROM_RESTORE); returns the level whose `abandoned` column gains 1 -- the dropped episode had steps, was not closed and
// was not begun by a restore -- or -1.  CLEAR: the same without counting (the replay players).  TICK marks the current episode.
// The finished episode and n_finished stay, except under INIT.
NPP_HD inline int ep_event(EpRecord &r, int event, int level_now) {
    if (event == EP_EV_INIT) { ep_init(r); return -1; }
    if (event == EP_EV_TICK) { r.i[EP_BITS] |= EP_TICKED; return -1; }
    int charged = -1;
    if (event != EP_EV_CLEAR && r.i[EP_STEPS] > 0 && !(r.i[EP_BITS] & (EP_CLOSED | EP_FROM_RESTORE))) charged = r.i[EP_LEVEL];
    ep_start<true>(r, level_now, event == EP_EV_RESTORE ? EP_FROM_RESTORE : 0);
    return charged;
}

}  // namespace npp
