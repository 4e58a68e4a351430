// npp_state.hpp -- the ONE definition of the packed per-env state: the bit fields of the five u32 state planes, the 2-bit entity
// state words, the exit switch's state and what is derived from them (the switch_states row, npp_dump_state's i32 row).  Every
// kernel and every host function that reads or writes these bits does it through this file ("packed state layout", has the
// same table).  No HIP header: the host sources (npp_level.cpp, npp_reach.cpp, npp_host.cpp) also build with plain g++.
#pragma once
#include <cstddef>
#include <cstdint>

#if defined(__HIPCC__) || defined(__HIP__)
#define NPP_HD __host__ __device__
#else
#define NPP_HD
#endif
// the accessors below: inlined before any optimisation runs, so that a kernel compiles to the literal shifts they replace
#define NPP_FIELD_FN NPP_HD constexpr __attribute__((always_inline))

namespace npp {

// ---- the five u32 planes: plane k of env e lives at d_u32[k * n_envs + e] ----------------------------------------------------------
enum U32Plane { U_A = 0, U_B, U_C, U_D, U_E, NU32 };

// One field: the stored bits are value + bias (bias 1: the value starts at -1).  sat: the value saturates at the field's maximum
// when it is stored (a counter that only matters below it) instead of being trusted to fit.
struct StateField {
    int plane, shift, width, bias;
    bool sat;
};
// word A: the ninja's small state
constexpr StateField S_STATE{U_A, 0, 4, 0, false}, S_AIRBORN{U_A, 4, 1, 0, false}, S_AIRBORN_OLD{U_A, 5, 1, 0, false},
    S_WALLED{U_A, 6, 1, 0, false}, S_WN{U_A, 7, 2, 1, false}, S_JIO{U_A, 9, 1, 0, false}, S_HOR{U_A, 10, 2, 1, false},
    S_JUMP{U_A, 12, 1, 0, false}, S_GJUMP{U_A, 13, 1, 0, false}, S_DSLOW{U_A, 14, 1, 0, false}, S_JBUF{U_A, 15, 3, 1, false},
    S_FBUF{U_A, 18, 3, 1, false}, S_WBUF{U_A, 21, 3, 1, false}, S_LBUF{U_A, 24, 3, 1, false}, S_CAUSE{U_A, 27, 2, 0, false},
    S_TIMPACT{U_A, 29, 1, 0, false};
// word B: jump duration (<= 46 in play), floor / ceiling counts, previous state
constexpr StateField S_JDUR{U_B, 0, 6, 0, true}, S_FCOUNT{U_B, 6, 8, 0, true}, S_CCOUNT{U_B, 14, 8, 0, true}, S_PSTATE{U_B, 22, 4, 0, false};
// word C: frames airborne, state change frame
constexpr StateField S_FAIR{U_C, 0, 16, 0, true}, S_SCF{U_C, 16, 16, 0, true};
// word D: frame, gold, doors
constexpr StateField S_FRAME{U_D, 0, 16, 0, true}, S_GOLD{U_D, 16, 8, 0, true}, S_DOORS{U_D, 24, 8, 0, true};
// word E: the cell of the previous mine think, "the cached mine overlay is valid", and the reset history -- fast-ordered (the
// cell lists are in entity_dic order: a Simulator.fast_reset ran), fresh (the level was assigned and no Simulator.reset has run
// since), the episode counter mod 8192 (bumped by every reset)
constexpr StateField S_PCELL{U_E, 0, 16, 0, false}, S_SCVALID{U_E, 16, 1, 0, false}, S_FAST_ORDERED{U_E, 17, 1, 0, false},
    S_FRESH{U_E, 18, 1, 0, false}, S_EPISODE{U_E, 19, 13, 0, false};
// the step kernel carries the three reset-history fields as one value (Nj::fastord)
constexpr StateField S_FASTORD{U_E, S_FAST_ORDERED.shift, S_FAST_ORDERED.width + S_FRESH.width + S_EPISODE.width, 0, false};
// a part of S_FASTORD as a field of that value
constexpr StateField fastord_part(StateField f) { return {f.plane, f.shift - S_FASTORD.shift, f.width, f.bias, f.sat}; }

constexpr StateField STATE_FIELDS[] = {S_STATE, S_AIRBORN, S_AIRBORN_OLD, S_WALLED, S_WN, S_JIO, S_HOR, S_JUMP, S_GJUMP, S_DSLOW, S_JBUF,
                                       S_FBUF, S_WBUF, S_LBUF, S_CAUSE, S_TIMPACT, S_JDUR, S_FCOUNT, S_CCOUNT, S_PSTATE, S_FAIR, S_SCF,
                                       S_FRAME, S_GOLD, S_DOORS, S_PCELL, S_SCVALID, S_FAST_ORDERED, S_FRESH, S_EPISODE};

constexpr uint32_t field_max(StateField f) { return (uint32_t)((1ull << f.width) - 1); }
constexpr uint32_t field_mask(StateField f) { return field_max(f) << f.shift; }
// the fields of a plane lie inside its 32 bits and do not overlap
constexpr bool plane_ok(int plane) {
    uint32_t covered = 0;
    for (StateField f : STATE_FIELDS)
        if (f.plane == plane) {
            if (f.width < 1 || f.shift < 0 || f.shift + f.width > 32 || (covered & field_mask(f))) return false;
            covered |= field_mask(f);
        }
    return true;
}
static_assert(plane_ok(U_A) && plane_ok(U_B) && plane_ok(U_C) && plane_ok(U_D) && plane_ok(U_E), "state fields overlap or leave their word");
static_assert(field_mask(S_FASTORD) == (field_mask(S_FAST_ORDERED) | field_mask(S_FRESH) | field_mask(S_EPISODE)), "S_FASTORD is its three parts");

// one word: the stored bits of a field, its value, and a value's contribution to the word.  field_bits trusts a value without
// `sat` to fit (the writer's invariant), so that the step kernel's store is a chain of ORs and nothing else
NPP_FIELD_FN uint32_t field_raw(uint32_t word, StateField f) { return (word >> f.shift) & field_max(f); }
NPP_FIELD_FN int field_get(uint32_t word, StateField f) { return (int)field_raw(word, f) - f.bias; }
NPP_FIELD_FN uint32_t field_bits(StateField f, int value) {
    return (uint32_t)((f.sat && value > (int)field_max(f) ? (int)field_max(f) : value) + f.bias) << f.shift;
}
// the five words of an env, words[plane]; state_put ORs into words that start as zero
NPP_FIELD_FN uint32_t state_raw(const uint32_t *words, StateField f) { return field_raw(words[f.plane], f); }
NPP_FIELD_FN int state_get(const uint32_t *words, StateField f) { return field_get(words[f.plane], f); }
NPP_FIELD_FN void state_put(uint32_t *words, StateField f, int value) { words[f.plane] |= field_bits(f, value); }
// the SoA planes: a field of env `index` among `stride` envs
NPP_FIELD_FN uint32_t state_word(const uint32_t *planes, size_t stride, size_t index, int plane) { return planes[(size_t)plane * stride + index]; }
NPP_FIELD_FN int state_load(const uint32_t *planes, size_t stride, size_t index, StateField f) {
    return field_get(state_word(planes, stride, index, f.plane), f);
}

// ---- entity state: 2 bits per CSR slot, 16 slots per word; word w of env e at ent_bits[w * n_envs + e] ------------------------------
NPP_FIELD_FN int ent_word(int slot) { return slot >> 4; }
NPP_FIELD_FN int ent_shift(int slot) { return (slot & 15) * 2; }
NPP_FIELD_FN uint32_t ent_field(uint32_t word, int slot) { return (word >> ent_shift(slot)) & 3u; }
NPP_FIELD_FN uint32_t ent_bits_at(uint32_t bits, int slot) { return bits << ent_shift(slot); }   // bits (a state, a mask) at a slot's place
NPP_FIELD_FN uint32_t ent_state(const uint32_t *words, size_t stride, size_t index, int slot) {
    return ent_field(words[(size_t)ent_word(slot) * stride + index], slot);
}

// ---- the exit switch (slot LevelHdr::obs_switch, -1 = the level has none) ------------------------------------------------------------
// Its state is 1 until the ninja collects it and 0 afterwards, never 2 or 3: the level compiler's init word gives an exit switch 1
// (npp_level.cpp), a fast reset keeps bits of boost pads and regular doors only, and the one write the step kernels make to an
// EK_SWITCH slot is the 0 of logical_collisions / logical_collisions_zoo (the 1 of their pending writes goes to the switch's door).
// So "the state is 0, or there is no switch" and "the state is not 1" are one predicate, exit_switch_activated -- the reference's
// `not switch.active` (nplay_headless.py:566-576).
constexpr int EXIT_SWITCH_NONE = 2;   // npp_dump_state column 13 of a level without an exit switch
NPP_FIELD_FN int exit_switch_state(const uint32_t *words, size_t stride, size_t index, int obs_switch) {
    int st = EXIT_SWITCH_NONE;
    if (obs_switch >= 0) st = (int)ent_state(words, stride, index, obs_switch);
    return st;
}
NPP_FIELD_FN bool exit_switch_activated(int sw_state) { return sw_state != 1; }

// ---- switch_states (gym_environment/npp_environment.py:1782-1847): one env's row of up to MAX_LOCKED_DOORS = 5 locked doors x
// [switch x, switch y, door x, door y, collected].  _extract_locked_door_positions looks for `segment.p1`, which GridSegmentLinear
// does not have (entities.py: x1, y1, x2, y2), so the "door" position falls back to the entity's xpos / ypos -- the switch position
// (entity_door_base.py:94-97).  Reproduced as is.  locked_slots: LevelHdr::locked_slots; ent_x / ent_y: the level's entity positions.
NPP_HD inline void switch_states_row(const int32_t *locked_slots, const double *ent_x, const double *ent_y, const uint32_t *words, size_t stride,
                                     size_t index, float *o) {
    for (int k = 0; k < 5; k++) {
        const int slot = locked_slots[k];
        float fx = 0.f, fy = 0.f, collected = 0.f;
        if (slot >= 0) {
            const double sx = ent_x[slot] / 1056.0, sy = ent_y[slot] / 600.0;
            fx = (float)(sx < 0.0 ? 0.0 : (sx > 1.0 ? 1.0 : sx)); fy = (float)(sy < 0.0 ? 0.0 : (sy > 1.0 ? 1.0 : sy));
            collected = (ent_state(words, stride, index, slot) & 1u) ? 0.f : 1.f;
        }
        o[5 * k] = fx; o[5 * k + 1] = fy; o[5 * k + 2] = fx; o[5 * k + 3] = fy; o[5 * k + 4] = collected;
    }
}

// ---- npp_dump_state's i32 row (column meanings: DESIGN.md, "state dump layout") from the five words, the exit switch's state and
// the level.  Columns 3-7 are the stored (biased) bits; the row is STATE_DUMP_I32 = NPP_DUMP_I32 wide, its tail zero.
constexpr int STATE_DUMP_I32 = 32;
inline void state_decode_row(const uint32_t *w, int sw_state, int level, int32_t *o) {
    o[0] = state_get(w, S_STATE); o[1] = state_get(w, S_AIRBORN); o[2] = state_get(w, S_WALLED); o[3] = (int32_t)state_raw(w, S_WN);
    o[4] = (int32_t)state_raw(w, S_JBUF); o[5] = (int32_t)state_raw(w, S_FBUF); o[6] = (int32_t)state_raw(w, S_WBUF);
    o[7] = (int32_t)state_raw(w, S_LBUF); o[8] = state_get(w, S_FCOUNT); o[9] = state_get(w, S_CCOUNT); o[10] = state_get(w, S_JDUR);
    o[11] = !state_get(w, S_GJUMP); o[12] = !state_get(w, S_DSLOW); o[13] = sw_state;
    o[14] = state_get(w, S_GOLD); o[15] = state_get(w, S_DOORS); o[16] = state_get(w, S_FAIR); o[17] = state_get(w, S_SCF);
    o[18] = state_get(w, S_AIRBORN_OLD); o[19] = state_get(w, S_JIO); o[20] = state_get(w, S_CAUSE); o[21] = state_get(w, S_TIMPACT);
    o[22] = state_get(w, S_FRAME); o[23] = state_get(w, S_HOR); o[24] = state_get(w, S_JUMP); o[25] = state_get(w, S_PSTATE);
    o[26] = state_get(w, S_PCELL); o[27] = level;
    for (int k = 28; k < STATE_DUMP_I32; k++) o[k] = 0;
}

}  // namespace npp
