// npp_seed.hpp -- seeding the cell index from recorded replays (include/npp_amd.h, npp_archive_seed): the per-tick
// rows of the rule, shared by the feed kernel (npp_seed.hip) and the host-only entry point (npp_host.cpp:
// npp_archive_seed_rows_host).  No HIP header: the host side also builds with plain g++.  Integer and IEEE f64 / f32 only (the build
// has -ffp-contract=off), so the device and the host entry agree bit for bit.
#pragma once
#include <cstdint>

#include "npp_demo.hpp"   // demo_action_of_byte, the one byte-to-action table

namespace npp {

enum SeedScoreMode { SEED_PROGRESS = 0, SEED_FRAMES = 1, SEED_TABLE = 2 };

// The byte's action does not press what decode_input_to_controls(b) presses (replay/replay_executor.py:42-84): 7 is LEFT + RIGHT +
// JUMP, played as a jump and mapped to NOOP; a byte >= 8 is mapped to NOOP whatever its low three bits press.  A route through
// such a byte does not lead to the state when it is replayed with step(): route bit 2 from this tick on.
NPP_HD inline bool seed_byte_mismatch(uint32_t b) { return b == 7u || (b >= 8u && (b & 7u) != 0u && (b & 7u) != 6u); }

// The score of the state after tick f of a replay of len ticks (modes 0 and 1; mode 2 reads the caller's table).
//   progress  the seeder's frame_idx / max(1, total_frames) (replay/demo_checkpoint_seeder.py:777-779), an fp64 division rounded
//             once to f32
//   frames    the index's own NULL score: -(float)frame with frame = f + 1, the frame counter after the tick (saturating at
//             65535 as S_FRAME does)
NPP_HD inline float seed_score(int mode, int64_t f, int64_t len) {
    if (mode == SEED_FRAMES) return -(float)(f + 1 > 65535 ? (int64_t)65535 : f + 1);
    return (float)((double)f / (double)(len < 1 ? (int64_t)1 : len));
}

}  // namespace npp
