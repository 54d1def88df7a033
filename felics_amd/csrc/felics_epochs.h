// felics_epochs.h -- the epoch rules of the three buffers a context keeps valid between calls by a tag instead of a clear:
//   the look-back status words of k_pack_t (a lane's `status`): tag = the low LOOKBACK_EPOCH_BITS bits of the lane's epoch, one epoch
//       per sub-batch (run_lane);
//   the dense estimator tables of k_decode16 (`dec_table`): tag = the whole 32-bit epoch, three consecutive epochs per pass;
//   the hashed estimator tables of k_decode16_lanes (`dec_lane16_table`): tag = 15 bits (felics_lanetable.h), three consecutive
//       epochs per launch, all within 1 .. DEC16L_EPOCH_MAX.
// Each rule takes the LAST epoch handed out on the buffer (0 on a fresh, zeroed one) and answers the epoch to use next (the first
// of three for the decoders, whose callers then keep `epoch + 2` as the last) and whether the buffer has to be cleared in front of
// the launch that uses it; the caller queues that clear on the stream the launch runs on.  What the kernels rely on, and what
// epoch_check.cpp walks every rule for over a whole period and its wrap:
//   - between two clears no tag value is handed out twice;
//   - tag 0 is handed out directly behind a clear at most, where a zeroed word still reads as "nothing" (the look-back's state 0);
//     the decoders never hand it out at all (a zeroed row is an empty row).
// The host code (felics_encode.cpp, felics_decode_device.cpp) and the native check compile these same functions.
#pragma once
#include <stdint.h>

#include "felics_lanetable.h"

namespace felics {

constexpr uint32_t LOOKBACK_EPOCH_BITS = 18;
constexpr uint32_t LOOKBACK_EPOCH_MASK = (1u << LOOKBACK_EPOCH_BITS) - 1u;  // ST_EPOCH_MASK of the status words (felics_codes.h)
constexpr uint32_t DEC16_EPOCH_LAST = 0xFFFFFFF0u;  // the wave form clears once its counter has passed this

struct EpochStep {
    uint32_t epoch;  // the epoch to use (the decoders: the first of three)
    bool clear;      // zero the buffer first
};

// The look-back's: the 32-bit counter runs over by itself; every value whose tag bits are zero -- 0x40000, 0x80000, ... and 0 behind
// 0xFFFFFFFF -- clears, so a period of tags is the 2^18 sub-batches between two clears and tag 0 is the first of each.
FELICS_HD EpochStep lookback_epoch_next(uint32_t last) {
    const uint32_t epoch = last + 1u;
    return EpochStep{epoch, (epoch & LOOKBACK_EPOCH_MASK) == 0u};
}

// k_decode16's: epochs last + 1 .. last + 3; behind DEC16_EPOCH_LAST the tables are cleared and the epochs start over at 1 .. 3
// (last + 3 then never overflows: last <= 0xFFFFFFF0).
FELICS_HD EpochStep dec16_epoch_next(uint32_t last) {
    if (last > DEC16_EPOCH_LAST) return EpochStep{1u, true};
    return EpochStep{last + 1u, false};
}

// k_decode16_lanes': epochs last + 1 .. last + 3 while they stay within DEC16L_EPOCH_MAX, otherwise a clear and 1 .. 3: a clear
// every 10 922 launches, on launch 10 923 of a buffer ((0x7FFF - 2) / 3 launches fit).
FELICS_HD EpochStep dec16_lanes_epoch_next(uint32_t last) {
    if (last > DEC16L_EPOCH_MAX - 3u) return EpochStep{1u, true};
    return EpochStep{last + 1u, false};
}

}  // namespace felics
