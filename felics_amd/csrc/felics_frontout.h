// felics_frontout.h -- the pure pieces of k_front's back half (felics_kernels.hip, steps 3 and 5, FELICS_FORMS bit 256): the sorted tile
// lies in LDS in SLOT order -- contexts ascending, every context's run padded to whole records of 16, a padding slot all ones -- and
// goes out four consecutive slots a thread: one word (u8 planes) or two (Y / Co / Cg planes) of values, two words of pixel offsets.
//
// An entry: context << 22 | value << 13 | above << 12 | pixel offset in the tile (bit 31 clear), or all ones in a padding slot.
//   pix = offset | above << 12 = the low 13 bits; 0xFFFF in a padding slot (the mask alone would leave 0x1FFF: pixel 4095, above)
//   ev  = the value; whatever falls out in a padding slot (nobody reads it)
//
// Included by felics_kernels.hip and compilable by a plain host compiler (frontout_check.cpp compares every piece with its scalar
// definition): the AMD builtin has a C++ stand-in outside device code.  No memory instruction and no inline assembly in here.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define FELICS_FRONTOUT_FN __host__ __device__ __forceinline__
#else
#define FELICS_FRONTOUT_FN static inline
#endif

namespace felics {

#if defined(__HIP_DEVICE_COMPILE__)
FELICS_FRONTOUT_FN uint32_t frontout_perm(uint32_t hi, uint32_t lo, uint32_t sel) { return __builtin_amdgcn_perm(hi, lo, sel); }
// (a & c) | (b & ~c) as one v_bitop3_b32
FELICS_FRONTOUT_FN uint32_t frontout_select(uint32_t a, uint32_t b, uint32_t c) { return __builtin_amdgcn_bitop3_b32(a, b, c, 0xE4); }
#else
FELICS_FRONTOUT_FN uint32_t frontout_select(uint32_t a, uint32_t b, uint32_t c) { return (a & c) | (b & ~c); }
// v_perm_b32: byte i of the result is picked by byte i of sel: 0-3 = that byte of lo, 4-7 = of hi, 8-11 = the sign of a 16-bit half
// (lo's, then hi's) spread over the byte, 12 = 0x00, 13 and above = 0xFF
FELICS_FRONTOUT_FN uint32_t frontout_perm(uint32_t hi, uint32_t lo, uint32_t sel) {
    const uint64_t src = ((uint64_t)hi << 32) | lo;
    uint32_t r = 0;
    for (uint32_t i = 0; i < 4; i++) {
        const uint32_t s = (sel >> (8 * i)) & 0xFFu;
        uint32_t b;
        if (s <= 7) b = (uint32_t)(src >> (8 * s)) & 0xFFu;
        else if (s <= 11) b = ((src >> (16 * (s - 8) + 15)) & 1u) ? 0xFFu : 0u;
        else b = s == 12 ? 0u : 0xFFu;
        r |= b << (8 * i);
    }
    return r;
}
#endif

constexpr uint32_t FRONTOUT_KEY = 0xFFC00FFFu;  // context and pixel offset of an entry
constexpr uint32_t FRONTOUT_PAD = 0xFFFFFFFFu;  // a padding slot
constexpr uint32_t FRONTOUT_REC = 16;           // slots per record (felics_kernels.h: REC)

// ---- step 5: two entries -> the word of their two pix.  The low halves side by side (one v_perm_b32), the entries' signs spread over
// the halves (another: a padding slot is the one entry with bit 31 set), and the low 13 bits of the first under the rest of the second
// (one v_bitop3_b32).
FELICS_FRONTOUT_FN uint32_t frontout_pix_pair(uint32_t r0, uint32_t r1) {
    const uint32_t low = frontout_perm(r1, r0, 0x05040100u);
    const uint32_t pad = frontout_perm(r1, r0, 0x0b0b0909u);
    return frontout_select(low, pad, 0x1FFF1FFFu);
}
// the values of four entries as four bytes (u8 planes: value < 256, bits 13 .. 20 of the entry)
FELICS_FRONTOUT_FN uint32_t frontout_ev_u8(uint32_t r0, uint32_t r1, uint32_t r2, uint32_t r3) {
    const uint32_t lo = frontout_perm(r1 >> 13, r0 >> 13, 0x0c0c0400u);  // {r0's byte, r1's byte, 0, 0}
    const uint32_t hi = frontout_perm(r3 >> 13, r2 >> 13, 0x04000c0cu);  // {0, 0, r2's byte, r3's byte}
    return lo | hi;
}
// the values of two entries as two 16-bit fields (Y / Co / Cg planes: value < 512)
FELICS_FRONTOUT_FN uint32_t frontout_ev_u16(uint32_t r0, uint32_t r1) {
    return frontout_perm(r1 >> 13, r0 >> 13, 0x05040100u) & 0x01FF01FFu;
}

// ---- step 5's order check: an entry and the entry in the next slot.  A violation: both of one tile, and (context, pixel offset) does
// not ascend strictly.  A padding successor passes by construction (its key is larger than any entry's); a padding slot has no
// successor to be compared with (the next run starts a context of its own: its place comes from the counts, not from the ranks).
// As two cheap instructions an entry and one compare a pair: the key with the bits between context and offset all SET orders the
// entries as the masked key does and leaves a padding slot all ones; one more than it is 0 for a padding slot -- nothing is below
// that -- and does not wrap for an entry (bit 31 clear).  next <= this  <=>  next < this + 1.
FELICS_FRONTOUT_FN uint32_t frontout_key(uint32_t e) { return e | ~FRONTOUT_KEY; }
FELICS_FRONTOUT_FN bool frontout_pair_bad(uint32_t r, uint32_t nxt) { return frontout_key(nxt) < frontout_key(r) + 1u; }

// ---- step 3: the tile's layout.  Two running sums in one register over the contexts in ascending order: the events in front (low
// half) and the slots in front (high half: every run rounded up to whole records).  No carry between the halves: at most 4096 events.
FELICS_FRONTOUT_FN uint32_t frontout_layout_term(uint32_t events) {
    return events | (((events + FRONTOUT_REC - 1u) & ~(FRONTOUT_REC - 1u)) << 16);
}
// where wave w's events of a context begin: the context's first slot (the high half of the sums in front of it) + the events of the
// waves in front of w.  cursor[w] for the four waves, from their counts n[w].
FELICS_FRONTOUT_FN void frontout_slot_bases(uint32_t sums_in_front, const uint32_t (&n)[4], uint32_t (&cursor)[4]) {
    uint32_t at = sums_in_front >> 16;
    for (uint32_t w = 0; w < 4; w++) {
        cursor[w] = at;
        at += n[w];
    }
}

// ---- which tiles go out this way: those whose slots fit the LDS window at once
FELICS_FRONTOUT_FN bool frontout_one_window(uint32_t slots, uint32_t window) { return slots <= window; }

}  // namespace felics
