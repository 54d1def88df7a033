// felics_pairs.h -- the codes of TWO adjacent 8-bit pixels per instruction: what code_pixel / code_in_range (felics_kernels.hip) compute
// per pixel up to the Rice code, on registers that hold one pixel in each 16-bit half (low half = the left pixel).
//
// For u8 samples everything up to the phased-in code fits 16 bits: the neighbour rule, ctx <= 255, d and t (signed, |.| <= 255), the
// masks, val <= 254, n <= 256, P <= 256, 2 P <= 512, the code with its leading `1` (at most 10 bits) and its length (at most 10).  The
// packed instructions (v_pk_min/max/sub/add/ashrrev/lshrrev on 16-bit halves) never carry from one half into the other, and the selects
// are bitwise (v_bitop3_b32), so the halves do not mix.  The Rice code needs up to 32 bits and stays per pixel in the kernel.
//
// Included by felics_kernels.hip and compilable by a plain host compiler with clang's vector extensions (pairs_check.cpp compares
// pair_codes with the scalar formulas for every (p, left, up)): the two AMD builtins have C++ stand-ins outside device code.  No memory
// instruction and no inline assembly in here.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define FELICS_PAIR_FN __host__ __device__ __forceinline__
#else
#define FELICS_PAIR_FN static inline
#endif

namespace felics {

typedef unsigned short pair_u16 __attribute__((ext_vector_type(2)));
typedef short pair_i16 __attribute__((ext_vector_type(2)));

#if defined(__HIP_DEVICE_COMPILE__)
FELICS_PAIR_FN uint32_t pair_perm(uint32_t hi, uint32_t lo, uint32_t sel) { return __builtin_amdgcn_perm(hi, lo, sel); }
template <uint32_t TABLE>
FELICS_PAIR_FN uint32_t pair_bitop3(uint32_t a, uint32_t b, uint32_t c) {
    return __builtin_amdgcn_bitop3_b32(a, b, c, TABLE);
}
#else
// v_perm_b32: byte i of the result is picked by byte i of sel: 0-3 = that byte of lo, 4-7 = of hi, 8-11 = the sign of a 16-bit half
// (lo's, then hi's) spread over the byte, 12 = 0x00, 13 and above = 0xFF
FELICS_PAIR_FN uint32_t pair_perm(uint32_t hi, uint32_t lo, uint32_t sel) {
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
// v_bitop3_b32: bit i of the result = TABLE[a_i << 2 | b_i << 1 | c_i]
template <uint32_t TABLE>
FELICS_PAIR_FN uint32_t pair_bitop3(uint32_t a, uint32_t b, uint32_t c) {
    uint32_t r = 0;
    for (uint32_t m = 0; m < 8; m++)
        if ((TABLE >> m) & 1u) r |= ((m & 4u) ? a : ~a) & ((m & 2u) ? b : ~b) & ((m & 1u) ? c : ~c);
    return r;
}
#endif

constexpr uint32_t PAIR_SEL = 0xE4;      // c ? a : b
constexpr uint32_t PAIR_SEL_NOT = 0x72;  // c ? ~b : a
constexpr uint32_t PAIR_NOR = 0x03;      // ~(a | b)

FELICS_PAIR_FN uint32_t pair_bits(pair_u16 v) { return __builtin_bit_cast(uint32_t, v); }
FELICS_PAIR_FN pair_u16 pair_of(uint32_t v) { return __builtin_bit_cast(pair_u16, v); }
// the sign of each half spread over the half (v_pk_ashrrev_i16 15)
FELICS_PAIR_FN uint32_t pair_sign(pair_u16 v) {
    return __builtin_bit_cast(uint32_t, __builtin_bit_cast(pair_i16, v) >> (pair_i16){15, 15});
}

// ---- Byte selection: the pairs of a dword x of four consecutive samples (byte i = sample i; pair h = samples 2 h, 2 h + 1), each sample
// zero-extended into a half.  One v_perm_b32 each.
// the samples of pair h themselves (also: the samples above them, from the dword of the row above)
FELICS_PAIR_FN uint32_t pair_samples(uint32_t x, uint32_t h) { return h == 0 ? pair_perm(0u, x, 0x0c010c00u) : pair_perm(0u, x, 0x0c030c02u); }
// their left neighbours: pair 1's are samples 1, 2 of x; pair 0's are the last sample of the dword in front (byte 3 of prev) and sample 0
FELICS_PAIR_FN uint32_t pair_lefts(uint32_t prev, uint32_t x, uint32_t h) {
    return h == 0 ? pair_perm(prev, x, 0x0c000c07u) : pair_perm(0u, x, 0x0c020c01u);
}
// the same for pair 0 of a group's first dword: the sample in front of the group is the low byte of `before`
FELICS_PAIR_FN uint32_t pair_lefts_first(uint32_t before, uint32_t x) { return pair_perm(before, x, 0x0c000c04u); }

// ---- One pixel of a pair back in 32 bits (e = 0: the low half, 1: the high half): a value zero-extended, a mask sign-extended
FELICS_PAIR_FN uint32_t pair_value(uint32_t v, uint32_t e) { return e ? v >> 16 : v & 0xFFFFu; }
FELICS_PAIR_FN uint32_t pair_mask(uint32_t m, uint32_t e) { return e ? (uint32_t)((int32_t)m >> 16) : (uint32_t)(int32_t)(int16_t)(m & 0xFFFFu); }

// What code_pixel needs of two pixels before it builds the Rice code, packed (each field in the pixel's own half):
//   val       p - L in range, L - p - 1 below, p - H - 1 above (L, H = min, max of the two neighbours)
//   above     all ones in the half: p > H
//   in_range  all ones in the half: L <= p <= H
//   code_in   `1` in front of p - L phased-in on n = H - L + 1 values (phase_in_coding.rs:59-84), as in code_in_range
//   len_in    its length, with the `1`: m + 1 or m + 2, 2^m = the largest power of two <= n
// code_in and len_in of a pixel out of range are garbage within the pixel's half (d wraps in 16 bits), and harmless: the caller keeps
// the Rice side there.
struct PairCodes {
    uint32_t val, above, in_range, code_in, len_in;
};
// pp = the two pixels, ll = their left neighbours, uu = the samples above them (pair_samples / pair_lefts: each value < 256 in its half)
FELICS_PAIR_FN PairCodes pair_codes(uint32_t pp, uint32_t ll, uint32_t uu) {
    const pair_u16 p = pair_of(pp), a = pair_of(ll), b = pair_of(uu);
    const pair_u16 L = __builtin_elementwise_min(a, b), H = __builtin_elementwise_max(a, b);
    const pair_u16 ctx = H - L;
    const pair_u16 d = p - L;  // in range: 0 <= d <= ctx; below: negative in 16 bits
    const pair_u16 t = H - p;  // negative: above
    const uint32_t below = pair_sign(d);
    PairCodes pc;
    pc.above = pair_sign(t);
    pc.val = pair_bitop3<PAIR_SEL_NOT>(pair_bits(d) ^ below, pair_bits(t), pc.above);  // ~d = L - p - 1 | d | ~t = p - H - 1
    pc.in_range = pair_bitop3<PAIR_NOR>(pc.above, below, 0u);
    // phased-in.  Leading zeros per half: both counts are 16 + clz16 (of the half zero-extended: v_ffbh_u32 with a word select), and
    // v_pk_lshrrev_b16 shifts by the low four bits of each half's count = clz16 itself, so P needs no subtract; the mask below is there
    // for the language (a count of 16 or more is undefined in C++) and folds into the OR that packs the counts.
    const pair_u16 n = ctx + (pair_u16){1, 1};  // 1 <= n <= 256
    const uint32_t nn = pair_bits(n);
    const uint32_t zl = (uint32_t)__builtin_clz(nn & 0xFFFFu), zh = (uint32_t)__builtin_clz(nn >> 16);
    const pair_u16 zz = pair_of(((zh << 16) | zl) & 0x000F000Fu);  // clz16(n) in each half: 7 .. 15
    const pair_u16 P = (pair_u16){0x8000, 0x8000} >> zz;           // 2^m
    const pair_u16 r0 = d + P;
    const pair_u16 r = __builtin_elementwise_min(r0, r0 - n);  // r0 mod n, r0 < 2 n: the difference wraps to more than r0 where r0 < n
    const pair_u16 P2 = P + P, right_p = P2 - n;
    const uint32_t is_short = pair_sign(r - right_p);
    const pair_u16 long_base = P2 + right_p;
    pc.code_in = pair_bits(r + pair_of(pair_bitop3<PAIR_SEL>(pair_bits(P), pair_bits(long_base), is_short)));  // `1` in front of m or m + 1 bits
    pc.len_in = pair_bits((pair_u16){17, 17} - zz + pair_of(is_short));                                          // (33 - clz32 n) - 1 if short
    return pc;
}

}  // namespace felics
