// felics_lanewalk.h -- what ONE LANE of the lane-per-stream decoders does (k_decode8_lanes, k_decode8_seg_lanes, k_decode16_lanes,
// felics_gpudecode.hip): the bit reader, the groups of four samples, the pieces of the pixel step, the two estimators, the walk over a
// whole plane and the walk over a segment from its checkpoint.  It is scalar code per lane -- no cross-lane operation, no block index:
// those stay in the kernels (lane_view, the ballots, the cooperative checkpoint copy) -- so the kernels and a host program
// (lanewalk_check.cpp, under AddressSanitizer too) compile these same functions, and what the comments below promise about the
// addresses a walk touches is checked there on buffers of exactly that size.  On the host a lane's "LDS column" is an ordinary array
// with the same stride of 64 dwords.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/felics.h"
#include "felics_lanetable.h"

// a piece of the step: inlined into its caller on either side
#define FELICS_HDI FELICS_HD __attribute__((always_inline))
// lanewalk_check.cpp counts the pixels that take the rare paths (`cold`, `long_code`); nothing anywhere else
#ifndef FELICS_LANEWALK_NOTE
#define FELICS_LANEWALK_NOTE(what) ((void)0)
#endif

namespace felics {

constexpr uint32_t DEC8L_HOT = 32;                 // contexts per stream in LDS: 64 x 32 x 12 B = 24 KB per wave
constexpr uint32_t DEC8L_TABLE_DW = 256 * 3;       // dwords per stream in HBM: 256 contexts x three pairs of u16 counters
constexpr uint32_t DEC8L_TABLE_DW_RGB = 512 * 3;   // per plane of an RGB stream (contexts 0 .. 510)

template <typename T>
FELICS_HDI T lane_min(T a, T b) { return b < a ? b : a; }
template <typename T>
FELICS_HDI T lane_max(T a, T b) { return a < b ? b : a; }

// MSB-first bit reader of ONE LANE over [base, base + len) (bitstream-io BitReader<_, BigEndian>).  It loads the ALIGNED dwords that
// hold a stream byte: up to three bytes in front of `base` and behind the stream's end are read with them, never looked at.
struct LaneReader {
    const uint32_t *al;   // aligned-down dword pointer of the stream's first byte
    uint32_t total_dw;    // dwords from `al` that hold stream bytes
    uint32_t pos;         // dwords moved into acc so far
    uint32_t nxt;         // dword `pos` as it lies in memory (zero past the end): asked for when dword pos - 1 was taken and first
                          // LOOKED AT when it is taken itself (the byte swap at the load would be a wait for the load)
    uint64_t acc;         // unread bits, left-aligned
    uint32_t navail;      // valid bits in acc
    uint64_t end_bit;     // bits from `al` to the end of the stream

    FELICS_HDI uint32_t fetch(uint32_t i) const { return i < total_dw ? al[i] : 0u; }
    FELICS_HDI void init(const uint8_t *p, uint64_t n) {
        const uint32_t skew = (uint32_t)(reinterpret_cast<uintptr_t>(p) & 3u);
        al = reinterpret_cast<const uint32_t *>(p - skew);
        total_dw = (uint32_t)lane_min<uint64_t>((skew + n + 3u) >> 2, 0xFFFFFFFFull);
        pos = 0;
        nxt = fetch(0);
        acc = 0;
        navail = 0;
        end_bit = (skew + n) * 8u;
        refill();
        if (skew) {  // the first dword starts before the stream: drop those bytes
            acc <<= 8u * skew;
            navail -= 8u * skew;
        }
    }
    // the same, positioned `bit` bits behind p (bit <= 8 n: the caller's check, so the first dword asked for holds a stream byte or lies
    // right behind the last one; like every fetch it is bounded by total_dw)
    FELICS_HDI void init_at(const uint8_t *p, uint64_t n, uint64_t bit) {
        const uint32_t skew = (uint32_t)(reinterpret_cast<uintptr_t>(p) & 3u);
        al = reinterpret_cast<const uint32_t *>(p - skew);
        total_dw = (uint32_t)lane_min<uint64_t>((skew + n + 3u) >> 2, 0xFFFFFFFFull);
        end_bit = (skew + n) * 8u;
        const uint64_t at = 8u * skew + bit;
        pos = (uint32_t)lane_min<uint64_t>(at >> 5, 0xFFFFFFFEull);
        nxt = fetch(pos);
        acc = 0;
        navail = 0;
        refill();
        acc <<= (uint32_t)(at & 31u);
        navail -= (uint32_t)(at & 31u);
    }
    // bits consumed so far, counted from p (the pointer init / init_at was given)
    FELICS_HDI uint64_t bit_pos(const uint8_t *p) const {
        return (uint64_t)pos * 32u - navail - 8u * (uint32_t)(reinterpret_cast<uintptr_t>(p) & 3u);
    }
    // at least 33 valid bits in acc afterwards (zeros past the end of the stream)
    FELICS_HDI void refill() {
        if (navail <= 32u) {
            acc |= (uint64_t)__builtin_bswap32(nxt) << (32u - navail);
            navail += 32u;
            pos++;
            nxt = fetch(pos);
        }
    }
    FELICS_HDI uint32_t take(uint32_t n) {  // the next n <= 32 bits; the caller has refilled (n <= navail)
        const uint32_t v = n ? (uint32_t)(acc >> (64u - n)) : 0u;
        acc <<= n;
        navail -= n;
        return v;
    }
    FELICS_HDI uint32_t get(uint32_t n) {
        refill();
        return take(n);
    }
    FELICS_HDI bool failed() const { return (uint64_t)pos * 32u - navail > end_bit; }
    FELICS_HDI uint64_t unary0() {  // ones before the first zero, the zero consumed (read_unary0)
        uint64_t q = 0;
        while (true) {
            refill();
            const uint32_t top = (uint32_t)(acc >> 32);
            const uint32_t ones = top == 0xFFFFFFFFu ? 32u : (uint32_t)__builtin_clz(~top);
            if (ones == 32u) {
                q += 32u;
                take(32u);
                if (failed()) return q;
                continue;
            }
            take(ones + 1u);
            return q + ones;
        }
    }
};

// four consecutive samples of a stream's own output plane (one unaligned load / store; the plane is this lane's to write and to read)
template <typename ST>
struct Four;
template <>
struct Four<uint8_t> {
    uint32_t v;
    FELICS_HDI void clear() { v = 0; }
    FELICS_HDI void load(const uint8_t *p) { __builtin_memcpy(&v, p, 4); }
    FELICS_HDI void load_n(const uint8_t *p, uint32_t n) {  // samples 0 .. n - 1 only (n < 4), nothing behind them touched
        v = 0;
        for (uint32_t j = 0; j < n; j++) v |= (uint32_t)p[j] << (8u * j);
    }
    FELICS_HDI void store(uint8_t *p) const { __builtin_memcpy(p, &v, 4); }
    FELICS_HDI int get(uint32_t j) const { return (int)((v >> (8u * j)) & 0xFFu); }
    FELICS_HDI void set(uint32_t j, int s) { v |= (uint32_t)s << (8u * j); }  // (0 <= s <= 255, the field still zero)
};
template <>
struct Four<int16_t> {
    uint32_t lo, hi;  // (two named dwords: an array indexed by the sample's number went to scratch memory)
    FELICS_HDI void clear() { lo = hi = 0; }
    FELICS_HDI void load(const int16_t *p) {
        uint32_t v[2];
        __builtin_memcpy(v, p, 8);
        lo = v[0];
        hi = v[1];
    }
    FELICS_HDI void store(int16_t *p) const {
        const uint32_t v[2] = {lo, hi};
        __builtin_memcpy(p, v, 8);
    }
    FELICS_HDI int get(uint32_t j) const { return (int)(int16_t)(((j & 2u) ? hi : lo) >> (16u * (j & 1u))); }
    FELICS_HDI void set(uint32_t j, int s) {  // (the field still zero)
        const uint32_t f = ((uint32_t)s & 0xFFFFu) << (16u * (j & 1u));
        lo |= (j & 2u) ? 0u : f;
        hi |= (j & 2u) ? f : 0u;
    }
};
template <>
struct Four<uint16_t> {
    uint32_t lo, hi;
    FELICS_HDI void clear() { lo = hi = 0; }
    FELICS_HDI void load(const uint16_t *p) {
        uint32_t v[2];
        __builtin_memcpy(v, p, 8);
        lo = v[0];
        hi = v[1];
    }
    FELICS_HDI void load_n(const uint16_t *p, uint32_t n) {  // samples 0 .. n - 1 only (n < 4)
        lo = hi = 0;
        for (uint32_t j = 0; j < n; j++) set(j, (int)p[j]);
    }
    FELICS_HDI void store(uint16_t *p) const {
        const uint32_t v[2] = {lo, hi};
        __builtin_memcpy(p, v, 8);
    }
    FELICS_HDI int get(uint32_t j) const { return (int)((((j & 2u) ? hi : lo) >> (16u * (j & 1u))) & 0xFFFFu); }
    FELICS_HDI void set(uint32_t j, int s) {  // (0 <= s <= 65535, the field still zero)
        const uint32_t f = (uint32_t)s << (16u * (j & 1u));
        lo |= (j & 2u) ? 0u : f;
        hi |= (j & 2u) ? f : 0u;
    }
};
// sixteen bytes as one access: four int32 samples at the samples' own alignment; an estimator row's quarter, aligned (four named words: of
// a vector type the search's loop loaded the whole quarter where it looks at the tag word alone)
typedef uint32_t LaneQuad4 __attribute__((vector_size(16), aligned(4)));
struct alignas(16) LaneQuad {
    uint32_t x, y, z, w;
};
template <>
struct Four<int32_t> {
    uint64_t lo, hi;  // samples 0 | 1 and 2 | 3 (picked out with shifts: selects between four named dwords came back as an indexed array)
    FELICS_HDI void clear() { lo = hi = 0; }
    FELICS_HDI void load(const int32_t *p) {
        const LaneQuad4 q = *reinterpret_cast<const LaneQuad4 *>(p);
        lo = (uint64_t)q[0] | ((uint64_t)q[1] << 32);
        hi = (uint64_t)q[2] | ((uint64_t)q[3] << 32);
    }
    FELICS_HDI void store(int32_t *p) const {
        const LaneQuad4 q = {(uint32_t)lo, (uint32_t)(lo >> 32), (uint32_t)hi, (uint32_t)(hi >> 32)};
        *reinterpret_cast<LaneQuad4 *>(p) = q;
    }
    FELICS_HDI int get(uint32_t j) const { return (int)(uint32_t)(((j & 2u) ? hi : lo) >> (32u * (j & 1u))); }
    FELICS_HDI void set(uint32_t j, int s) {  // (the field still zero)
        const uint64_t f = (uint64_t)(uint32_t)s << (32u * (j & 1u));
        lo |= (j & 2u) ? 0ull : f;
        hi |= (j & 2u) ? f : 0ull;
    }
};

// ---- the pieces of a pixel's step ----

// The two neighbours of pixel (x, y), not one of the plane's first two (misc.rs:14-23): left and above; in row 0 the two to the left; in
// column 0 above and `first_col2`.  ctx = hi - lo: every sample kept is in range, so it is inside the estimator.
struct LaneNeighbours {
    int hi, lo;
    uint32_t ctx;
};
FELICS_HDI LaneNeighbours lane_neighbours(uint32_t x, uint32_t y, int left, int left2, int above, int first_col2) {
    const bool row0 = y == 0, col0 = x == 0 && !row0;
    const int v1 = col0 ? above : left;
    const int v2 = col0 ? first_col2 : (row0 ? left2 : above);
    const int hi = lane_max(v1, v2), lo = lane_min(v1, v2);
    return LaneNeighbours{hi, lo, (uint32_t)(hi - lo)};
}

// In range: `1`, then the phased-in code of p - L in m or m + 1 bits (phase_in_coding.rs:86-112), off the top 32 bits of the reader
// (m <= 8 for an 8-bit plane, <= 16 for a 16-bit one: at most 18 bits).  Worked out whatever the flag says.
struct LaneInRange {
    int pv;
    uint32_t bits;
};
FELICS_HDI LaneInRange lane_in_range(uint32_t top, uint32_t ctx, int lo) {
    const uint32_t nn = ctx + 1;
    const uint32_t m = 31u - (uint32_t)__builtin_clz(nn);
    const uint32_t right_p = (2u << m) - nn, left_p = nn - (1u << m);
    const uint32_t t1 = top << 1;
    uint32_t r = (t1 >> 1) >> (31u - m);               // the m bits behind the flag
    const uint32_t extra = (t1 >> (31u - m)) & 1u;      // the bit behind them
    const uint32_t longer = r >= right_p ? 1u : 0u;     // the code has one more bit
    r = longer ? (r - right_p) * 2u + right_p + extra : r;
    uint32_t rot = r + left_p;                          // rotate_left: (r + left_p) mod n, r < n
    rot = rot >= nn ? rot - nn : rot;
    return LaneInRange{lo + (int)rot, 1u + m + longer};
}

// Out of range: `0`, above / below flag, q ones, `0`, k bits -- off the same 32 bits when it fits in them (k <= 14)
struct LaneRice {
    uint32_t e, nbits;  // the operand, and the whole code's bits with its two flags
    bool fits;          // false: e and nbits mean nothing, lane_rice_long reads the code
};
FELICS_HDI LaneRice lane_rice_short(uint32_t top, uint32_t k) {
    const uint32_t t2 = top << 2;                                  // 30 bits of the stream, two zeros behind them
    const uint32_t ones = (uint32_t)__builtin_clz(~t2);            // (<= 30: ~t2 ends in ones)
    const bool fits = ones + 1u + k <= 30u;                        // unary part, its zero and the k bits lie inside the 30
    const uint32_t e = (ones << k) + (((t2 << (ones & 31u)) << 1 >> 1) >> (31u - k));  // k bits behind the zero
    return LaneRice{e, 3u + ones + k, fits};
}
// a long code (or the end of the stream): the general reader, bit field by bit field, bounded by the stream's length.  No sample of a
// plane is more than `limit` from its neighbours (1024 for 8-bit planes, 262144 for 16-bit ones): the operand is 0 then, with the code.
FELICS_HDI uint32_t lane_rice_long(LaneReader &br, uint32_t k, uint32_t limit, int &rc) {
    FELICS_LANEWALK_NOTE(long_code);
    br.take(2);
    const uint64_t q = br.unary0();
    const uint64_t e64 = (q << k) + br.get(k);
    uint32_t e = (uint32_t)e64;
    if (e64 > limit) {
        if (rc == FELICS_OK) rc = e64 > 0xFFFFFFFFull ? FELICS_E_VALUE_OVERFLOW : FELICS_E_INVALID_VALUE;
        e = 0;
    }
    return e;
}

// update (parameter_selection.rs:49-68): add the N Rice lengths; the row is halved (shift 1) when the smallest passes 1024
template <uint32_t N>
FELICS_HDI uint32_t lane_estimator_update(uint32_t (&S)[N], uint32_t e) {
    uint32_t mn = 0xFFFFFFFFu;
#pragma unroll
    for (uint32_t kk = 0; kk < N; kk++) {
        S[kk] += (e >> kk) + 1u + kk;
        mn = lane_min(mn, S[kk]);
    }
    return mn > 1024u ? 1u : 0u;
}

// ---- the 8-bit step ----

// The estimator of an 8-bit plane: three pairs of 16-bit counters per context; the first DEC8L_HOT contexts in the lane's column of the
// wave's LDS block ([context][pair][lane]: dword i of the lane at myhot[i * 64]), the others in tab[ctx * 3 + pair].
struct Lane8Estimator {
    uint32_t *myhot, *tab;
};

// Pixel (x, y) of an 8-bit plane, as decoded.  Every lane works out both kinds of code under its own flag: the context's row is
// fetched whether the pixel turns out to be an event or not (no divergence, and the LDS round trip runs beside the arithmetic).
FELICS_HDI int lane8_pixel(LaneReader &br, const Lane8Estimator &est, uint32_t x, uint32_t y, int left, int left2, int above, int first_col2,
                           int &rc) {
    const LaneNeighbours nb = lane_neighbours(x, y, left, left2, above, first_col2);
    const uint32_t ctx = nb.ctx;  // <= 255 (510)
    const bool is_hot = ctx < DEC8L_HOT;
    const uint32_t hrow = lane_min(ctx, DEC8L_HOT - 1u) * 3u * 64u;
    uint32_t w01 = est.myhot[hrow], w23 = est.myhot[hrow + 64], w45 = est.myhot[hrow + 128];
    br.refill();  // >= 33 valid bits: both kinds of code are read off the top 32 of them, then consumed in one go
    const uint32_t top = (uint32_t)(br.acc >> 32);
    const bool in_range = (top >> 31) != 0;
    const LaneInRange in = lane_in_range(top, ctx, nb.lo);
    const bool above_flag = ((top >> 30) & 1u) != 0;
    if (!in_range && !is_hot) {  // (noise: a cold context's row comes from the table in HBM)
        FELICS_LANEWALK_NOTE(cold);
        w01 = est.tab[ctx * 3 + 0];
        w23 = est.tab[ctx * 3 + 1];
        w45 = est.tab[ctx * 3 + 2];
    }
    uint32_t S[6] = {w01 & 0xFFFFu, w01 >> 16, w23 & 0xFFFFu, w23 >> 16, w45 & 0xFFFFu, w45 >> 16};
    // get_k: smallest counter, ties to the largest k (parameter_selection.rs:71-85)
    const uint32_t key = lane_min(lane_min(lane_min((S[0] << 3) | 7u, (S[1] << 3) | 6u), lane_min((S[2] << 3) | 5u, (S[3] << 3) | 4u)),
                                  lane_min((S[4] << 3) | 3u, (S[5] << 3) | 2u));
    const uint32_t k = 7u - (key & 7u);
    const LaneRice rice = lane_rice_short(top, k);  // (k <= 5: the operand stays below 1024)
    uint32_t e = rice.e;
    uint32_t nbits = in_range ? in.bits : rice.nbits;
    if (!in_range && !rice.fits) {
        e = lane_rice_long(br, k, 1024u, rc);
        nbits = 0;
    }
    br.acc <<= nbits;  // (nbits <= 32 < the valid bits)
    br.navail -= nbits;
    if (!in_range) {
        const uint32_t hsh = lane_estimator_update(S, e);
        w01 = (S[0] >> hsh) | ((S[1] >> hsh) << 16);
        w23 = (S[2] >> hsh) | ((S[3] >> hsh) << 16);
        w45 = (S[4] >> hsh) | ((S[5] >> hsh) << 16);
        if (is_hot) {
            est.myhot[hrow] = w01;
            est.myhot[hrow + 64] = w23;
            est.myhot[hrow + 128] = w45;
        } else {
            est.tab[ctx * 3 + 0] = w01;
            est.tab[ctx * 3 + 1] = w23;
            est.tab[ctx * 3 + 2] = w45;
        }
    }
    return in_range ? in.pv : (above_flag ? nb.hi + (int)e + 1 : nb.lo - (int)e - 1);
}

// try_into::<u8>() (for RGB planes: the estimator's context bound) would fail on anything outside the range: remembered in
// `out_of_range` (gray: the OR of every sample as decoded, above 255 if one did not fit eight bits, negative ones included; RGB:
// nonzero if one was outside -255 .. 255) and reported at the end of the row; the sample is cut into the range, so that a failed
// stream's contexts stay inside the table
template <bool RGB>
FELICS_HDI int lane8_keep(int pv, uint32_t &out_of_range) {
    if (RGB) {
        out_of_range |= (uint32_t)pv + 255u > 510u ? 1u : 0u;
        return lane_min(lane_max(pv, -255), 255);
    }
    out_of_range |= (uint32_t)pv;
    return pv & 255;
}
template <bool RGB>
FELICS_HDI bool lane8_bad(uint32_t out_of_range) { return RGB ? out_of_range != 0 : out_of_range > 255u; }

// the 8-bit step as the plane walk takes it
template <bool RGB>
struct Lane8Step {
    Lane8Estimator est;
    uint32_t out_of_range;
    FELICS_HDI int pixel(LaneReader &br, uint32_t x, uint32_t y, int left, int left2, int above, int first_col2, int &rc) {
        return lane8_pixel(br, est, x, y, left, left2, above, first_col2, rc);
    }
    FELICS_HDI int keep(int pv) { return lane8_keep<RGB>(pv, out_of_range); }
    FELICS_HDI bool bad() const { return lane8_bad<RGB>(out_of_range); }
};

// ---- the 16-bit step ----

// The 16-bit step: the in-range code for every lane; the lanes whose pixel is out of range then take the estimator path together -- the
// context's row of the lane's hashed table (felics_lanetable.h: fifteen 32-bit counters and the tag word, four 16-byte accesses; `rows`
// rows in epoch `epoch`, a row of another epoch is empty), get_k, the Rice code, the update.  A table found full is FELICS_E_IO (the
// sizing rule does not let it happen) and nothing is stored.  lo_ok .. hi_ok: Y 0 .. 65535, Co / Cg -65535 .. 65535.
struct Lane16Step {
    LaneQuad *tab;
    uint32_t rows, epoch;
    int lo_ok, hi_ok;
    uint32_t out_of_range;
    FELICS_HDI int pixel(LaneReader &br, uint32_t x, uint32_t y, int left, int left2, int above, int first_col2, int &rc) {
        const LaneNeighbours nb = lane_neighbours(x, y, left, left2, above, first_col2);
        const uint32_t ctx = nb.ctx;  // <= 131 070
        br.refill();  // >= 33 valid bits: both kinds of code are read off the top 32 of them where they fit
        const uint32_t top = (uint32_t)(br.acc >> 32);
        const bool in_range = (top >> 31) != 0;
        const LaneInRange in = lane_in_range(top, ctx, nb.lo);
        int pv = in.pv;
        uint32_t nbits = in.bits;  // <= 18
        if (!in_range) {
            const bool above_flag = ((top >> 30) & 1u) != 0;
            LaneQuad q0, q1, q2, q3;
            q0 = q1 = q2 = q3 = LaneQuad{0, 0, 0, 0};
            bool found;
            LaneQuad *const t = tab;
            const uint32_t at = dec16l_find(ctx, rows, epoch,
                                            [&](uint32_t rw) {
                                                const LaneQuad *p = t + (uint64_t)rw * 4u;
                                                q0 = p[0];
                                                q1 = p[1];
                                                q2 = p[2];
                                                q3 = p[3];
                                                return q3.w;
                                            },
                                            found);
            const bool full = at == DEC16L_FULL;
            if (full && rc == FELICS_OK) rc = FELICS_E_IO;  // (internal: the sizing rule admits every context a plane can use)
            uint32_t S[15] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w, q2.x, q2.y, q2.z, q2.w, q3.x, q3.y, q3.z};
            if (!found) {
#pragma unroll
                for (uint32_t kk = 0; kk < 15; kk++) S[kk] = 0;
            }
            // get_k: smallest counter, ties to the largest k (parameter_selection.rs:71-85)
            uint32_t key = 0xFFFFFFFFu;
#pragma unroll
            for (uint32_t kk = 0; kk < 15; kk++) key = lane_min(key, (S[kk] << 4) | (15u - kk));
            const uint32_t k = 15u - (key & 15u);
            const LaneRice rice = lane_rice_short(top, k);
            uint32_t e;
            if (rice.fits) {
                e = rice.e;
                nbits = rice.nbits;  // <= 32 < the valid bits
                if (e > 262144u) {
                    if (rc == FELICS_OK) rc = FELICS_E_INVALID_VALUE;
                    e = 0;
                }
            } else {
                e = lane_rice_long(br, k, 262144u, rc);
                nbits = 0;
            }
            const uint32_t hsh = lane_estimator_update(S, e);
            if (!full) {
                LaneQuad *p = t + (uint64_t)at * 4u;
                p[0] = LaneQuad{S[0] >> hsh, S[1] >> hsh, S[2] >> hsh, S[3] >> hsh};
                p[1] = LaneQuad{S[4] >> hsh, S[5] >> hsh, S[6] >> hsh, S[7] >> hsh};
                p[2] = LaneQuad{S[8] >> hsh, S[9] >> hsh, S[10] >> hsh, S[11] >> hsh};
                p[3] = LaneQuad{S[12] >> hsh, S[13] >> hsh, S[14] >> hsh, dec16l_tag(epoch, ctx)};
            }
            pv = above_flag ? nb.hi + (int)e + 1 : nb.lo - (int)e - 1;
        }
        br.acc <<= nbits;
        br.navail -= nbits;
        return pv;
    }
    // try_into::<u16>() (Co / Cg: the estimator's context bound) would fail on anything outside lo_ok .. hi_ok: remembered and
    // reported at the end of the row; the sample is cut into the range so that a failed stream's contexts stay below 131 071
    FELICS_HDI int keep(int pv) {
        out_of_range |= (uint32_t)pv - (uint32_t)lo_ok > (uint32_t)(hi_ok - lo_ok) ? 1u : 0u;  // (the raw samples are any 32 bits)
        return lane_min(lane_max(pv, lo_ok), hi_ok);
    }
    FELICS_HDI bool bad() const { return out_of_range != 0; }
};

// ---- the walks ----

// One whole plane of W x H samples (W >= 8, H >= 1) behind its two raw samples p0, p1 (compression.rs:166-167), row y at
// out + y * (PITCHED ? pitch : W).  On the GPU (x, y) and everything derived from them alone is wave-uniform: the streams of a wave
// have one shape.  The row above is read back from the lane's own output, four samples at a time and a group ahead; the four samples
// of a group are stored at once.  PITCHED: no load or store leaves [0, W) of its row -- the samples between a row's end and the pitch
// are somebody else's (a neighbouring cell of a mosaic) -- so a row's short last group is read sample by sample; dense, a group's load
// may run into the next row of the same plane (W >= 8: at most three samples, never past the plane's last row, which nothing reads).
// rc takes the first error; a lane that has failed keeps walking on zeros with its samples cut into range.
template <typename ST, bool PITCHED, typename Step>
FELICS_HDI void lane_walk_plane(LaneReader &br, Step &step, ST *out, int64_t pitch, uint32_t W, uint32_t H, int32_t p0, int32_t p1, int &rc) {
    int left = 0, left2 = 0;
    Four<ST> up4, up4_next, out4;
    up4.clear();
    up4_next.clear();
    out4.clear();
    step.out_of_range = 0;
    int first_col2 = 0;
    for (uint32_t y = 0; y < H; y++) {
        ST *row = out + (uint64_t)y * W;  // this row of the stream's plane, and the one above it
        const ST *prow = row - W;
        if constexpr (PITCHED) {
            row = out + (int64_t)y * pitch;
            prow = row - pitch;
        }
        if (y > 0) {
            up4.load(prow);                   // row above, samples 0 .. 3 (later groups are asked for four samples ahead)
            if (4 < W) up4_next.load(prow + 4);
            // second neighbour of a row's first pixel (misc.rs:14-23): two rows up, or above-right in row 1
            if constexpr (PITCHED)
                first_col2 = y >= 2 ? (int)prow[-pitch] : up4.get(1);  // (W >= 8)
            else
                first_col2 = y >= 2 ? (int)prow[-(int64_t)W] : (W > 1 ? up4.get(1) : 0);
        }
        for (uint32_t x = 0; x < W; x++) {
            const uint32_t xs = x & 3u;
            if (xs == 0 && y > 0 && x != 0) {
                up4 = up4_next;
                if constexpr (PITCHED) {  // (wave-uniform: x and W) the row's last group may be short: sample by sample, never past W
                    if (x + 8 <= W) up4_next.load(prow + x + 4);
                    else if (x + 4 < W) up4_next.load_n(prow + x + 4, W - (x + 4));
                } else if (x + 4 < W) {
                    up4_next.load(prow + x + 4);
                }
            }
            int pv;
            if (y == 0 && x < 2) pv = x == 0 ? p0 : p1;
            else pv = step.pixel(br, x, y, left, left2, up4.get(xs), first_col2, rc);
            pv = step.keep(pv);
            out4.set(xs, pv);
            left2 = left;
            left = pv;
            if (xs == 3u) {  // four samples complete: one (unaligned) store to the stream's plane
                out4.store(row + (x - 3u));
                out4.clear();
            } else if (x + 1 == W) {  // the last one to three samples of a row
                for (uint32_t j = 0; j <= xs; j++) row[(x - xs) + j] = (ST)out4.get(j);
                out4.clear();
            }
        }
        if (rc == FELICS_OK) rc = br.failed() ? FELICS_E_IO : (step.bad() ? FELICS_E_INVALID_VALUE : FELICS_OK);
    }
}

// Pixels [p0, pend) of an 8-bit plane from a checkpoint (k_decode8_seg_lanes): the reader stands on the checkpoint's
// bit offset, the estimator holds its state, `win` is its window -- sample t is pixel p0 - 2 W + t -- and raw0, raw1 are the plane's
// two raw samples (segment 0 only).  W >= 8, p0 < pend <= W H.
//   * the row above: pixel q >= p0 is read back from the lane's own output plane (it wrote it itself), q < p0 from the window at
//     2 W - (p0 - q) -- the pixels in front of p0 are another wave's, which may not have written them yet: the output is NEVER read
//     below p0.  A group of four that straddles p0, and a row's short last group, are assembled sample by sample: no load runs past
//     sample W - 1 of a row, in the window or in the plane.  Window positions in front of the plane (p0 + t < 2 W) are never looked at;
//   * only pixels p0 .. pend - 1 are written: a first group with x0 & 3 != 0 is stored from x0 on, a last group that ends inside four
//     samples is flushed sample by sample.
// rc as in lane_walk_plane, without the last look at out_of_range, which is returned: the caller's, with the reader's state and the
// end check.
template <bool RGB, typename ST>
FELICS_HDI uint32_t lane8_walk_segment(LaneReader &br, const Lane8Estimator &est, ST *out, const ST *win, uint32_t W, uint64_t p0, uint64_t pend,
                                       int32_t raw0, int32_t raw1, int &rc) {
    // pixel q of the plane as this lane may read it: its own output from p0 on, the window in front (p0 - 2 W <= q: the callers' business)
    auto rd = [&](uint64_t q) -> int { return q >= p0 ? (int)out[q] : (int)win[2ull * W - (p0 - q)]; };
    // (x, y) and everything derived from them alone is wave-uniform
    uint32_t x = (uint32_t)(p0 % W), y = (uint32_t)(p0 / W);
    // row y - 1 from column xg (a multiple of four below W) on: four samples, or the row's last one to three
    auto load_up = [&](uint32_t xg) {
        Four<ST> f;
        const uint64_t q0 = (uint64_t)(y - 1) * W + xg;
        const uint32_t cnt = lane_min(4u, W - xg);
        if (cnt == 4u && q0 >= p0) {
            f.load(out + q0);
        } else if (cnt == 4u && q0 + 4u <= p0) {
            f.load(win + (2ull * W - (p0 - q0)));
        } else {
            f.clear();
            for (uint32_t k = 0; k < cnt; k++) f.set(k, rd(q0 + k));
        }
        return f;
    };
    int left = x >= 1 ? (int)win[2ull * W - 1] : 0, left2 = x >= 2 ? (int)win[2ull * W - 2] : 0;
    Four<ST> up4, up4_next, out4;
    up4.clear();
    up4_next.clear();
    out4.clear();
    if (x != 0 && y > 0) {  // a start inside a row: the groups of the row above that the row's start would have asked for
        if ((x & 3u) == 0) {
            up4_next = load_up(x);  // (moved into up4 by the first pixel)
        } else {
            up4 = load_up(x & ~3u);
            if ((x & ~3u) + 4 < W) up4_next = load_up((x & ~3u) + 4);
        }
    }
    uint32_t gfirst = x & 3u;  // first sample of the current group that is this segment's to store
    uint32_t out_of_range = 0;
    int first_col2 = 0;
    for (uint64_t i = p0; i < pend; i++) {
        const uint32_t xs = x & 3u;
        if (x == 0 && y > 0) {
            up4 = load_up(0);  // row above, samples 0 .. 3 (later groups are asked for four samples ahead); W >= 8
            up4_next = load_up(4);
            // second neighbour of a row's first pixel (misc.rs:14-23): two rows up, or above-right in row 1
            first_col2 = y >= 2 ? rd((uint64_t)(y - 2) * W) : up4.get(1);
        } else if (xs == 0 && y > 0) {
            up4 = up4_next;
            if (x + 4 < W) up4_next = load_up(x + 4);
        }
        int pv;
        if (i < 2) pv = i == 0 ? raw0 : raw1;
        else pv = lane8_pixel(br, est, x, y, left, left2, up4.get(xs), first_col2, rc);  // (every window sample is checked: ctx in the table)
        pv = lane8_keep<RGB>(pv, out_of_range);
        out4.set(xs, pv);
        left2 = left;
        left = pv;
        const bool row_end = x + 1 == W;
        if (xs == 3u || row_end || i + 1 == pend) {  // a group is complete, or the row is, or the segment
            ST *grp = out + (i - xs);                 // the group's first sample; samples gfirst .. xs of it are this segment's
            if (xs == 3u && gfirst == 0) {
                out4.store(grp);  // four samples: one (unaligned) store to the lane's plane
            } else {
                for (uint32_t k = gfirst; k <= xs; k++) grp[k] = (ST)out4.get(k);
            }
            out4.clear();
            gfirst = 0;
        }
        if (row_end) {
            if (rc == FELICS_OK) rc = br.failed() ? FELICS_E_IO : (lane8_bad<RGB>(out_of_range) ? FELICS_E_INVALID_VALUE : FELICS_OK);
            x = 0;
            y++;
        } else {
            x++;
        }
    }
    return out_of_range;
}

}  // namespace felics
