// felics_hostdec.h -- the host decoder's parts, shared by felics_decode.cpp (whole streams) and felics_index.cpp (a stream
// segment by segment, felics.h "restart index"): the bit reader, the estimator and the loop of decompress_channel over a range
// of a plane's pixels.  Host only, header only.
#ifndef FELICS_HOSTDEC_H
#define FELICS_HOSTDEC_H

#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/felics.h"

namespace felics_hostdec {

// MSB-first bit reader over a byte range (bitstream-io BitReader<_, BigEndian> semantics).
class BitReader {
  public:
    BitReader(const uint8_t *p, size_t n) : begin_(p), p_(p), end_(p + n) {}
    // positioned `bit` bits behind p (bit <= 8 n: the caller's check)
    BitReader(const uint8_t *p, size_t n, uint64_t bit) : begin_(p), p_(p + (size_t)(bit >> 3)), end_(p + n) { bits((unsigned)(bit & 7u)); }

    bool failed() const { return failed_; }
    // bits consumed since the range's first byte
    uint64_t pos() const { return (uint64_t)(p_ - begin_) * 8u - have_; }

    uint32_t bit() {
        if (have_ == 0 && !refill()) return 0;
        have_--;
        return (uint32_t)(window_ >> have_) & 1u;
    }

    // up to 32 bits, most significant first
    uint32_t bits(unsigned n) {
        uint64_t v = 0;
        while (n) {
            if (have_ == 0 && !refill()) return 0;
            const unsigned take = n < have_ ? n : have_;  // <= 32
            have_ -= take;
            v = (v << take) | ((window_ >> have_) & ((1ull << take) - 1ull));
            n -= take;
        }
        return (uint32_t)v;
    }

    // read_unary0: number of one-bits before the first zero-bit
    uint32_t unary0() {
        uint32_t q = 0;
        for (;;) {
            if (have_ == 0 && !refill()) return q;
            // count leading ones of the `have_` unread bits
            uint64_t unread = window_ << (64 - have_);
            unsigned ones = unread == ~0ull ? 64 : (unsigned)__builtin_clzll(~unread);
            if (ones >= have_) {
                q += have_;
                have_ = 0;
                continue;
            }
            q += ones;
            have_ -= ones + 1;
            return q;
        }
    }

  private:
    bool refill() {
        if (p_ == end_) {
            failed_ = true;
            return false;
        }
        window_ = 0;
        have_ = 0;
        while (p_ != end_ && have_ <= 48) {
            window_ = (window_ << 8) | *p_++;
            have_ += 8;
        }
        return true;
    }

    const uint8_t *begin_, *p_, *end_;
    uint64_t window_ = 0;  // low `have_` bits are unread, MSB of them first
    unsigned have_ = 0;
    bool failed_ = false;
};

struct Options {  // traits.rs:25-43
    uint32_t max_context;
    unsigned nk;  // k in 0..nk-1
};

// KEstimator (parameter_selection.rs:24-85) with a flat table.
class Estimator {
  public:
    Estimator(const Options &o) : nk_(o.nk), table_((size_t)(o.max_context + 1) * o.nk, 0u) {}

    unsigned get_k(uint32_t ctx) const {
        const uint32_t *row = &table_[(size_t)ctx * nk_];
        uint32_t best = row[0];
        unsigned k = 0;
        for (unsigned i = 1; i < nk_; i++)
            if (row[i] <= best) {  // ties: last wins
                best = row[i];
                k = i;
            }
        return k;
    }

    void update(uint32_t ctx, uint32_t v) {
        uint32_t *row = &table_[(size_t)ctx * nk_];
        uint32_t mn = 0xFFFFFFFFu;
        for (unsigned i = 0; i < nk_; i++) {
            row[i] += (v >> i) + 1 + i;
            if (row[i] < mn) mn = row[i];
        }
        if (mn > 1024)
            for (unsigned i = 0; i < nk_; i++) row[i] >>= 1;
    }

    // the counters of a context, to save and to restore a checkpoint
    uint32_t *row(uint32_t ctx) { return &table_[(size_t)ctx * nk_]; }

  private:
    unsigned nk_;
    std::vector<uint32_t> table_;
};

// The pixel loop of decompress_channel (compression.rs:169-246) over the pixels [i0, i1) of a plane, 2 <= i0: `out` is the plane,
// and the samples in front of i0 that the neighbour rule reaches (at most 2 W of them) are in it.  last_event (optional):
// [ctx] = the latest pixel of that context that was coded out of range.
inline int decode_span(BitReader &br, uint32_t W, const Options &opt, Estimator &est, int32_t *out, size_t i0, size_t i1,
                       uint32_t *last_event) {
    uint32_t x = (uint32_t)(i0 % W), y = (uint32_t)(i0 / W);
    for (size_t i = i0; i < i1; i++) {
        size_t a, b;  // misc.rs:6-24
        if (x > 0 && y > 0) {
            a = i - 1;
            b = i - W;
        } else if (y == 0) {
            a = i - 1;
            b = i - 2;
        } else if (y >= 2) {
            a = i - W;
            b = i - 2 * (size_t)W;
        } else {
            a = i - W;
            b = i - W + 1;
        }
        const int64_t v1 = out[a], v2 = out[b];
        const int64_t hi = v1 > v2 ? v1 : v2, lo = v1 < v2 ? v1 : v2;
        if (hi - lo > (int64_t)opt.max_context) return FELICS_E_INVALID_VALUE;
        const uint32_t ctx = (uint32_t)(hi - lo);
        int64_t pv;
        if (br.bit()) {  // in range: phased-in code of p - L in [0, ctx]
            const uint32_t n = ctx + 1;
            const unsigned m = 31u - (unsigned)__builtin_clz(n);
            const uint32_t right_p = (2u << m) - n, left_p = n - (1u << m);
            uint32_t r = br.bits(m);
            if (r >= right_p) r = (r - right_p) * 2 + right_p + br.bit();
            pv = lo + (int64_t)(((uint64_t)r + left_p) % n);  // rotate_left, phase_in_coding.rs:50-52
        } else {
            const bool above = br.bit() != 0;
            const unsigned k = est.get_k(ctx);
            const uint64_t q = br.unary0();
            const uint64_t e = (q << k) + br.bits(k);
            if (br.failed()) return FELICS_E_IO;
            if (e > 0xFFFFFFFFull) return FELICS_E_VALUE_OVERFLOW;
            est.update(ctx, (uint32_t)e);
            if (last_event) last_event[ctx] = (uint32_t)i;
            if (e > 0x7FFFFFFFull) return FELICS_E_INVALID_VALUE;
            pv = above ? hi + (int64_t)e + 1 : lo - (int64_t)e - 1;
        }
        if (br.failed()) return FELICS_E_IO;
        if (pv > INT32_MAX || pv < INT32_MIN) return FELICS_E_VALUE_OVERFLOW;
        out[i] = (int32_t)pv;
        if (++x == W) {
            x = 0;
            y++;
        }
    }
    return FELICS_OK;
}

}  // namespace felics_hostdec

#endif
