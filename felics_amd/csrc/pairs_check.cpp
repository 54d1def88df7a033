// pairs_check -- host check of felics_pairs.h: the pair builder k_pack_t's 8-bit instantiations compile, against the scalar formulas
// (the neighbour rule and classification of compression.rs:124-145, the phased-in code of phase_in_coding.rs:23-84 as felics_codes.h's
// phase_in has it), for EVERY (p, left, up) in 256^3, in either half of the pair and with two different partners in the other half.
// Then the byte selection: the pairs of a 16-sample group as the kernel walks it -- the left neighbour across a dword boundary, and
// the sample in front of the group -- against the samples picked one by one.  Host code only (tests/test_pack_pairs.py runs it, and
// the sanitizer build of the Makefile).  Prints one line and returns 0 if everything agrees.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "felics_pairs.h"

using namespace felics;

namespace {

struct Ref {
    uint32_t val, above, in_range, code_in, len_in;  // above / in_range: 0 or 1; code_in, len_in: only where in_range
};

// phase_in (felics_codes.h), with the host's clz
void phase_in(uint32_t n, uint32_t v, uint32_t &bits, uint32_t &nbits) {
    const uint32_t m = 31u - (uint32_t)__builtin_clz(n);
    const uint32_t right_p = (2u << m) - n;
    uint32_t r = v + (1u << m);
    if (r >= n) r -= n;
    if (r < right_p) {
        bits = r;
        nbits = m;
    } else {
        bits = r + right_p;
        nbits = m + 1;
    }
}

Ref ref_pixel(uint32_t p, uint32_t a, uint32_t b) {
    const uint32_t L = a < b ? a : b, H = a < b ? b : a;
    Ref r{0, 0, 0, 0, 0};
    if (p < L) {
        r.val = L - p - 1;
    } else if (p > H) {
        r.val = p - H - 1;
        r.above = 1;
    } else {
        r.val = p - L;
        r.in_range = 1;
        uint32_t bits, nbits;
        phase_in(H - L + 1, r.val, bits, nbits);
        r.code_in = (1u << nbits) | bits;
        r.len_in = nbits + 1;
    }
    return r;
}

uint64_t failures = 0;
void fail(const char *what, uint32_t p, uint32_t l, uint32_t u, uint32_t e, uint32_t got, uint32_t want) {
    if (failures++ < 20) fprintf(stderr, "pairs_check: %s of (p %u, left %u, up %u) in half %u: %#x, expected %#x\n", what, p, l, u, e, got, want);
}

// one pixel's five outputs, out of the pair's
struct Half {
    uint32_t val, above, in_range, code_in, len_in;
};
Half half_of(const PairCodes &pc, uint32_t e) {
    return Half{pair_value(pc.val, e), pair_mask(pc.above, e), pair_mask(pc.in_range, e), pair_value(pc.code_in, e), pair_value(pc.len_in, e)};
}

uint32_t put(uint32_t mine, uint32_t other, uint32_t e) { return e ? (mine << 16) | other : (other << 16) | mine; }

void check_triple(uint32_t p, uint32_t l, uint32_t u, uint32_t e, uint32_t &rng) {
    rng = rng * 1664525u + 1013904223u;
    const uint32_t q0 = rng >> 24, l0 = (rng >> 16) & 0xFFu, u0 = (rng >> 8) & 0xFFu;  // an arbitrary partner
    const uint32_t q1 = 255u - p, l1 = u, u1 = 255u - l0;                              // and another
    const PairCodes a = pair_codes(put(p, q0, e), put(l, l0, e), put(u, u0, e));
    const PairCodes b = pair_codes(put(p, q1, e), put(l, l1, e), put(u, u1, e));
    const Half h = half_of(a, e), g = half_of(b, e);
    const Ref r = ref_pixel(p, l, u);
    if (h.val != r.val) fail("val", p, l, u, e, h.val, r.val);
    if (h.above != (r.above ? ~0u : 0u)) fail("above", p, l, u, e, h.above, r.above ? ~0u : 0u);
    if (h.in_range != (r.in_range ? ~0u : 0u)) fail("in_range", p, l, u, e, h.in_range, r.in_range ? ~0u : 0u);
    if (r.in_range) {
        if (h.code_in != r.code_in) fail("code_in", p, l, u, e, h.code_in, r.code_in);
        if (h.len_in != r.len_in) fail("len_in", p, l, u, e, h.len_in, r.len_in);
    }
    // the other half never reaches this one: garbage included, the half is a function of its own triple
    if (memcmp(&h, &g, sizeof h) != 0) fail("partner dependence (val)", p, l, u, e, h.val ^ g.val, 0);
    // and the partner's own half is right beside it
    const Half o = half_of(a, e ^ 1u);
    const Ref ro = ref_pixel(q0, l0, u0);
    if (o.val != ro.val || (o.in_range != 0) != (ro.in_range != 0) || (ro.in_range && (o.code_in != ro.code_in || o.len_in != ro.len_in)))
        fail("partner", q0, l0, u0, e ^ 1u, o.val, ro.val);
}

// a group of sixteen samples walked as the kernel walks it: four dwords, two pairs each
void check_group(const uint8_t (&cur)[16], const uint8_t (&up)[16], uint8_t before) {
    uint32_t cw[4], uw[4];
    memcpy(cw, cur, 16);
    memcpy(uw, up, 16);
    for (uint32_t w = 0; w < 4; w++) {
        for (uint32_t h = 0; h < 2; h++) {
            const uint32_t pp = pair_samples(cw[w], h), uu = pair_samples(uw[w], h);
            const uint32_t ll = (w == 0 && h == 0) ? pair_lefts_first(before, cw[0]) : pair_lefts(w ? cw[w - 1] : 0u, cw[w], h);
            const PairCodes pc = pair_codes(pp, ll, uu);
            for (uint32_t e = 0; e < 2; e++) {
                const uint32_t j = 4 * w + 2 * h + e;
                const uint32_t left = j ? cur[j - 1] : before;
                if (pair_value(pp, e) != cur[j]) fail("selected sample", cur[j], left, up[j], e, pair_value(pp, e), cur[j]);
                if (pair_value(ll, e) != left) fail("selected left neighbour", cur[j], left, up[j], e, pair_value(ll, e), left);
                if (pair_value(uu, e) != up[j]) fail("selected sample above", cur[j], left, up[j], e, pair_value(uu, e), up[j]);
                const Ref r = ref_pixel(cur[j], left, up[j]);
                const Half hf = half_of(pc, e);
                if (hf.val != r.val || (hf.in_range != 0) != (r.in_range != 0) || (hf.above != 0) != (r.above != 0) ||
                    (r.in_range && (hf.code_in != r.code_in || hf.len_in != r.len_in)))
                    fail("group pixel", cur[j], left, up[j], e, hf.val, r.val);
            }
        }
    }
}

}  // namespace

int main() {
    uint32_t rng = 12345u;
    uint64_t triples = 0;
    for (uint32_t p = 0; p < 256; p++)
        for (uint32_t l = 0; l < 256; l++)
            for (uint32_t u = 0; u < 256; u++) {
                check_triple(p, l, u, 0, rng);
                check_triple(p, l, u, 1, rng);
                triples++;
            }
    // byte selection: every value in every position beside all-ones and all-zeros neighbours, then random groups
    uint64_t groups = 0;
    for (uint32_t pos = 0; pos < 17; pos++)
        for (uint32_t v = 0; v < 256; v++)
            for (uint32_t fill = 0; fill < 2; fill++) {
                uint8_t cur[16], up[16], before = fill ? 0xFF : 0;
                memset(cur, fill ? 0xFF : 0, 16);
                memset(up, fill ? 0 : 0xFF, 16);
                if (pos < 16) cur[pos] = (uint8_t)v, up[15 - pos] = (uint8_t)v;
                else before = (uint8_t)v;
                check_group(cur, up, before);
                groups++;
            }
    for (uint32_t i = 0; i < 200000; i++) {
        uint8_t cur[16], up[16];
        for (uint32_t j = 0; j < 16; j++) {
            rng = rng * 1664525u + 1013904223u;
            cur[j] = (uint8_t)(rng >> 24);
            up[j] = (i & 1u) ? (uint8_t)(cur[j] + ((rng >> 16) & 7u) - 3u) : (uint8_t)(rng >> 12);  // (near the pixel: many in range)
        }
        rng = rng * 1664525u + 1013904223u;
        check_group(cur, up, (uint8_t)(rng >> 24));
        groups++;
    }
    if (failures) {
        fprintf(stderr, "pairs_check: %llu mismatches\n", (unsigned long long)failures);
        return 1;
    }
    printf("pairs_check: %llu triples in both halves with two partners each, %llu groups: ok\n", (unsigned long long)triples, (unsigned long long)groups);
    return 0;
}
