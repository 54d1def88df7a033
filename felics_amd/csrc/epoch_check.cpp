// epoch_check.cpp -- host check of felics_epochs.h, the rules by which a context hands out the epochs that tag its look-back status
// words (run_lane), the dense estimator tables of k_decode16 and the hashed ones of k_decode16_lanes: the very functions the host code
// compiles are walked from the value a fresh buffer starts with (0), and from start values close to every wrap (a fresh buffer with
// such a start value is what the FELICS_TEST_*_EPOCH switches create), with a model of the tagged buffer beside them:
//   - between two clears no tag value is handed out twice (look-back: the low 18 bits; lane form: epoch0 .. epoch0 + 2 within
//     1 .. DEC16L_EPOCH_MAX; wave form: 32 bits -- too many for a set, so the model asks for what implies it: since the last clear
//     every epoch0 lies above the last epoch handed out, and epoch0 + 2 does not run over);
//   - tag 0 is only handed out directly behind a clear (look-back), or never (the decoders);
//   - a fresh buffer's first epochs are 1, 1 .. 3 and 1 .. 3.
// The ordinary build walks every rule over its whole period and the wrap (2^32 steps for the look-back's counter); under
// AddressSanitizer (make asan) the two 32-bit walks keep to 2^27 steps on either side of each wrap.  The look-back rule as it stood
// before it was left to run over -- back to 1 at 0x03FFFFFF, without a clear -- is walked too and MUST be reported: the check of the
// check.  tests/test_epochs.py runs both builds; exit status 0 and a last line "all checks held" = every check held, otherwise the
// first failure is named.
#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <vector>

#include "felics_epochs.h"

using namespace felics;

#if defined(__SANITIZE_ADDRESS__)
#define EPOCH_CHECK_WINDOWS 1
#elif defined(__has_feature)
#if __has_feature(address_sanitizer)
#define EPOCH_CHECK_WINDOWS 1
#endif
#endif
#ifndef EPOCH_CHECK_WINDOWS
#define EPOCH_CHECK_WINDOWS 0
#endif

#define FAIL(...)                 \
    do {                          \
        printf("FAILED: ");       \
        printf(__VA_ARGS__);      \
        printf("\n");             \
        exit(1);                  \
    } while (0)

static std::string text(const char *fmt, unsigned long long a, unsigned long long b = 0, unsigned long long c = 0, unsigned long long d = 0) {
    char buf[256];
    snprintf(buf, sizeof buf, fmt, a, b, c, d);
    return buf;
}

// A buffer of words tagged with `bits` bits: which tags are in use since the last clear, and the epoch that first used each.
struct TagModel {
    uint32_t mask;
    std::vector<uint64_t> slot;  // generation << 32 | epoch; the current generation: in use
    uint64_t gen = 1;
    explicit TagModel(uint32_t bits) : mask((1u << bits) - 1u), slot((size_t)1 << bits, 0u) {}
    void clear() { gen++; }
    bool used(uint32_t epoch) const { return (slot[epoch & mask] >> 32) == gen; }
    uint32_t first(uint32_t epoch) const { return (uint32_t)slot[epoch & mask]; }
    void use(uint32_t epoch) { slot[epoch & mask] = (gen << 32) | epoch; }
};

// ---- the look-back's rule: `steps` sub-batches on a fresh (zeroed) buffer whose lane starts at `last`.  "" or the first violation.
template <typename Rule>
static std::string walk_lookback(Rule next, uint32_t last, uint64_t steps, uint64_t *clears = nullptr) {
    TagModel m(LOOKBACK_EPOCH_BITS);
    for (uint64_t step = 1; step <= steps; step++) {
        const EpochStep s = next(last);
        if (s.clear) {
            m.clear();
            if (clears) ++*clears;
        }
        const uint32_t tag = s.epoch & LOOKBACK_EPOCH_MASK;
        if (tag == 0 && !s.clear) return text("step %llu epoch 0x%llx masked 0x0 handed out without a clear: a zeroed word would read as this epoch's", step, s.epoch);
        if (m.used(s.epoch))
            return text("step %llu epoch 0x%llx masked 0x%llx reused, first used at epoch 0x%llx, no clear between", step, s.epoch, tag, m.first(s.epoch));
        m.use(s.epoch);
        last = s.epoch;
    }
    return "";
}

// the two lines of run_lane before the counter was left to run over: `if (++l.epoch >= 0x03FFFFFFu) l.epoch = 1;` and the clear on
// eighteen zero bits
static EpochStep lookback_epoch_next_before(uint32_t last) {
    uint32_t epoch = last + 1u;
    if (epoch >= 0x03FFFFFFu) epoch = 1u;
    return EpochStep{epoch, (epoch & 0x3FFFFu) == 0u};
}

// ---- the lane form's rule: three tags per launch, each within 1 .. DEC16L_EPOCH_MAX
static std::string walk_lanes(uint32_t last, uint64_t steps, uint64_t *clears, uint64_t *first_clear_at) {
    TagModel m(15);
    for (uint64_t step = 1; step <= steps; step++) {
        const EpochStep s = dec16_lanes_epoch_next(last);
        if (s.clear) {
            m.clear();
            if (!*clears) *first_clear_at = step;
            ++*clears;
        }
        if (s.epoch < 1u || s.epoch > DEC16L_EPOCH_MAX - 2u)
            return text("launch %llu: epochs 0x%llx .. 0x%llx leave 1 .. DEC16L_EPOCH_MAX", step, s.epoch, (unsigned long long)s.epoch + 2);
        for (uint32_t e = s.epoch; e < s.epoch + 3u; e++) {
            if (m.used(e)) return text("launch %llu epoch 0x%llx reused, first used at epoch 0x%llx, no clear between", step, e, m.first(e));
            m.use(e);
        }
        last = s.epoch + 2u;
    }
    return "";
}

// ---- the wave form's rule: since the last clear every epoch0 above the last epoch handed out, epoch0 + 2 within 32 bits, never 0
static std::string walk_wave(uint32_t last, uint64_t steps, uint64_t *clears) {
    uint64_t high = last;  // the highest epoch in use in the buffer (a fresh buffer: none, and `last` is where its context starts)
    for (uint64_t step = 1; step <= steps; step++) {
        const EpochStep s = dec16_epoch_next(last);
        if (s.clear) {
            high = 0;
            ++*clears;
        }
        if (s.epoch == 0u) return text("pass %llu: epoch 0 handed out: a zeroed row would read as this epoch's", step);
        if ((uint64_t)s.epoch + 2u > 0xFFFFFFFFull) return text("pass %llu: epochs from 0x%llx run over 32 bits", step, s.epoch);
        if (s.epoch <= high) return text("pass %llu epoch 0x%llx not above 0x%llx, handed out since the last clear", step, s.epoch, high);
        high = last = s.epoch + 2u;
    }
    return "";
}

int main() {
    // what a fresh buffer hands out first
    if (lookback_epoch_next(0).epoch != 1u || lookback_epoch_next(0).clear) FAIL("look-back: a fresh lane does not start with epoch 1 and no clear");
    if (dec16_epoch_next(0).epoch != 1u || dec16_epoch_next(0).clear) FAIL("wave form: a fresh table does not start with epochs 1 .. 3 and no clear");
    if (dec16_lanes_epoch_next(0).epoch != 1u || dec16_lanes_epoch_next(0).clear) FAIL("lane form: a fresh table does not start with epochs 1 .. 3 and no clear");
    printf("fresh buffers: first epochs 1, 1 .. 3, 1 .. 3\n");

    // the rule as it stood: the reuse behind 0x03FFFFFF must be found
    {
        const std::string bad = walk_lookback(lookback_epoch_next_before, 0, 0x04000000ull + (1u << 19));
        if (bad.empty()) FAIL("look-back, the rule before the fix: the walk did not notice the reuse behind 0x03FFFFFF");
        printf("look-back, the rule before the fix (expected to fail): %s\n", bad.c_str());
        if (bad.find("epoch 0x1 masked 0x1 reused, first used at epoch 0x3fc0001") == std::string::npos)
            FAIL("look-back, the rule before the fix: another failure than the reuse of epoch 0x1");
    }

    // the look-back rule: the counter's whole period and the wrap behind it; start values around both wraps
    {
        uint64_t clears = 0;
        std::string bad;
        uint64_t walked = 0;
        if (EPOCH_CHECK_WINDOWS) {
            for (uint32_t start : {0u, 0x3FFFFu - (1u << 17), 0xFFFFFFFFu - (1u << 27)}) {
                if (!(bad = walk_lookback(lookback_epoch_next, start, 1ull << 28, &clears)).empty()) FAIL("look-back from 0x%x: %s", start, bad.c_str());
                walked += 1ull << 28;
            }
        } else {
            walked = (1ull << 32) + (1ull << 20);
            if (!(bad = walk_lookback(lookback_epoch_next, 0, walked, &clears)).empty()) FAIL("look-back: %s", bad.c_str());
            if (clears != (1ull << 14) + 4) FAIL("look-back: %llu clears in 2^32 + 2^20 sub-batches, not one every 2^18", (unsigned long long)clears);
        }
        for (uint32_t below : {1u, 2u, 5u, 100u})
            for (uint32_t wrap : {0x3FFFFu, 0x03FFFFFEu, 0xFFFFFFFFu})
                if (!(bad = walk_lookback(lookback_epoch_next, wrap - below, 1u << 20)).empty()) FAIL("look-back from 0x%x: %s", wrap - below, bad.c_str());
        printf("look-back: %llu sub-batches walked, %llu clears, no tag of 18 bits handed out twice between two of them\n", (unsigned long long)walked,
               (unsigned long long)clears);
    }

    // the lane form: many periods from a fresh table, and from start values up to the last
    {
        uint64_t clears = 0, first_clear = 0;
        std::string bad = walk_lanes(0, 1u << 20, &clears, &first_clear);
        if (!bad.empty()) FAIL("lane form: %s", bad.c_str());
        if (first_clear != 10923 || clears != (1u << 20) / 10922) FAIL("lane form: first clear on launch %llu, %llu clears in 2^20 launches", (unsigned long long)first_clear, (unsigned long long)clears);
        for (uint32_t start = 0; start <= DEC16L_EPOCH_MAX; start += start + 64u < DEC16L_EPOCH_MAX ? 61u : 1u) {  // (every residue of 3; the last 64 all)
            uint64_t c = 0, f = 0;
            if (!(bad = walk_lanes(start, 11000, &c, &f)).empty()) FAIL("lane form from 0x%x: %s", start, bad.c_str());
        }
        printf("lane form: first clear on launch %llu, one every 10922 launches, start values 0 .. 0x%x walked over their wraps\n",
               (unsigned long long)first_clear, DEC16L_EPOCH_MAX);
    }

    // the wave form: the whole period and the wrap; start values around the wrap
    {
        uint64_t clears = 0, walked = 0;
        std::string bad;
        if (EPOCH_CHECK_WINDOWS) {
            for (uint32_t start : {0u, 0xFFFFFFF0u - 3u * (1u << 27)}) {
                if (!(bad = walk_wave(start, 1ull << 28, &clears)).empty()) FAIL("wave form from 0x%x: %s", start, bad.c_str());
                walked += 1ull << 28;
            }
            if (clears != 1) FAIL("wave form: %llu clears around the wrap", (unsigned long long)clears);
        } else {
            walked = (1ull << 32) / 3 + (1u << 20);
            if (!(bad = walk_wave(0, walked, &clears)).empty()) FAIL("wave form: %s", bad.c_str());
            if (clears != 1) FAIL("wave form: %llu clears in one period and a little", (unsigned long long)clears);
        }
        for (uint32_t start = 0xFFFFFFFFu - 64u; start >= 0xFFFFFFFFu - 64u; start++) {  // (until it runs over)
            uint64_t c = 0;
            if (!(bad = walk_wave(start, 1u << 16, &c)).empty()) FAIL("wave form from 0x%x: %s", start, bad.c_str());
            if (c != 1) FAIL("wave form from 0x%x: %llu clears", start, (unsigned long long)c);
        }
        printf("wave form: %llu passes walked, %llu clear, epochs rising between clears, none 0, none over 32 bits\n", (unsigned long long)walked,
               (unsigned long long)clears);
    }
    printf("all checks held\n");
    return 0;
}
