// frontout_check -- host check of felics_frontout.h: the pure pieces of k_front's back half, against their scalar definitions.
//   1. the output words: the pix word of two entries and the ev words of four (u8) or two (u16), for every class of (context, value,
//      pixel offset, above) in every position, beside every kind of partner, padding slots included (pix = 0xFFFF, not 0x1FFF);
//   2. the order predicate, for every pair of (context, offset) classes and padding on either side;
//   3. the layout of step 3 and steps 4 and 5 as the kernel runs them: tiles whose runs of 0 .. 33 events lie at every distance from
//      a pass boundary and from the end of the LDS image (inside a run, between runs, at the padding; 4096 - 16, 4096 and more slots
//      in use), laid out by the header's sums and slot bases, placed and written out four slots at a time -- against the slots
//      counted one by one; then the same tiles with two neighbouring events of a run exchanged: the check must see it.
// Host code only (tests/test_front_out.py runs it, and the sanitizer build of the Makefile).  Prints one line, returns 0 if all agree.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "felics_frontout.h"

using namespace felics;

namespace {

constexpr uint32_t WINDOW = 4096, PASS = 1024;  // slots of a window; slots the workgroup takes per pass (256 threads, four each)

uint64_t failures = 0;
void fail(const char *what, uint64_t a, uint64_t b, uint64_t got, uint64_t want) {
    if (failures++ < 20) fprintf(stderr, "frontout_check: %s (%#llx, %#llx): %#llx, expected %#llx\n", what, (unsigned long long)a, (unsigned long long)b,
                                 (unsigned long long)got, (unsigned long long)want);
}

uint32_t entry(uint32_t ctx, uint32_t val, uint32_t above, uint32_t off) { return ctx << 22 | val << 13 | above << 12 | off; }
// the scalar definitions
uint32_t ref_pix(uint32_t r) { return r == FRONTOUT_PAD ? 0xFFFFu : ((r >> 12) & 1u) << 12 | (r & 0xFFFu); }
uint32_t ref_val(uint32_t r) { return (r >> 13) & 0x1FFu; }
bool ref_bad(uint32_t r, uint32_t nxt) {
    if (r == FRONTOUT_PAD || nxt == FRONTOUT_PAD) return false;
    const uint32_t c0 = r >> 22, c1 = nxt >> 22, o0 = r & 0xFFFu, o1 = nxt & 0xFFFu;
    return c1 < c0 || (c1 == c0 && o1 <= o0);
}

const uint32_t OFFS[] = {0, 1, 2, 63, 64, 255, 256, 0x7FF, 0x800, 0xFFE, 0xFFF};
const uint32_t CTXS[] = {0, 1, 2, 127, 128, 254, 255, 256, 257, 510, 511};

// ---- 1. the output words
uint64_t check_words() {
    uint64_t n = 0;
    std::vector<uint32_t> partners = {FRONTOUT_PAD, 0u, entry(511, 511, 1, 0xFFF), entry(255, 255, 0, 0x800), entry(256, 1, 1, 1)};
    for (uint32_t ctx = 0; ctx < 512; ctx++)
        for (uint32_t val = 0; val < 512; val++)
            for (uint32_t off : OFFS)
                for (uint32_t above = 0; above < 2; above++) {
                    const uint32_t r = entry(ctx, val, above, off);
                    for (uint32_t q : partners) {
                        const uint32_t a = frontout_pix_pair(r, q), b = frontout_pix_pair(q, r);
                        if (a != (ref_pix(r) | ref_pix(q) << 16)) fail("pix word, low half", r, q, a, ref_pix(r) | ref_pix(q) << 16);
                        if (b != (ref_pix(q) | ref_pix(r) << 16)) fail("pix word, high half", q, r, b, ref_pix(q) | ref_pix(r) << 16);
                        const uint32_t e = frontout_ev_u16(r, q), f = frontout_ev_u16(q, r);
                        if ((e & 0xFFFFu) != ref_val(r)) fail("ev word (u16), low half", r, q, e, ref_val(r));
                        if ((f >> 16) != ref_val(r)) fail("ev word (u16), high half", q, r, f, ref_val(r));
                        if (q != FRONTOUT_PAD && (e >> 16) != ref_val(q)) fail("ev word (u16), partner", r, q, e, ref_val(q));
                        if (val < 256 && ctx < 256) {  // (u8 planes)
                            for (uint32_t pos = 0; pos < 4; pos++) {
                                uint32_t four[4] = {q, q, q, q};
                                four[pos] = r;
                                const uint32_t w = frontout_ev_u8(four[0], four[1], four[2], four[3]);
                                if (((w >> (8 * pos)) & 0xFFu) != val) fail("ev word (u8)", r, pos, w, val);
                                if (q != FRONTOUT_PAD && ((w >> (8 * (pos ^ 1u))) & 0xFFu) != (ref_val(q) & 0xFFu)) fail("ev word (u8), partner", q, pos, w, ref_val(q));
                            }
                        }
                        n++;
                    }
                }
    // the padding fix by itself
    if (frontout_pix_pair(FRONTOUT_PAD, FRONTOUT_PAD) != 0xFFFFFFFFu) fail("pix word of two padding slots", 0, 0, frontout_pix_pair(FRONTOUT_PAD, FRONTOUT_PAD), 0xFFFFFFFFu);
    return n;
}

// ---- 2. the order predicate
uint64_t check_pairs() {
    uint64_t n = 0;
    std::vector<uint32_t> es = {FRONTOUT_PAD};
    for (uint32_t c : CTXS)
        for (uint32_t o : OFFS)
            for (uint32_t va = 0; va < 4; va++) es.push_back(entry(c, va & 1u ? 511u : 0u, va >> 1, o));
    for (uint32_t r : es)
        for (uint32_t nx : es) {
            if (frontout_pair_bad(r, nx) != ref_bad(r, nx)) fail("order predicate", r, nx, frontout_pair_bad(r, nx), ref_bad(r, nx));
            n++;
        }
    return n;
}

// ---- 3. layout, windows, out
struct Tile {
    uint32_t nctx;
    std::vector<uint32_t> n[4];  // [wave][context]: events
};
struct Event {
    uint32_t rec, wave, rank;
};

// the kernel's steps 3 to 5 with the header's pieces; swap_at: exchange the ranks of the events that belong at slots swap_at, swap_at + 1
// (~0: none).  Returns whether the order check fired; pix / ev: what went out.
bool run_tile(const Tile &t, uint32_t swap_at, std::vector<uint16_t> &pix, std::vector<uint16_t> &ev, uint32_t &slots_out) {
    // events in raster order per (wave, context): pixel offsets ascend with the wave, then with the rank
    std::vector<Event> events;
    std::vector<uint32_t> cursor[4];
    uint32_t sums = 0, off = 0;
    for (uint32_t w = 0; w < 4; w++) cursor[w].resize(t.nctx);
    std::vector<uint32_t> off_of[4];
    for (uint32_t w = 0; w < 4; w++) {  // a wave's pixels come before the next wave's
        off_of[w].resize(t.nctx);
        for (uint32_t c = 0; c < t.nctx; c++) {
            off_of[w][c] = off;
            off += t.n[w][c];
        }
    }
    if (off > 4096) fail("the generator made more than 4096 events", off, 0, off, 4096);
    for (uint32_t c = 0; c < t.nctx; c++) {
        const uint32_t nw[4] = {t.n[0][c], t.n[1][c], t.n[2][c], t.n[3][c]};
        uint32_t cur[4];
        frontout_slot_bases(sums, nw, cur);
        for (uint32_t w = 0; w < 4; w++) {
            cursor[w][c] = cur[w];
            for (uint32_t k = 0; k < nw[w]; k++) events.push_back(Event{entry(c, (c + k) & 0x1FFu, k & 1u, (off_of[w][c] + k) & 0xFFFu), w, k});
        }
        sums += frontout_layout_term(nw[0] + nw[1] + nw[2] + nw[3]);
    }
    const uint32_t slots = sums >> 16;
    slots_out = slots;
    if (swap_at != ~0u) {
        Event *a = nullptr, *b = nullptr;
        for (Event &e : events) {
            const uint32_t s = cursor[e.wave][e.rec >> 22] + e.rank;
            if (s == swap_at) a = &e;
            if (s == swap_at + 1) b = &e;
        }
        if (!a || !b || a->wave != b->wave || (a->rec >> 22) != (b->rec >> 22)) return false;  // (not two events of one wave and context)
        const uint32_t k = a->rank;
        a->rank = b->rank;
        b->rank = k;
    }
    if (!frontout_one_window(slots, WINDOW)) return false;  // (a larger tile keeps the events' order in LDS: nothing of this header)
    pix.assign(slots, 0x1234);
    ev.assign(slots, 0x1234);
    std::vector<uint32_t> srt(WINDOW + 1 + 1, FRONTOUT_PAD);  // (the fill; [WINDOW]: the successor of the last slot, [WINDOW + 1]: a dummy word)
    for (const Event &e : events) srt[cursor[e.wave][e.rec >> 22] + e.rank] = e.rec;
    bool bad = false;
    for (uint32_t p0 = 0; p0 < slots; p0 += PASS)
        for (uint32_t j = p0; j < p0 + PASS && j < slots; j += 4) {  // (slots is a multiple of 16: no four are partial)
            const uint32_t *e = &srt[j];
            const uint32_t p01 = frontout_pix_pair(e[0], e[1]), p23 = frontout_pix_pair(e[2], e[3]);
            const uint32_t v01 = frontout_ev_u16(e[0], e[1]), v23 = frontout_ev_u16(e[2], e[3]);
            const uint32_t ps[4] = {p01 & 0xFFFFu, p01 >> 16, p23 & 0xFFFFu, p23 >> 16}, vs[4] = {v01 & 0xFFFFu, v01 >> 16, v23 & 0xFFFFu, v23 >> 16};
            for (uint32_t i = 0; i < 4; i++) {
                pix[j + i] = (uint16_t)ps[i];
                ev[j + i] = (uint16_t)vs[i];
                bad |= frontout_pair_bad(e[i], e[i + 1]);
            }
        }
    if (srt[WINDOW] != FRONTOUT_PAD) fail("the word behind the last slot", slots, 0, srt[WINDOW], FRONTOUT_PAD);
    return bad;
}

// the same tile's slots counted one by one
void ref_tile(const Tile &t, std::vector<uint16_t> &pix, std::vector<uint16_t> &ev) {
    pix.clear();
    ev.clear();
    uint32_t off = 0;
    std::vector<uint32_t> off_of[4];
    for (uint32_t w = 0; w < 4; w++) {
        off_of[w].resize(t.nctx);
        for (uint32_t c = 0; c < t.nctx; c++) {
            off_of[w][c] = off;
            off += t.n[w][c];
        }
    }
    for (uint32_t c = 0; c < t.nctx; c++) {
        for (uint32_t w = 0; w < 4; w++)
            for (uint32_t k = 0; k < t.n[w][c]; k++) {
                pix.push_back((uint16_t)(((off_of[w][c] + k) & 0xFFFu) | (k & 1u) << 12));
                ev.push_back((uint16_t)((c + k) & 0x1FFu));
            }
        while (pix.size() % FRONTOUT_REC) {
            pix.push_back(0xFFFF);
            ev.push_back(0xFFFF);  // (free)
        }
    }
}

uint64_t exchanges = 0, large = 0;
uint64_t check_tiles() {
    uint64_t n = 0;
    // a tile: `lead` records of filler contexts, so that the run under test starts `gap` records short of a mark -- a pass boundary
    // (1024, 2048 slots) or the end of the LDS image (4096: slots in use of 4096 - 16, 4096 and more) --, then a run of `len` events
    // split over the waves in one of several ways, then a run of `len2` directly behind it
    for (uint32_t mark : {1024u, 2048u, 4096u})
        for (uint32_t gap = 0; gap <= 3; gap++)
            for (uint32_t len = 0; len <= 33; len++)
                for (uint32_t split = 0; split < 3; split++)
                    for (uint32_t len2 : {0u, 1u, 16u, 33u}) {
                        const uint32_t lead = mark / FRONTOUT_REC - gap;
                        // filler: twenty contexts of 17 events (two records, 15 padding slots), the rest one record each with 1 .. 16
                        // events (a tile has at most 4096 events: 12 bits of pixel offset)
                        Tile t;
                        t.nctx = 512;
                        for (uint32_t w = 0; w < 4; w++) t.n[w].assign(t.nctx, 0);
                        uint32_t c = 0, left = lead;
                        while (left) {
                            const uint32_t recs = c < 20 ? 2u : 1u;
                            const uint32_t evs = recs == 2 ? 17u : 1u + (c * 5u) % 16u;
                            for (uint32_t k = 0; k < evs; k++) t.n[(k * 7 + c) & 3u][c]++;
                            left -= recs;
                            c++;
                        }
                        const uint32_t cu = c + 3;  // (an empty context or two in between: a run of length 0)
                        for (uint32_t k = 0; k < len; k++) t.n[split == 0 ? 0u : split == 1 ? (k & 3u) : (k < len / 2 ? 1u : 3u)][cu]++;
                        for (uint32_t k = 0; k < len2; k++) t.n[(k + 1) & 3u][cu + 1]++;
                        if (cu + 1 >= t.nctx) {
                            fail("the generator ran out of contexts", lead, cu, cu, t.nctx);
                            continue;
                        }
                        std::vector<uint16_t> pix, ev, rpix, rev;
                        uint32_t slots = 0;
                        const bool bad = run_tile(t, ~0u, pix, ev, slots);
                        ref_tile(t, rpix, rev);
                        if (!frontout_one_window(slots, WINDOW)) {
                            if (rpix.size() <= WINDOW || slots != rpix.size()) fail("a tile taken for large", lead, len, slots, rpix.size());
                            large++;
                            continue;
                        }
                        if (bad) fail("order check fired on a sorted tile", lead, len, 1, 0);
                        if (pix.size() != rpix.size()) fail("slots in use", lead, len, pix.size(), rpix.size());
                        else
                            for (size_t s = 0; s < pix.size(); s++) {
                                if (pix[s] != rpix[s]) fail("pix of slot", s, len, pix[s], rpix[s]);
                                if (rpix[s] != 0xFFFF && ev[s] != rev[s]) fail("ev of slot", s, len, ev[s], rev[s]);
                            }
                        // exchanged neighbours: around the run under test, at every slot near the mark
                        for (uint32_t s = mark - 72; s < mark + 72 && s + 1 < slots; s++) {
                            // (run_tile leaves p2 empty if slots s, s + 1 are not two events of one wave and context)
                            std::vector<uint16_t> p2, e2;
                            uint32_t s2 = 0;
                            const bool caught = run_tile(t, s, p2, e2, s2);
                            if (p2.empty()) continue;
                            if (!caught) fail("exchanged neighbours not caught at slot", s, len, 0, 1);
                            exchanges++;
                        }
                        n++;
                    }
    return n;
}

}  // namespace

int main() {
    const uint64_t words = check_words(), pairs = check_pairs(), tiles = check_tiles();
    if (failures) {
        fprintf(stderr, "frontout_check: %llu mismatches\n", (unsigned long long)failures);
        return 1;
    }
    printf("frontout_check: %llu entry classes beside their partners, %llu ordered pairs, %llu tiles at the pass boundaries and the window's end (and %llu larger), %llu exchanges caught: ok\n",
           (unsigned long long)words, (unsigned long long)pairs, (unsigned long long)tiles, (unsigned long long)large, (unsigned long long)exchanges);
    return 0;
}
