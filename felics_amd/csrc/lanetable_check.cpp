// lanetable_check.cpp -- host check of felics_lanetable.h, the index rule k_decode16_lanes compiles: for every table size the rule
// can return, the most contexts it admits for that size are inserted and found again, in sets chosen to collide (all congruent
// modulo the row count, consecutive, the top of the range), no search is longer than the row count, and the byte count is the
// rows' (tests/test_lanetable.py runs this; exit status 0 = every check held).
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <vector>

#include "felics_lanetable.h"

using namespace felics;

static int failures = 0;
#define CHECK(c, ...)                      \
    do {                                   \
        if (!(c)) {                        \
            failures++;                    \
            printf("FAILED %s: ", #c);     \
            printf(__VA_ARGS__);           \
            printf("\n");                  \
            if (failures > 20) exit(1);    \
        }                                  \
    } while (0)

// inserts `set` (distinct contexts) into an empty table of `rows` rows in `epoch`, then finds each again; stale rows of another
// epoch (`stale`) fill the table beforehand
static void run(uint32_t rows, const std::vector<uint32_t> &set, const char *name, uint32_t epoch, uint32_t stale) {
    std::vector<uint32_t> tags(rows);
    for (uint32_t r = 0; r < rows; r++) tags[r] = stale ? dec16l_tag(stale, r % DEC16L_CONTEXTS) : 0u;
    std::vector<uint32_t> where(set.size());
    uint32_t longest = 0;
    for (size_t i = 0; i < set.size(); i++) {
        bool found = true;
        uint32_t probes = 0;
        const uint32_t at = dec16l_find(set[i], rows, epoch, [&](uint32_t r) { return r < rows ? tags[r] : (failures++, 0u); }, found, &probes);
        CHECK(at != DEC16L_FULL && at < rows, "%s rows %u: context %u has no row", name, rows, set[i]);
        CHECK(!found, "%s rows %u: context %u found before it was inserted", name, rows, set[i]);
        CHECK(probes >= 1 && probes <= rows, "%s rows %u: %u probes", name, rows, probes);
        if (at >= rows) return;
        tags[at] = dec16l_tag(epoch, set[i]);
        where[i] = at;
        longest = std::max(longest, probes);
    }
    for (size_t i = 0; i < set.size(); i++) {
        bool found = false;
        uint32_t probes = 0;
        const uint32_t at = dec16l_find(set[i], rows, epoch, [&](uint32_t r) { return r < rows ? tags[r] : (failures++, 0u); }, found, &probes);
        CHECK(found && at == where[i], "%s rows %u: context %u not found again (row %u, was %u)", name, rows, set[i], at, where[i]);
        CHECK(probes <= rows, "%s rows %u: %u probes", name, rows, probes);
        longest = std::max(longest, probes);
    }
    printf("rows %6u %-12s %6zu contexts, longest search %u\n", rows, name, set.size(), longest);
}

int main() {
    // every size the rule returns, smallest to dense, and the pixel counts at which it changes
    std::vector<uint32_t> sizes;
    uint32_t last = 0;
    for (uint64_t npix = 0; npix <= 140000; npix++) {
        for (uint32_t planes : {1u, 3u}) {
            const uint32_t rows = dec16l_rows(npix, planes);
            CHECK(dec16l_max_contexts(npix) <= dec16l_capacity(rows), "npix %llu: %u contexts in %u rows", (unsigned long long)npix,
                  dec16l_max_contexts(npix), rows);
            CHECK(dec16l_dense(rows) || (rows >= DEC16L_MIN_ROWS && rows <= DEC16L_MAX_HASHED_ROWS && (rows & (rows - 1)) == 0), "npix %llu: %u rows",
                  (unsigned long long)npix, rows);
            CHECK(rows >= last, "npix %llu: rows shrink", (unsigned long long)npix);
            const uint32_t W = npix ? 8 : 0, H = (uint32_t)(npix / 8);  // (a shape with W * H = npix where 8 divides it)
            if (npix % 8 == 0)
                CHECK((size_t)rows * 64 * planes == decode16_lanes_table_bytes(1, W, H, planes == 3), "npix %llu planes %u: %zu bytes",
                      (unsigned long long)npix, planes, decode16_lanes_table_bytes(1, W, H, planes == 3));
            if (planes == 1 && rows != last) {
                printf("from %6llu pixels: %6u rows\n", (unsigned long long)npix, rows);
                sizes.push_back(rows);
                last = rows;
            }
        }
    }
    CHECK(dec16l_rows(0xFFFFFFFFull, 1) == DEC16L_CONTEXTS && dec16l_rows(1ull << 40, 3) == DEC16L_CONTEXTS, "large frames are dense");
    CHECK(sizes.front() == DEC16L_MIN_ROWS && sizes.back() == DEC16L_CONTEXTS && sizes.size() == 12, "%zu sizes", sizes.size());
    CHECK(dec16l_rows(64 * 64, 1) * 64 == 512 * 1024, "a 64 x 64 plane takes %u rows", dec16l_rows(64 * 64, 1));
    CHECK(dec16l_rows(128 * 256, 1) == 65536 && dec16l_rows(129 * 256, 1) == DEC16L_CONTEXTS, "the switch to the dense table");
    for (uint32_t rows : sizes) {
        const uint32_t cap = dec16l_capacity(rows), top = DEC16L_CONTEXTS - 1;
        std::vector<uint32_t> set;
        // all congruent modulo the row count (as many as the context range holds, then the next residue's)
        for (uint32_t i = 0; i < rows && set.size() < cap; i++)
            for (uint32_t c = (5 + i) % rows; set.size() < cap && c <= top; c += rows) set.push_back(c);
        run(rows, set, "congruent", 1, 0);
        set.clear();
        for (uint32_t c = 0; c < cap; c++) set.push_back(c);  // consecutive from 0
        run(rows, set, "consecutive", 2, 1);
        set.clear();
        for (uint32_t c = 0; c < cap; c++) set.push_back(top - c);  // 131 070 and its neighbours
        run(rows, set, "top", DEC16L_EPOCH_MAX, DEC16L_EPOCH_MAX - 1);
        set.clear();
        for (uint32_t c = 0; c < cap && c * 4096u <= top; c++) set.push_back(c * 4096u);  // one bucket under a masking hash
        run(rows, set, "x4096", 7, 7 + 1);
    }
    // a table with no empty row and without the context: the search gives up after `rows` probes
    {
        const uint32_t rows = DEC16L_MIN_ROWS;
        std::vector<uint32_t> tags(rows);
        for (uint32_t r = 0; r < rows; r++) tags[r] = dec16l_tag(3, 1000 + r);
        bool found = true;
        uint32_t probes = 0;
        const uint32_t at = dec16l_find(5, rows, 3, [&](uint32_t r) { return tags[r]; }, found, &probes);
        CHECK(at == DEC16L_FULL && !found && probes == rows, "full table: row %u after %u probes", at, probes);
    }
    printf(failures ? "%d checks FAILED\n" : "all checks held\n", failures);
    return failures ? 1 : 0;
}
