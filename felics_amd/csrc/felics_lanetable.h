// felics_lanetable.h -- the index rule of a lane's estimator table in the 16-bit lane decoder (k_decode16_lanes,
// felics_gpudecode.hip): how many rows a stream's table has, where a context's row is looked for, and how the search ends.
// The kernel, the host code that sizes the tables (felics_api.cpp) and the native check (lanetable_check.cpp) compile these
// same functions.
//
// A 16-bit plane has contexts 0 .. 131 070, but only a pixel coded out of range touches the estimator, and every such pixel
// touches ONE context: a plane of N pixels (the first two are stored raw) uses at most N - 2 of them.  So a table has
//     rows = the power of two >= 2 * (N - 2), at least DEC16L_MIN_ROWS        (open addressing, never more than half full)
// and once that would pass 65 536 rows it is the dense table of the wave form: DEC16L_CONTEXTS rows, row = context.
// Every plane of a stream has a table of its own, so a stream's tables are rows * planes rows of DEC16L_ROW_BYTES.
//
// A row is sixteen words: fifteen counters and a tag = (epoch << 17) | context.  A launch owns one epoch per plane; a row whose
// tag carries another epoch is EMPTY (left over from another plane, stream or call), so the buffer is zeroed once and never
// between calls (epoch 0 is never handed out).  Within an epoch rows are only ever added, so a search that starts at the
// context's home row and walks on by dec16l_next ends at the context's row or at the first empty one -- or, in a table with no
// empty row, after `rows` steps with DEC16L_FULL (cannot happen under the sizing rule; the kernel reports it, it does not loop).
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FELICS_HD __host__ __device__ inline
#else
#define FELICS_HD inline
#endif

namespace felics {

constexpr uint32_t DEC16L_CONTEXTS = 2u * 65535u + 1u;  // MAX_CONTEXT + 1 (traits.rs:38): the dense table's rows
constexpr uint32_t DEC16L_MIN_ROWS = 64;                // 4 KB: the smallest table
constexpr uint32_t DEC16L_MAX_HASHED_ROWS = 65536;      // the largest hashed table; the next size is the dense one
constexpr uint32_t DEC16L_ROW_BYTES = 64;               // fifteen counters + tag
constexpr uint32_t DEC16L_EPOCH_MAX = 0x7FFFu;          // 15 bits of a tag; 17 for the context
constexpr uint32_t DEC16L_FULL = 0xFFFFFFFFu;

// distinct contexts a plane of npix pixels can use
FELICS_HD uint32_t dec16l_max_contexts(uint64_t npix) {
    const uint64_t c = npix > 2 ? npix - 2 : 0;
    return c < DEC16L_CONTEXTS ? (uint32_t)c : DEC16L_CONTEXTS;
}

// rows of ONE plane's table (a stream has `planes` of them, all of this size: the argument is there for the caller's arithmetic)
FELICS_HD uint32_t dec16l_rows(uint64_t npix, uint32_t planes) {
    (void)planes;
    const uint64_t need = 2ull * dec16l_max_contexts(npix);
    if (need > DEC16L_MAX_HASHED_ROWS) return DEC16L_CONTEXTS;
    uint32_t rows = DEC16L_MIN_ROWS;
    while (rows < need) rows <<= 1;
    return rows;
}

// table memory of n streams of W x H (color: 0 gray, 1 RGB) in one launch of the lane form
FELICS_HD size_t decode16_lanes_table_bytes(uint32_t n, uint32_t W, uint32_t H, uint32_t color) {
    const uint32_t np = color ? 3u : 1u;
    return (size_t)n * np * dec16l_rows((uint64_t)W * H, np) * DEC16L_ROW_BYTES;
}

FELICS_HD bool dec16l_dense(uint32_t rows) { return rows == DEC16L_CONTEXTS; }

// contexts a table of `rows` rows admits (what the sizing rule promises never to exceed)
FELICS_HD uint32_t dec16l_capacity(uint32_t rows) { return dec16l_dense(rows) ? DEC16L_CONTEXTS : rows / 2; }

// home row of a context: the top log2(rows) bits of a multiplicative hash (contexts congruent modulo the row count, or
// consecutive, spread over the table); dense: the context itself
FELICS_HD uint32_t dec16l_home(uint32_t ctx, uint32_t rows) {
    if (dec16l_dense(rows)) return ctx;
    return (ctx * 0x9E3779B1u) >> ((uint32_t)__builtin_clz(rows) + 1u);  // 32 - log2(rows); rows is a power of two in 64 .. 65 536
}

// probe step: the next row, around the end
FELICS_HD uint32_t dec16l_next(uint32_t row, uint32_t rows) { return (row + 1u) & (rows - 1u); }

FELICS_HD uint32_t dec16l_tag(uint32_t epoch, uint32_t ctx) { return (epoch << 17) | ctx; }

// The row of `ctx` in a table of `rows` rows in epoch `epoch`.  tag_at(row) returns that row's tag word (the caller may keep the
// rest of the row it loaded with it: the last call of tag_at is for the row returned).  found: the row holds the context's
// counters; otherwise it is empty and the context's to fill.  Returns DEC16L_FULL after `rows` probes without either.
// probes (optional) counts the calls of tag_at.
template <typename TagAt>
FELICS_HD uint32_t dec16l_find(uint32_t ctx, uint32_t rows, uint32_t epoch, TagAt tag_at, bool &found, uint32_t *probes = nullptr) {
    const uint32_t want = dec16l_tag(epoch, ctx);
    uint32_t row = dec16l_home(ctx, rows);
    const uint32_t limit = dec16l_dense(rows) ? 1u : rows;
    uint32_t n = 0;
    found = false;
    uint32_t at = DEC16L_FULL;
    while (n < limit) {
        const uint32_t tag = tag_at(row);
        n++;
        if (tag == want) {
            found = true;
            at = row;
            break;
        }
        if ((tag >> 17) != epoch) {  // empty
            at = row;
            break;
        }
        row = dec16l_next(row, rows);
    }
    if (probes) *probes = n;
    return at;
}

}  // namespace felics
