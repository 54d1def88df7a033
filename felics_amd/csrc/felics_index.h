// felics_index.h -- layout of the restart index (include/felics.h), for the host builder / decoder
// (felics_index.cpp), the host side of the device calls and the segment kernels alike.  Little-endian throughout.
#ifndef FELICS_INDEX_H
#define FELICS_INDEX_H

#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <new>
#include <vector>

#include "../../include/felics.h"

#ifdef __HIPCC__
#define FELICS_IDX_HD __host__ __device__
#else
#define FELICS_IDX_HD
#endif

namespace felics {

constexpr uint32_t INDEX_HEADER_BYTES = 64;
constexpr uint32_t INDEX_VERSION = 1;
// byte offsets of the header's fields: "FLCX" | u16 version | u8 colour | u8 depth | u32 width | u32 height | u32 segment_pixels |
// u32 K | u64 plane_end_bit[3] | 16 reserved zero bytes
constexpr uint32_t IDX_VERSION = 4, IDX_COLOR = 6, IDX_DEPTH = 7, IDX_WIDTH = 8, IDX_HEIGHT = 12, IDX_SEGPIX = 16, IDX_K = 20, IDX_PLANE_END = 24,
                   IDX_RESERVED = 48;
constexpr uint64_t STREAM_HEADER_BITS = 8ull * FELICS_HEADER_BYTES;  // 112: where plane 0 starts

// A checkpoint: u64 bit_offset | u16 state[nctx][6] | window[2 W] (u8 gray, i16 Y / Co / Cg) | zeros up to a multiple of 16.
// Checkpoint (plane c, segment j) lies at INDEX_HEADER_BYTES + (c * K + j) * cp_bytes.
struct IndexLayout {
    uint32_t planes, nctx, K;
    uint32_t sample_bytes;  // of a window sample
    uint64_t win_off;       // of the window in a checkpoint (the state is at CP_STATE_OFF)
    uint64_t cp_bytes;
    uint64_t total;         // bytes of the whole index
};
constexpr uint32_t CP_STATE_OFF = 8;

FELICS_IDX_HD inline bool index_segment_ok(uint32_t segment_pixels) {
    return segment_pixels >= FELICS_INDEX_GRANULE && segment_pixels % FELICS_INDEX_GRANULE == 0;
}
// (w * h < 2^32 and index_segment_ok: the caller's checks)
FELICS_IDX_HD inline IndexLayout index_layout(uint32_t w, uint32_t h, uint32_t color, uint32_t segment_pixels) {
    IndexLayout L;
    L.planes = color ? 3u : 1u;
    L.nctx = color ? 512u : 256u;
    L.sample_bytes = color ? 2u : 1u;
    const uint64_t npix = (uint64_t)w * h;
    L.K = (uint32_t)((npix + segment_pixels - 1) / segment_pixels);
    L.win_off = CP_STATE_OFF + (uint64_t)L.nctx * 6u * 2u;
    L.cp_bytes = (L.win_off + 2ull * w * L.sample_bytes + 15u) & ~15ull;
    L.total = INDEX_HEADER_BYTES + (uint64_t)L.planes * L.K * L.cp_bytes;
    return L;
}

// The whole index of an empty image (K = 0, INDEX_HEADER_BYTES bytes): the header, every plane its two raw samples long.
inline void empty_index(uint8_t *ih, uint32_t w, uint32_t h, uint32_t color, uint32_t segment_pixels) {
    for (uint32_t i = 0; i < INDEX_HEADER_BYTES; i++) ih[i] = 0;
    ih[0] = 'F', ih[1] = 'L', ih[2] = 'C', ih[3] = 'X';
    ih[IDX_VERSION] = INDEX_VERSION;
    ih[IDX_COLOR] = (uint8_t)color;
    for (int k = 0; k < 4; k++) {
        ih[IDX_WIDTH + k] = (uint8_t)(w >> (8 * k));
        ih[IDX_HEIGHT + k] = (uint8_t)(h >> (8 * k));
        ih[IDX_SEGPIX + k] = (uint8_t)(segment_pixels >> (8 * k));
    }
    for (uint32_t c = 0; c < (color ? 3u : 1u); c++) {
        const uint64_t end = STREAM_HEADER_BITS + 64u * (c + 1);
        for (int k = 0; k < 8; k++) ih[IDX_PLANE_END + 8 * c + k] = (uint8_t)(end >> (8 * k));
    }
}

FELICS_IDX_HD inline uint32_t idx_rd16(const uint8_t *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8); }
FELICS_IDX_HD inline uint32_t idx_rd32(const uint8_t *p) { return idx_rd16(p) | (idx_rd16(p + 2) << 16); }
FELICS_IDX_HD inline uint64_t idx_rd64(const uint8_t *p) { return (uint64_t)idx_rd32(p) | ((uint64_t)idx_rd32(p + 4) << 32); }

// The checks of an index header against the stream's (felics.h): 0, or FELICS_E_INVALID_INDEX.  `ih` holds INDEX_HEADER_BYTES bytes;
// the stream is 8-bit (FELICS_E_UNSUPPORTED is the caller's answer otherwise) with w * h < 2^32.  On success L is the layout the
// header names, and the caller compares L.total with the bytes it was given.
FELICS_IDX_HD inline int index_header_check(const uint8_t *ih, uint32_t color, uint32_t w, uint32_t h, uint64_t stream_len, IndexLayout &L) {
    if (ih[0] != 'F' || ih[1] != 'L' || ih[2] != 'C' || ih[3] != 'X' || idx_rd16(ih + IDX_VERSION) != INDEX_VERSION) return FELICS_E_INVALID_INDEX;
    if (ih[IDX_COLOR] != color || ih[IDX_DEPTH] != FELICS_DEPTH_8 || idx_rd32(ih + IDX_WIDTH) != w || idx_rd32(ih + IDX_HEIGHT) != h)
        return FELICS_E_INVALID_INDEX;
    const uint32_t seg = idx_rd32(ih + IDX_SEGPIX);
    if (!index_segment_ok(seg)) return FELICS_E_INVALID_INDEX;
    L = index_layout(w, h, color, seg);
    if (idx_rd32(ih + IDX_K) != L.K) return FELICS_E_INVALID_INDEX;
    // the planes follow each other from the header on and the last one ends in the stream's last byte
    uint64_t prev = STREAM_HEADER_BITS;
    for (uint32_t c = 0; c < 3; c++) {
        const uint64_t e = idx_rd64(ih + IDX_PLANE_END + 8 * c);
        if (c >= L.planes) {
            if (e) return FELICS_E_INVALID_INDEX;
            continue;
        }
        if (e < prev + 64u || e > 8u * stream_len) return FELICS_E_INVALID_INDEX;  // (a plane holds its two raw samples at least)
        prev = e;
    }
    if ((prev + 7u) / 8u != stream_len) return FELICS_E_INVALID_INDEX;
    for (uint32_t i = IDX_RESERVED; i < INDEX_HEADER_BYTES; i++)
        if (ih[i]) return FELICS_E_INVALID_INDEX;
    return FELICS_OK;
}

// Where segment (c, j) must start and end, and what is wrong with that before a bit is decoded: 0, or FELICS_E_INVALID_INDEX.
// idx: the whole index (header checked); K = 0 (an empty image) has one pseudo segment per plane, the two raw samples.
FELICS_IDX_HD inline int index_segment_bounds(const uint8_t *idx, const IndexLayout &L, uint32_t c, uint32_t j, uint64_t stream_len, uint64_t &start,
                                          uint64_t &end) {
    const uint64_t plane_start = c ? idx_rd64(idx + IDX_PLANE_END + 8 * (c - 1)) : STREAM_HEADER_BITS;
    const uint64_t plane_end = idx_rd64(idx + IDX_PLANE_END + 8 * c);
    if (L.K == 0) {
        start = plane_start;
        end = plane_end;
        return FELICS_OK;
    }
    const uint8_t *cp = idx + INDEX_HEADER_BYTES + ((uint64_t)c * L.K + j) * L.cp_bytes;
    start = idx_rd64(cp);
    end = j + 1 < L.K ? idx_rd64(cp + L.cp_bytes) : plane_end;
    if (start < STREAM_HEADER_BITS || start > 8u * stream_len || end > 8u * stream_len || end < start) return FELICS_E_INVALID_INDEX;
    if (j == 0 ? start != plane_start : start < idx_rd64(cp - L.cp_bytes)) return FELICS_E_INVALID_INDEX;
    return FELICS_OK;
}

// ---- version 2: the index of a 16-bit stream (felics.h "Restart index: 16-bit streams").  A 16-bit plane has up to 131 071 contexts of
// fifteen 32-bit counters, so a checkpoint's state is SPARSE: the rows of the contexts that are live at it, of any number.  Header (64
// bytes) | directory of C K entries | windows | state rows; everything but the rows lies where the header says.
constexpr uint32_t INDEX16_VERSION = 2;
constexpr uint32_t IDX16_TOTAL = 48, IDX16_RESERVED = 56;  // u64 total_bytes | 8 zero bytes (the fields in front are version 1's)
// a directory entry: u64 bit_offset | u64 rows_off | u32 n_rows | 12 zero bytes
constexpr uint32_t INDEX16_ENTRY_BYTES = 32, E16_BIT = 0, E16_ROWS_OFF = 8, E16_NROWS = 16, E16_RESERVED = 20;
// a state row: u32 counter[15] | u32 context (k_decode16's row with the context where the epoch goes)
constexpr uint32_t INDEX16_ROW_BYTES = 64, INDEX16_ROW_CTX = 15;
constexpr uint32_t INDEX16_CONTEXTS = 2u * 65535u + 1u;  // contexts a Co / Cg plane can have; gray and Y: 65 536

struct Index16Layout {
    uint32_t planes, K;
    uint32_t sample_bytes;  // of a window sample: 2 (u16) gray, 4 (i32) Y / Co / Cg
    uint64_t win_bytes;     // of a window: 2 W samples, rounded up to 16
    uint64_t win_base;      // window (c, j) at win_base + (c K + j) win_bytes
    uint64_t rows_base;     // the first state row; the least an index of this shape is long
};

FELICS_IDX_HD inline uint32_t index16_contexts(uint32_t color, uint32_t c) { return color && c ? INDEX16_CONTEXTS : 65536u; }
// (w * h < 2^32 and index_segment_ok: the caller's checks)
FELICS_IDX_HD inline Index16Layout index16_layout(uint32_t w, uint32_t h, uint32_t color, uint32_t segment_pixels) {
    Index16Layout L;
    L.planes = color ? 3u : 1u;
    L.sample_bytes = color ? 4u : 2u;
    const uint64_t npix = (uint64_t)w * h;
    L.K = (uint32_t)((npix + segment_pixels - 1) / segment_pixels);
    L.win_bytes = (2ull * w * L.sample_bytes + 15u) & ~15ull;
    L.win_base = (INDEX_HEADER_BYTES + (uint64_t)INDEX16_ENTRY_BYTES * L.planes * L.K + 63u) & ~63ull;
    L.rows_base = (L.win_base + (uint64_t)L.planes * L.K * L.win_bytes + 63u) & ~63ull;
    return L;
}

// The checks of a version-2 header against the stream's and the length the caller gave: 0, or FELICS_E_INVALID_INDEX.  `ih` holds
// INDEX_HEADER_BYTES bytes; the stream is 16-bit with w * h < 2^32.  On success L is the layout the header names and
// index_len >= L.rows_base: the directory and every window lie inside the index.
FELICS_IDX_HD inline int index16_header_check(const uint8_t *ih, uint32_t color, uint32_t w, uint32_t h, uint64_t stream_len, uint64_t index_len,
                                              Index16Layout &L) {
    if (ih[0] != 'F' || ih[1] != 'L' || ih[2] != 'C' || ih[3] != 'X' || idx_rd16(ih + IDX_VERSION) != INDEX16_VERSION) return FELICS_E_INVALID_INDEX;
    if (ih[IDX_COLOR] != color || ih[IDX_DEPTH] != FELICS_DEPTH_16 || idx_rd32(ih + IDX_WIDTH) != w || idx_rd32(ih + IDX_HEIGHT) != h)
        return FELICS_E_INVALID_INDEX;
    const uint32_t seg = idx_rd32(ih + IDX_SEGPIX);
    if (!index_segment_ok(seg)) return FELICS_E_INVALID_INDEX;
    L = index16_layout(w, h, color, seg);
    if (idx_rd32(ih + IDX_K) != L.K) return FELICS_E_INVALID_INDEX;
    uint64_t prev = STREAM_HEADER_BITS;
    for (uint32_t c = 0; c < 3; c++) {
        const uint64_t e = idx_rd64(ih + IDX_PLANE_END + 8 * c);
        if (c >= L.planes) {
            if (e) return FELICS_E_INVALID_INDEX;
            continue;
        }
        if (e < prev + 64u || e > 8u * stream_len) return FELICS_E_INVALID_INDEX;
        prev = e;
    }
    if ((prev + 7u) / 8u != stream_len) return FELICS_E_INVALID_INDEX;
    const uint64_t total = idx_rd64(ih + IDX16_TOTAL);
    if (total != index_len || total < L.rows_base || total % INDEX16_ROW_BYTES) return FELICS_E_INVALID_INDEX;
    for (uint32_t i = IDX16_RESERVED; i < INDEX_HEADER_BYTES; i++)
        if (ih[i]) return FELICS_E_INVALID_INDEX;
    return FELICS_OK;
}

// Where segment (c, j) starts and ends in the stream and where its state rows lie, and what is wrong with that before a bit is decoded
// or a row is read: 0, or FELICS_E_INVALID_INDEX.  idx: the whole index of `total` bytes (header checked, so every directory entry is
// inside it).  The bit range by version 1's rules; the rows inside [rows_base, total), whole rows, none for segment 0, and CHAINED:
// (0, 0)'s start at rows_base, an entry's end where its successor's start in (plane, segment) order, the last one's at `total`.
// K = 0 (an empty image) has one pseudo segment per plane, the two raw samples, and no rows.
FELICS_IDX_HD inline int index16_segment_bounds(const uint8_t *idx, const Index16Layout &L, uint32_t c, uint32_t j, uint64_t stream_len,
                                                uint64_t total, uint64_t &start, uint64_t &end, uint64_t &rows_off, uint32_t &n_rows) {
    const uint64_t plane_start = c ? idx_rd64(idx + IDX_PLANE_END + 8 * (c - 1)) : STREAM_HEADER_BITS;
    const uint64_t plane_end = idx_rd64(idx + IDX_PLANE_END + 8 * c);
    rows_off = L.rows_base;
    n_rows = 0;
    if (L.K == 0) {
        start = plane_start;
        end = plane_end;
        return FELICS_OK;
    }
    const uint8_t *e = idx + INDEX_HEADER_BYTES + ((uint64_t)c * L.K + j) * INDEX16_ENTRY_BYTES;
    start = idx_rd64(e + E16_BIT);
    end = j + 1 < L.K ? idx_rd64(e + INDEX16_ENTRY_BYTES + E16_BIT) : plane_end;
    if (start < STREAM_HEADER_BITS || start > 8u * stream_len || end > 8u * stream_len || end < start) return FELICS_E_INVALID_INDEX;
    if (j == 0 ? start != plane_start : start < idx_rd64(e - INDEX16_ENTRY_BYTES + E16_BIT)) return FELICS_E_INVALID_INDEX;
    rows_off = idx_rd64(e + E16_ROWS_OFF);
    n_rows = idx_rd32(e + E16_NROWS);
    if (rows_off < L.rows_base || rows_off % INDEX16_ROW_BYTES || rows_off > total ||
        (uint64_t)n_rows * INDEX16_ROW_BYTES > total - rows_off)
        return FELICS_E_INVALID_INDEX;
    const bool last = c + 1 == L.planes && j + 1 == L.K;
    const uint64_t next = last ? total : idx_rd64(e + INDEX16_ENTRY_BYTES + E16_ROWS_OFF);
    if (rows_off + (uint64_t)n_rows * INDEX16_ROW_BYTES != next || (c == 0 && j == 0 && rows_off != L.rows_base)) return FELICS_E_INVALID_INDEX;
    if (j == 0 && n_rows != 0) return FELICS_E_INVALID_INDEX;
    for (uint32_t i = E16_RESERVED; i < INDEX16_ENTRY_BYTES; i++)
        if (e[i]) return FELICS_E_INVALID_INDEX;
    return FELICS_OK;
}

// ---- regions (felics.h "Restart index: regions"): the planner's arithmetic, for felics_region_segments, the host model and the host
// side of the device call alike.  W * H < 2^32, index_segment_ok(seg) and region_inside are the caller's checks.
FELICS_IDX_HD inline bool region_inside(uint32_t W, uint32_t H, const felics_region &r) {
    return (uint64_t)r.x + r.w <= W && (uint64_t)r.y + r.h <= H;
}
FELICS_IDX_HD inline bool region_empty(const felics_region &r) { return r.w == 0 || r.h == 0; }
// the pixel behind the region's last one: no walk goes further
FELICS_IDX_HD inline uint64_t region_last(uint32_t W, const felics_region &r) { return (uint64_t)(r.y + r.h - 1) * W + r.x + r.w; }
// Does segment j = pixels [a, b) hold a pixel of the (non-empty) region?  Row yy's span [yy W + x, yy W + x + w) meets [a, b) iff
// yy W + x < b and yy W + x + w > a: yy <= (b - x - 1) / W and, where a >= x + w, yy >= (a - x - w) / W + 1; some yy of
// [y, y + h) must satisfy both.
FELICS_IDX_HD inline bool region_needs(uint32_t W, uint64_t npix, uint32_t seg, const felics_region &r, uint32_t j) {
    const uint64_t a = (uint64_t)j * seg, b = a + seg < npix ? a + seg : npix;
    if (b <= r.x) return false;
    const uint64_t hi_row = (b - r.x - 1) / W, hi = hi_row < (uint64_t)r.y + r.h - 1 ? hi_row : (uint64_t)r.y + r.h - 1;
    const uint64_t lo_row = a >= (uint64_t)r.x + r.w ? (a - r.x - r.w) / W + 1 : 0, lo = lo_row > r.y ? lo_row : r.y;
    return lo <= hi;
}
// the segments that can be needed at all: those of the region's first and last pixel and the ones between
FELICS_IDX_HD inline void region_span(uint32_t W, uint32_t seg, const felics_region &r, uint32_t &first, uint32_t &last) {
    first = (uint32_t)(((uint64_t)r.y * W + r.x) / seg);
    last = (uint32_t)((region_last(W, r) - 1) / seg);
}

// The plan of a region call, 8- or 16-bit alike (felics_decompress_regions_device_indexed / _indexed16; index_fuzz checks it under the
// sanitizers): one wave per work item = (region, plane, needed segment).  A region's items are contiguous, in (plane, segment)
// order; an item whose segment is REGION_HEADER_ONLY makes the checks of its stream's header and index header and nothing else (the
// one item of an empty region).  Crops are dense and back to back: out_off in BYTES of the depth's sample; RGB crops go through
// crop-sized planes at plane_off (SAMPLES of the depth's plane type, three planes of w * h), converted where status[region] is clean.
constexpr uint32_t REGION_HEADER_ONLY = 0xFFFFFFFFu;
struct RegionRow {
    uint32_t stream;         // index into offsets / lens and of the index
    uint32_t x, y, w, h;
    uint32_t item0, nitems;  // its items: item0 .. item0 + nitems - 1, nitems >= 1
    uint32_t pad;
    uint64_t out_off, plane_off;
};
struct RegionItem {
    uint32_t region, plane, seg;
};
struct RegionPlan {
    std::vector<RegionRow> rows;
    std::vector<RegionItem> items;
    uint64_t plane_samples = 0;  // of all the RGB crops' planes
    uint64_t max_crop = 0;       // the largest w * h of an RGB region (0: gray)
    uint64_t walked = 0, skipped = 0, pixels_walked = 0;  // segments named / not named, pixels the named ones walk (per plane each)
};
// One request on a stream of W x H pixels, `planes` planes, segments of segment_pixels, added to the plan as region `region` (the
// number its items carry): its row, its items, what it walks.  The crop starts at out_at (advanced by its bytes; sample_bytes: of an
// output sample) and its RGB planes at P.plane_samples (advanced).  header_item: an empty region gets the one REGION_HEADER_ONLY
// item; without it an empty region has no item (felics_decompress_region_views_device_indexed: the header checks are the host's).
// P.skipped is the caller's.  0, or FELICS_E_UNSUPPORTED past 2^31 - 1 items; may throw std::bad_alloc.
inline int region_plan_add(uint32_t W, uint32_t H, uint32_t segment_pixels, uint32_t planes, uint32_t sample_bytes, const felics_region &g,
                           uint32_t region, bool header_item, uint64_t &out_at, std::vector<uint32_t> &segs, RegionPlan &P) {
    const uint64_t npix = (uint64_t)W * H;
    segs.clear();
    uint64_t stop_at = 0;
    if (!region_empty(g)) {
        uint32_t first, last;
        region_span(W, segment_pixels, g, first, last);
        for (uint32_t j = first; j <= last; j++)
            if (region_needs(W, npix, segment_pixels, g, j)) segs.push_back(j);
        stop_at = region_last(W, g);
    }
    const uint64_t cnt = segs.empty() ? (header_item ? 1 : 0) : (uint64_t)planes * segs.size();
    if (P.items.size() + cnt > 0x7FFFFFFFull) return FELICS_E_UNSUPPORTED;
    const uint64_t cpix = (uint64_t)g.w * g.h;
    P.rows.push_back(RegionRow{g.stream, g.x, g.y, g.w, g.h, (uint32_t)P.items.size(), (uint32_t)cnt, 0, out_at, P.plane_samples});
    out_at += cpix * planes * sample_bytes;
    if (planes == 3) {
        P.plane_samples += cpix * 3;
        P.max_crop = std::max(P.max_crop, cpix);
    }
    if (segs.empty() && header_item) P.items.push_back(RegionItem{region, 0, REGION_HEADER_ONLY});
    for (uint32_t c = 0; c < planes && !segs.empty(); c++)
        for (const uint32_t j : segs) P.items.push_back(RegionItem{region, c, j});
    for (const uint32_t j : segs) {
        const uint64_t p0 = (uint64_t)j * segment_pixels;
        P.pixels_walked += (std::min({npix, p0 + segment_pixels, stop_at}) - p0) * planes;
    }
    P.walked += (uint64_t)planes * segs.size();
    return FELICS_OK;
}
// n requests on streams of W x H pixels, `planes` planes, segments of segment_pixels; sample_bytes: of an output sample.
// out_offsets (may be null): where crop r starts.  0, FELICS_E_UNSUPPORTED past 2^31 - 1 items (one block per item, 32-bit item
// numbers) or FELICS_E_IO (no memory).
inline int region_plan(uint32_t W, uint32_t H, uint32_t segment_pixels, uint32_t planes, uint32_t sample_bytes, const felics_region *regions, size_t n,
                       uint64_t *out_offsets, RegionPlan &P) {
    const uint64_t npix = (uint64_t)W * H;
    std::vector<uint32_t> segs;
    uint64_t out_at = 0;
    try {
        P.rows.reserve(n);
        for (size_t r = 0; r < n; r++) {
            if (out_offsets) out_offsets[r] = out_at;
            const int rc = region_plan_add(W, H, segment_pixels, planes, sample_bytes, regions[r], (uint32_t)r, true, out_at, segs, P);
            if (rc) return rc;
        }
    } catch (const std::bad_alloc &) {
        return FELICS_E_IO;
    }
    P.skipped = (uint64_t)n * planes * ((npix + segment_pixels - 1) / segment_pixels) - P.walked;
    return FELICS_OK;
}

// ---- views (felics.h "Restart index: views and mixed shapes"): what felics_decompress_views_device_indexed's host side, its kernel's
// sink and the host model share.
// Where sample (col, y) of channel c of a view lies, in bytes from the view's `data`: the one place this is worked out for
// k_decode8_seg_views' ViewSink and for felics_decompress_indexed_view.
FELICS_IDX_HD inline int64_t view_sample_offset(int64_t row_stride, int64_t pixel_stride, int64_t channel_stride, uint32_t col, uint32_t y,
                                                uint32_t c) {
    return (int64_t)y * row_stride + (int64_t)col * pixel_stride + (int64_t)c * channel_stride;
}
// The dynamic LDS the wave form asks for a row of W samples (what decode8_lds_bytes returns: the estimator table of 256 or 512 rows
// of six words, two rows of int16 padded to whole blocks of 64), and the most a workgroup may ask for (DECODE_LDS_LIMIT).  A wider
// row is FELICS_E_UNSUPPORTED in every indexed call, on the host as on the device.
constexpr uint32_t INDEX_LDS_LIMIT = 160u * 1024u;
FELICS_IDX_HD inline uint64_t index_lds_bytes(uint32_t W, uint32_t color) {
    return (color ? 512u : 256u) * 6u * 4u + 2ull * (((uint64_t)W + 63u) & ~63ull) * 2u;
}
// The same for the 16-bit wave form (what decode16_lds_bytes returns: 512 cached estimator rows of sixteen words, their 512 tags, two
// rows of int32 padded to whole blocks of 64): the widest row is 16 128 samples.  For the host model of k_decode16_seg_views.
FELICS_IDX_HD constexpr uint64_t index16_lds_bytes(uint32_t W) { return 512u * 16u * 4u + 512u * 4u + 2ull * (((uint64_t)W + 63u) & ~63ull) * 4u; }

}  // namespace felics

#endif
