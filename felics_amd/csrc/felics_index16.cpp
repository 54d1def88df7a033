// felics_index16.cpp -- host side of the restart index of 16-bit streams (felics.h "Restart index: 16-bit streams", format version 2;
// DESIGN.md §3.4): felics_index16_size_max, felics_index16_build (the index of any 16-bit stream, from one pass of the host decoder
// and a replay of the estimator over the decoded samples) and felics_decompress_indexed16 (the stream decoded segment by segment, each from its
// checkpoint alone: the host model of k_decode16_seg, with the same checks in the same order) and felics_decompress_indexed16_view (the
// same walk written through a view's strides: the host model of k_decode16_seg_views).
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <new>
#include <vector>

#include "../../include/felics.h"
#include "felics_hostdec.h"
#include "felics_index.h"
#include "felics_viewcheck.h"

namespace {

using namespace felics;
using namespace felics_hostdec;

constexpr Options OPT16{65535u * 2u, 15};

void wr16(uint8_t *p, uint32_t v) {
    p[0] = (uint8_t)v;
    p[1] = (uint8_t)(v >> 8);
}
void wr32(uint8_t *p, uint32_t v) {
    wr16(p, v);
    wr16(p + 2, v >> 16);
}
void wr64(uint8_t *p, uint64_t v) {
    wr32(p, (uint32_t)v);
    wr32(p + 4, (uint32_t)(v >> 32));
}

// what a sample of a plane can be: Y (and gray) 0..65535, Co / Cg -65535..65535
bool in_plane_range(int32_t v, uint32_t color, uint32_t c) { return v <= 65535 && v >= (color && c ? -65535 : 0); }

// The header's claims against the stream and the caller (felics_decompress_with_header's checks, for a 16-bit stream): nothing is
// sized by a header the stream cannot back.
int check_stream16(const uint8_t *in, size_t len, felics_header &hdr) {
    const int rc = felics_read_header(in, len, &hdr);
    if (rc) return rc;
    if (hdr.pixel_depth != FELICS_DEPTH_16) return FELICS_E_UNSUPPORTED;
    const uint64_t npix = (uint64_t)hdr.width * hdr.height;
    if (npix > 0xFFFFFFFFull) return FELICS_E_INVALID_DIMENSIONS;
    const unsigned planes = hdr.color_type == FELICS_COLOR_RGB ? 3 : 1;
    const uint64_t body = len - FELICS_HEADER_BYTES;
    if (body < 8ull * planes) return FELICS_E_IO;
    if (npix > 2 && (npix - 2) * planes > (body - 8ull * planes) * 8ull) return FELICS_E_IO;
    return FELICS_OK;
}

// ycocg_to_rgb (color_transform.rs:20-26) of the planes, range-checked like try_into::<u16>(); dst (interleaved, or the gray frame)
// may be NULL (check only)
int store_rgb16(const std::vector<int32_t> (&ch)[3], unsigned planes, uint16_t *dst) {
    const size_t n = ch[0].size();
    for (size_t i = 0; i < n; i++) {
        int32_t v[3];
        if (planes == 1) {
            v[0] = ch[0][i];
        } else {
            const int32_t yv = ch[0][i], co = ch[1][i], cg = ch[2][i];
            const int32_t t = yv - cg / 2;
            v[1] = cg + t;
            v[2] = t - co / 2;
            v[0] = v[2] + co;
        }
        for (unsigned c = 0; c < planes; c++) {
            if (v[c] < 0 || v[c] > 65535) return FELICS_E_INVALID_VALUE;
            if (dst) dst[i * planes + c] = (uint16_t)v[c];
        }
    }
    return FELICS_OK;
}

// A 16-bit stream decoded through its version-2 index, segment by segment in (plane, segment) order, each from its checkpoint alone:
// what felics_decompress_indexed16 and felics_decompress_indexed16_view share, and the model of the kernels' walk -- the directory
// entry, the state rows (the table holds exactly the checkpoint's rows: what a segment loaded or touched is cleared behind it), the
// window samples, the two raw samples (j = 0), the walk, every decoded sample in range, done(c, s0, s1, plane c's samples) for the
// segment's pixels [s0, s1), then the end check.  hdr and L: the stream's header and the layout index16_header_check gave.  ch[c]:
// plane c, W * H samples.  The first failure is the code.
template <typename Done>
int walk_segments16(const uint8_t *in, size_t len, const uint8_t *index, size_t index_len, const Index16Layout &L, const felics_header &hdr,
                    std::vector<int32_t> (&ch)[3], Done done) {
    const uint32_t W = hdr.width, color = hdr.color_type, seg = idx_rd32(index + IDX_SEGPIX);
    const size_t npix = (size_t)W * hdr.height;
    try {
        Estimator est(OPT16);
        std::vector<uint32_t> touched(OPT16.max_context + 1, 0u);  // [ctx] != 0: the segment had an event of that context
        for (uint32_t c = 0; c < L.planes; c++) {
            ch[c].assign(npix, 0);
            int32_t *out = ch[c].data();
            for (uint32_t j = 0; j < std::max(L.K, 1u); j++) {
                uint64_t start, end, rows_off;
                uint32_t n_rows;
                if (index16_segment_bounds(index, L, c, j, len, index_len, start, end, rows_off, n_rows)) return FELICS_E_INVALID_INDEX;
                const uint8_t *rows = index + rows_off;
                int64_t prev = -1;
                for (uint32_t k = 0; k < n_rows; k++) {
                    const uint8_t *row = rows + (uint64_t)k * INDEX16_ROW_BYTES;
                    const uint32_t ctx = idx_rd32(row + 4 * INDEX16_ROW_CTX);
                    if (ctx >= index16_contexts(color, c) || (int64_t)ctx <= prev) return FELICS_E_INVALID_INDEX;
                    prev = ctx;
                    for (unsigned i = 0; i < 15; i++) est.row(ctx)[i] = idx_rd32(row + 4 * i);
                }
                const size_t s0 = (size_t)j * seg, s1 = std::min(npix, s0 + seg);
                if (L.K) {  // the 2 W samples in front of s0, range-checked; window positions in front of the plane are never looked at
                    const uint8_t *win = index + L.win_base + ((uint64_t)c * L.K + j) * L.win_bytes;
                    for (uint64_t s = 0; s < 2ull * W; s++) {
                        if (s0 + s < 2ull * W) continue;
                        const int32_t v = color ? (int32_t)idx_rd32(win + 4 * s) : (int32_t)idx_rd16(win + 2 * s);
                        if (!in_plane_range(v, color, c)) return FELICS_E_INVALID_INDEX;
                        out[s0 + s - 2ull * W] = v;
                    }
                }
                BitReader br(in, len, start);
                if (j == 0) {
                    const int32_t p0 = (int32_t)br.bits(32), p1 = (int32_t)br.bits(32);
                    if (br.failed()) return FELICS_E_IO;
                    if (npix > 0) out[0] = p0;
                    if (npix > 1) out[1] = p1;
                }
                if (s1 > s0) {
                    const int rc = decode_span(br, W, OPT16, est, out, std::max<size_t>(s0, 2), s1, touched.data());
                    if (rc) return rc;
                    for (size_t i = s0; i < s1; i++)
                        if (!in_plane_range(out[i], color, c)) return FELICS_E_INVALID_VALUE;
                    done(c, s0, s1, out);
                }
                if (br.pos() != end) return FELICS_E_INVALID_INDEX;  // the end check: exactly on the next checkpoint
                for (uint32_t k = 0; k < n_rows; k++)
                    memset(est.row(idx_rd32(rows + (uint64_t)k * INDEX16_ROW_BYTES + 4 * INDEX16_ROW_CTX)), 0, 15 * 4);
                for (uint32_t ctx = 0; ctx <= OPT16.max_context; ctx++)
                    if (touched[ctx]) {
                        touched[ctx] = 0;
                        memset(est.row(ctx), 0, 15 * 4);
                    }
            }
        }
    } catch (const std::bad_alloc &) {
        return FELICS_E_INVALID_DIMENSIONS;
    }
    return FELICS_OK;
}

// The needed segments of the non-empty region r (inside the image) of a 16-bit stream whose two headers passed their checks, in
// (plane, segment) order, each from its checkpoint alone -- the table is exactly the checkpoint's rows --, walked up to
// min(segment end, the pixel behind the region's last one): the walk of felics_decompress_region_indexed16 and
// felics_decompress_region_indexed16_view.  ch[c]: plane c of the crop (w * h samples); put(c, i, j, v): window sample (i, j) of
// plane c as it is decoded.  0 or the first failing segment's code.
template <typename Put>
int walk_region16(const uint8_t *in, size_t len, const uint8_t *index, size_t index_len, const Index16Layout &L, const felics_header &hdr,
                  const felics_region &r, std::vector<int32_t> (&ch)[3], Put put) {
    const uint32_t W = hdr.width, H = hdr.height, color = hdr.color_type;
    const size_t npix = (size_t)W * H, cpix = (size_t)r.w * r.h;
    const uint32_t seg = idx_rd32(index + IDX_SEGPIX);
    const uint64_t last = region_last(W, r);
    uint32_t jfirst, jlast;
    region_span(W, seg, r, jfirst, jlast);
    std::vector<int32_t> buf;
    int rc;
    try {
        Estimator est(OPT16);
        std::vector<uint32_t> touched(OPT16.max_context + 1, 0u);  // [ctx] != 0: the segment had an event of that context
        for (uint32_t c = 0; c < L.planes; c++) {
            ch[c].assign(cpix, 0);
            for (uint32_t j = jfirst; j <= jlast; j++) {
                if (!region_needs(W, npix, seg, r, j)) continue;
                uint64_t start, end, rows_off;
                uint32_t n_rows;
                if (index16_segment_bounds(index, L, c, j, len, index_len, start, end, rows_off, n_rows)) return FELICS_E_INVALID_INDEX;
                // the table: exactly the checkpoint's rows (it is all zero here: what a segment loaded or touched is cleared behind it)
                const uint8_t *rows = index + rows_off;
                int64_t prev = -1;
                for (uint32_t k = 0; k < n_rows; k++) {
                    const uint8_t *row = rows + (uint64_t)k * INDEX16_ROW_BYTES;
                    const uint32_t ctx = idx_rd32(row + 4 * INDEX16_ROW_CTX);
                    if (ctx >= index16_contexts(color, c) || (int64_t)ctx <= prev) return FELICS_E_INVALID_INDEX;
                    prev = ctx;
                    for (unsigned i = 0; i < 15; i++) est.row(ctx)[i] = idx_rd32(row + 4 * i);
                }
                const size_t s0 = (size_t)j * seg, s1 = std::min(npix, s0 + seg), stop = (size_t)std::min<uint64_t>(s1, last);
                // The walk's samples live in `buf`: whole rows from two rows above s0's on (the window's reach), up to `stop`.  The rows
                // dropped in front are an even count when s0's row is >= 2, none otherwise: the neighbour rule sees the same cases.
                const size_t y0 = s0 / W, base = y0 >= 2 ? (y0 - 2) * W : 0;
                buf.assign(stop - base, 0);
                int32_t *out = buf.data();
                const uint8_t *win = index + L.win_base + ((uint64_t)c * L.K + j) * L.win_bytes;
                for (uint64_t s = 0; s < 2ull * W; s++) {  // samples s0 - 2 W .. s0 - 1; those in front of the plane are never looked at
                    if (s0 + s < 2ull * W) continue;
                    const int32_t v = color ? (int32_t)idx_rd32(win + 4 * s) : (int32_t)idx_rd16(win + 2 * s);
                    if (!in_plane_range(v, color, c)) return FELICS_E_INVALID_INDEX;
                    out[s0 + s - 2ull * W - base] = v;
                }
                BitReader br(in, len, start);
                if (j == 0) {
                    const int32_t p0 = (int32_t)br.bits(32), p1 = (int32_t)br.bits(32);
                    if (br.failed()) return FELICS_E_IO;
                    out[0] = p0;
                    if (stop > 1) out[1] = p1;
                }
                rc = decode_span(br, W, OPT16, est, out, std::max<size_t>(s0, 2) - base, std::max<size_t>(stop, 2) - base, touched.data());
                if (rc) return rc;
                for (size_t i = s0; i < stop; i++) {
                    const int32_t v = out[i - base];
                    if (!in_plane_range(v, color, c)) return FELICS_E_INVALID_VALUE;
                    const size_t yy = i / W, xx = i - yy * W;
                    if (xx >= r.x && xx < (size_t)r.x + r.w && yy >= r.y) {
                        ch[c][(yy - r.y) * r.w + (xx - r.x)] = v;
                        put(c, (uint32_t)(xx - r.x), (uint32_t)(yy - r.y), v);
                    }
                }
                // the end check where the walk reached the segment's end; a walk that stops early has no bit position to stand on
                if (stop == s1 && br.pos() != end) return FELICS_E_INVALID_INDEX;
                for (uint32_t k = 0; k < n_rows; k++)
                    memset(est.row(idx_rd32(rows + (uint64_t)k * INDEX16_ROW_BYTES + 4 * INDEX16_ROW_CTX)), 0, 15 * 4);
                for (uint32_t ctx = 0; ctx <= OPT16.max_context; ctx++)
                    if (touched[ctx]) {
                        touched[ctx] = 0;
                        memset(est.row(ctx), 0, 15 * 4);
                    }
            }
        }
    } catch (const std::bad_alloc &) {
        return FELICS_E_INVALID_DIMENSIONS;
    }
    return FELICS_OK;
}

}  // namespace

extern "C" {

size_t felics_index_wide_size_max(uint32_t w, uint32_t h, int color, uint32_t segment_pixels) {
    if ((color != FELICS_COLOR_GRAY && color != FELICS_COLOR_RGB) || !index_segment_ok(segment_pixels)) return 0;
    const uint64_t npix = (uint64_t)w * h;
    if (npix > 0xFFFFFFFFull) return 0;
    const Index16Layout L = index16_layout(w, h, (uint32_t)color, segment_pixels);
    // a checkpoint's rows: contexts with an event in front of p0 (pixels 2 .. p0 - 1) and one at or behind it
    uint64_t rows = 0;
    for (uint32_t c = 0; c < L.planes; c++)
        for (uint32_t j = 1; j < L.K; j++) {
            const uint64_t p0 = (uint64_t)j * segment_pixels;
            rows += std::min<uint64_t>({p0 - 2, npix - p0, index16_contexts((uint32_t)color, c)});
        }
    return (size_t)(L.rows_base + rows * INDEX16_ROW_BYTES);
}

int felics_index_wide_build(const uint8_t *in, size_t len, uint32_t segment_pixels, uint8_t *index, size_t cap, size_t *index_len) {
    if (!index_len || (!in && len) || (!index && cap)) return FELICS_E_INVALID_ARGUMENT;
    *index_len = 0;
    felics_header hdr;
    int rc = check_stream16(in, len, hdr);
    if (rc) return rc;
    if (!index_segment_ok(segment_pixels)) return FELICS_E_INVALID_ARGUMENT;
    const uint32_t W = hdr.width, H = hdr.height, color = hdr.color_type;
    const Index16Layout L = index16_layout(W, H, color, segment_pixels);
    const size_t npix = (size_t)W * H;
    BitReader br(in, len, STREAM_HEADER_BITS);
    std::vector<uint8_t> head, rows;  // header | directory | windows, and the state rows behind them
    try {
        head.assign((size_t)L.rows_base, 0);
        memcpy(head.data(), "FLCX", 4);
        wr16(head.data() + IDX_VERSION, INDEX16_VERSION);
        head[IDX_COLOR] = (uint8_t)color;
        head[IDX_DEPTH] = FELICS_DEPTH_16;
        wr32(head.data() + IDX_WIDTH, W);
        wr32(head.data() + IDX_HEIGHT, H);
        wr32(head.data() + IDX_SEGPIX, segment_pixels);
        wr32(head.data() + IDX_K, L.K);
        std::vector<int32_t> ch[3];
        std::vector<uint32_t> last_event(OPT16.max_context + 1);
        std::vector<uint64_t> live((OPT16.max_context + 64) / 64);  // contexts with an event so far that may have another
        for (uint32_t c = 0; c < L.planes; c++) {
            const uint64_t plane_start = br.pos();
            const int32_t p0 = (int32_t)br.bits(32), p1 = (int32_t)br.bits(32);  // compression.rs:166-167
            if (br.failed()) return FELICS_E_IO;
            ch[c].assign(npix, 0);
            int32_t *out = ch[c].data();
            if (npix > 0) out[0] = p0;
            if (npix > 1) out[1] = p1;
            Estimator est(OPT16);
            std::fill(last_event.begin(), last_event.end(), 0u);  // (an event's pixel is never pixel 0)
            for (uint32_t j = 0; j < L.K; j++) {
                const size_t s0 = (size_t)j * segment_pixels, s1 = std::min(npix, s0 + segment_pixels);
                uint8_t *e = head.data() + INDEX_HEADER_BYTES + ((uint64_t)c * L.K + j) * INDEX16_ENTRY_BYTES;
                uint8_t *win = head.data() + L.win_base + ((uint64_t)c * L.K + j) * L.win_bytes;
                wr64(e + E16_BIT, j ? br.pos() : plane_start);
                for (uint64_t s = 0; s < 2ull * W; s++) {  // samples s0 - 2 W .. s0 - 1, zeros in front of the plane
                    if (s0 + s < 2ull * W) continue;
                    const int32_t v = out[s0 + s - 2ull * W];
                    if (color) wr32(win + 4 * s, (uint32_t)v);
                    else wr16(win + 2 * s, (uint32_t)v & 0xFFFFu);
                }
                rc = decode_span(br, W, OPT16, est, out, std::max<size_t>(s0, 2), s1, last_event.data());
                if (rc) return rc;
                for (size_t k = s0; k < s1; k++)
                    if (!in_plane_range(out[k], color, c)) return FELICS_E_INVALID_VALUE;
            }
            // The events again, from the decoded samples: pixel i is an event iff it lies outside [lo, hi] of its two neighbours, and
            // its operand is the distance to the nearer one minus one (compression.rs:200-230).  Replayed into a second estimator,
            // this yields every checkpoint's counters without a dense snapshot per checkpoint (7.9 MB each).
            Estimator rep(OPT16);
            std::fill(live.begin(), live.end(), 0ull);
            for (uint32_t j = 0; j < L.K; j++) {
                const size_t s0 = (size_t)j * segment_pixels, s1 = std::min(npix, s0 + segment_pixels);
                uint8_t *e = head.data() + INDEX_HEADER_BYTES + ((uint64_t)c * L.K + j) * INDEX16_ENTRY_BYTES;
                uint32_t n_rows = 0;
                wr64(e + E16_ROWS_OFF, L.rows_base + rows.size());
                if (j)  // canonical form: a row iff the context has an event in front of s0 (it is live) and one at or behind it
                    for (size_t wd = 0; wd < live.size(); wd++) {
                        uint64_t m = live[wd];
                        while (m) {
                            const uint32_t ctx = (uint32_t)(wd * 64 + (unsigned)__builtin_ctzll(m));
                            m &= m - 1;
                            if ((uint64_t)last_event[ctx] < s0) {  // never read again: dropped here and at every later checkpoint
                                live[wd] &= ~(1ull << (ctx & 63u));
                                continue;
                            }
                            const size_t at = rows.size();
                            rows.resize(at + INDEX16_ROW_BYTES);
                            for (unsigned k = 0; k < 15; k++) wr32(rows.data() + at + 4 * k, rep.row(ctx)[k]);
                            wr32(rows.data() + at + 4 * INDEX16_ROW_CTX, ctx);
                            n_rows++;
                        }
                    }
                wr32(e + E16_NROWS, n_rows);
                uint32_t x = (uint32_t)(std::max<size_t>(s0, 2) % W), y = (uint32_t)(std::max<size_t>(s0, 2) / W);
                for (size_t i = std::max<size_t>(s0, 2); i < s1; i++) {
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
                    const int64_t v1 = out[a], v2 = out[b], hi = std::max(v1, v2), lo = std::min(v1, v2), pv = out[i];
                    if (pv > hi || pv < lo) {
                        const uint32_t ctx = (uint32_t)(hi - lo);
                        rep.update(ctx, (uint32_t)(pv > hi ? pv - hi - 1 : lo - pv - 1));
                        live[ctx >> 6] |= 1ull << (ctx & 63u);
                    }
                    if (++x == W) {
                        x = 0;
                        y++;
                    }
                }
            }
            wr64(head.data() + IDX_PLANE_END + 8 * c, br.pos());
        }
        if ((rc = store_rgb16(ch, L.planes, nullptr)) != 0) return rc;
    } catch (const std::bad_alloc &) {
        return FELICS_E_INVALID_DIMENSIONS;
    }
    // the index names the stream's last byte: bytes behind the last code are not a stream this index can describe
    if ((br.pos() + 7u) / 8u != len) return FELICS_E_INVALID_ARGUMENT;
    const uint64_t total = L.rows_base + rows.size();
    wr64(head.data() + IDX16_TOTAL, total);
    *index_len = (size_t)total;
    if (total > cap) return FELICS_E_BUFFER_TOO_SMALL;
    memcpy(index, head.data(), head.size());
    if (!rows.empty()) memcpy(index + head.size(), rows.data(), rows.size());
    return FELICS_OK;
}

int felics_decompress_indexed_wide(const uint8_t *in, size_t len, const uint8_t *index, size_t index_len, void *pixels, size_t pixels_cap,
                                felics_header *hdr_out) {
    if ((!in && len) || (!index && index_len)) return FELICS_E_INVALID_ARGUMENT;
    felics_header hdr;
    int rc = check_stream16(in, len, hdr);
    if (hdr_out && (rc == FELICS_OK || rc == FELICS_E_UNSUPPORTED)) *hdr_out = hdr;
    if (rc) return rc;
    const uint32_t W = hdr.width, H = hdr.height, color = hdr.color_type;
    const size_t npix = (size_t)W * H;
    const unsigned planes = color ? 3 : 1;
    if ((uint64_t)npix * planes * 2 > pixels_cap) return FELICS_E_BUFFER_TOO_SMALL;
    if (npix && !pixels) return FELICS_E_INVALID_ARGUMENT;
    Index16Layout L;
    if (index_len < INDEX_HEADER_BYTES || index16_header_check(index, color, W, H, len, index_len, L)) return FELICS_E_INVALID_INDEX;
    std::vector<int32_t> ch[3];
    rc = walk_segments16(in, len, index, index_len, L, hdr, ch, [](uint32_t, size_t, size_t, const int32_t *) {});
    if (rc) return rc;
    return store_rgb16(ch, planes, (uint16_t *)pixels);
}

int felics_decompress_region_indexed_wide(const uint8_t *in, size_t len, const uint8_t *index, size_t index_len, const felics_region *rp,
                                          void *pixels, size_t pixels_cap, felics_header *hdr_out) {
    if ((!in && len) || (!index && index_len) || !rp) return FELICS_E_INVALID_ARGUMENT;
    felics_header hdr;
    int rc = check_stream16(in, len, hdr);
    if (hdr_out && (rc == FELICS_OK || rc == FELICS_E_UNSUPPORTED)) *hdr_out = hdr;
    if (rc) return rc;
    const uint32_t W = hdr.width, H = hdr.height, color = hdr.color_type;
    const felics_region r = *rp;
    if (!region_inside(W, H, r)) return FELICS_E_INVALID_ARGUMENT;
    const size_t cpix = (size_t)r.w * r.h;
    const unsigned planes = color ? 3 : 1;
    if ((uint64_t)cpix * planes * 2 > pixels_cap) return FELICS_E_BUFFER_TOO_SMALL;
    if (cpix && !pixels) return FELICS_E_INVALID_ARGUMENT;
    Index16Layout L;
    if (index_len < INDEX_HEADER_BYTES || index16_header_check(index, color, W, H, len, index_len, L)) return FELICS_E_INVALID_INDEX;
    if (region_empty(r)) return FELICS_OK;
    std::vector<int32_t> ch[3];
    if ((rc = walk_region16(in, len, index, index_len, L, hdr, r, ch, [](uint32_t, uint32_t, uint32_t, int32_t) {})) != 0) return rc;
    return store_rgb16(ch, planes, (uint16_t *)pixels);
}

int felics_decompress_region_indexed_view_wide(const uint8_t *in, size_t len, const uint8_t *index, size_t index_len, const felics_region *rp,
                                               const felics_view *view, felics_header *hdr_out) {
    if ((!in && len) || (!index && index_len) || !rp || !view) return FELICS_E_INVALID_ARGUMENT;
    int rc = view_writable_code(*view);
    if (rc) return rc;
    const felics_region r = *rp;
    if (view->width != r.w || view->height != r.h) return FELICS_E_INVALID_ARGUMENT;
    // the per-stream codes of felics_decompress_region_views_device_indexed16, in its order; then the region's
    felics_header hdr;
    rc = felics_read_header(in, len, &hdr);
    if (hdr_out) *hdr_out = rc ? felics_header{} : hdr;
    if (rc) return rc;
    const uint32_t W = hdr.width, H = hdr.height, color = hdr.color_type;
    const unsigned planes = color ? 3 : 1;
    if ((uint64_t)W * H > 0xFFFFFFFFull) return FELICS_E_INVALID_DIMENSIONS;
    const size_t npix = (size_t)W * H, cpix = (size_t)r.w * r.h;
    // (k_read_headers' rule: two raw 32-bit samples per plane, then at least one flag bit per pixel, padded to a byte)
    const uint64_t bits = (uint64_t)planes * (64u + (npix > 2 ? npix - 2 : 0));
    if (len - FELICS_HEADER_BYTES < (bits + 7) / 8) return FELICS_E_IO;
    if (hdr.pixel_depth != FELICS_DEPTH_16) return FELICS_E_UNSUPPORTED;
    if (index16_lds_bytes(W) > INDEX_LDS_LIMIT) return FELICS_E_UNSUPPORTED;  // what the wave form cannot hold, the model refuses too
    Index16Layout L;
    if (index_len < INDEX_HEADER_BYTES || index16_header_check(index, color, W, H, len, index_len, L)) return FELICS_E_INVALID_INDEX;
    if (!region_inside(W, H, r)) return FELICS_E_INVALID_ARGUMENT;
    if ((int)color != view->color || (int)hdr.pixel_depth != view->depth) return FELICS_E_INVALID_DIMENSIONS;
    if (region_empty(r)) return FELICS_OK;
    uint8_t *data = (uint8_t *)const_cast<void *>(view->data);
    const int64_t rs = view->row_stride, ps = view->pixel_stride, cs = color ? view->channel_stride : 0;
    auto sample = [&](uint32_t i, uint32_t j, unsigned c) {  // where the kernel's sink (gray) and the strided conversion (RGB) store window sample (i, j)
        return reinterpret_cast<uint16_t *>(data + view_sample_offset(rs, ps, cs, i, j, c));
    };
    std::vector<int32_t> ch[3];
    // gray: a window sample through the view, as the kernel's sink stores it (an RGB plane waits for the other two)
    rc = walk_region16(in, len, index, index_len, L, hdr, r, ch, [&](uint32_t, uint32_t i, uint32_t j, int32_t v) {
        if (!color) *sample(i, j, 0) = (uint16_t)v;
    });
    if (rc || !color) return rc;
    try {
        std::vector<uint16_t> rgb(cpix * 3);  // (converted and range-checked first: a region that fails here leaves the view as it was)
        if ((rc = store_rgb16(ch, planes, rgb.data())) != 0) return rc;
        for (size_t i = 0; i < cpix; i++)
            for (unsigned c = 0; c < 3; c++) *sample((uint32_t)(i % r.w), (uint32_t)(i / r.w), c) = rgb[i * 3 + c];
    } catch (const std::bad_alloc &) {
        return FELICS_E_INVALID_DIMENSIONS;
    }
    return FELICS_OK;
}

int felics_decompress_indexed_view_wide(const uint8_t *in, size_t len, const uint8_t *index, size_t index_len, const felics_view *view,
                                        felics_header *hdr_out) {
    if ((!in && len) || (!index && index_len) || !view) return FELICS_E_INVALID_ARGUMENT;
    int rc = view_writable_code(*view);
    if (rc) return rc;
    // the per-stream codes of felics_decompress_views_device_indexed16, in its order
    felics_header hdr;
    rc = felics_read_header(in, len, &hdr);
    if (hdr_out) *hdr_out = rc ? felics_header{} : hdr;
    if (rc) return rc;
    const uint32_t W = hdr.width, H = hdr.height, color = hdr.color_type;
    const unsigned planes = color ? 3 : 1;
    if ((uint64_t)W * H > 0xFFFFFFFFull) return FELICS_E_INVALID_DIMENSIONS;
    const size_t npix = (size_t)W * H;
    // (k_read_headers' rule: two raw 32-bit samples per plane, then at least one flag bit per pixel, padded to a byte)
    const uint64_t bits = (uint64_t)planes * (64u + (npix > 2 ? npix - 2 : 0));
    if (len - FELICS_HEADER_BYTES < (bits + 7) / 8) return FELICS_E_IO;
    if (hdr.pixel_depth != FELICS_DEPTH_16) return FELICS_E_UNSUPPORTED;
    if (index16_lds_bytes(W) > INDEX_LDS_LIMIT) return FELICS_E_UNSUPPORTED;  // what the wave form cannot hold, the model refuses too
    if ((int)color != view->color || (int)hdr.pixel_depth != view->depth || W != view->width || H != view->height) return FELICS_E_INVALID_DIMENSIONS;
    Index16Layout L;
    if (index_len < INDEX_HEADER_BYTES || index16_header_check(index, color, W, H, len, index_len, L)) return FELICS_E_INVALID_INDEX;
    uint8_t *data = (uint8_t *)const_cast<void *>(view->data);
    const int64_t rs = view->row_stride, ps = view->pixel_stride, cs = color ? view->channel_stride : 0;
    auto sample = [&](size_t i, unsigned c) {  // where the kernel's sink (gray) and the strided conversion (RGB) store pixel i
        const uint32_t y = (uint32_t)(i / W), x = (uint32_t)(i - (size_t)y * W);
        return reinterpret_cast<uint16_t *>(data + view_sample_offset(rs, ps, cs, x, y, c));
    };
    std::vector<int32_t> ch[3];
    // gray: a segment's samples through the view, as the kernel's sink stores them (an RGB plane waits for the other two)
    rc = walk_segments16(in, len, index, index_len, L, hdr, ch, [&](uint32_t, size_t s0, size_t s1, const int32_t *out) {
        for (size_t i = s0; i < s1 && !color; i++) *sample(i, 0) = (uint16_t)out[i];
    });
    if (rc || !color) return rc;
    try {
        std::vector<uint16_t> rgb(npix * 3);  // (converted and range-checked first: a stream that fails here leaves the view as it was)
        if ((rc = store_rgb16(ch, planes, rgb.data())) != 0) return rc;
        for (size_t i = 0; i < npix; i++)
            for (unsigned c = 0; c < 3; c++) *sample(i, c) = rgb[i * 3 + c];
    } catch (const std::bad_alloc &) {
        return FELICS_E_INVALID_DIMENSIONS;
    }
    return FELICS_OK;
}

}  // extern "C"
