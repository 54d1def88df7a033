// felics_index.cpp -- host side of the restart index (felics.h): felics_index_size, felics_index_build (the index
// of any 8-bit stream, from one pass of the host decoder) and felics_decompress_indexed (the stream decoded segment by segment,
// each from its checkpoint alone: the host model of k_decode8_seg, with the same checks in the same order) and
// felics_decompress_indexed_view (the same walk written through a view's strides: the host model of k_decode8_seg_views).
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

constexpr Options OPT8{255u * 2u, 6};

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

// what a sample of a plane can be: Y (and gray) 0..255, Co / Cg -255..255
bool in_plane_range(int32_t v, uint32_t color, uint32_t c) { return v <= 255 && v >= (color && c ? -255 : 0); }

// The header's claims against the stream and the caller (felics_decompress_with_header's checks, for an 8-bit stream): nothing is
// sized by a header the stream cannot back.
int check_stream(const uint8_t *in, size_t len, felics_header &hdr) {
    const int rc = felics_read_header(in, len, &hdr);
    if (rc) return rc;
    if (hdr.pixel_depth != FELICS_DEPTH_8) return FELICS_E_UNSUPPORTED;
    const uint64_t npix = (uint64_t)hdr.width * hdr.height;
    if (npix > 0xFFFFFFFFull) return FELICS_E_INVALID_DIMENSIONS;
    const unsigned planes = hdr.color_type == FELICS_COLOR_RGB ? 3 : 1;
    const uint64_t body = len - FELICS_HEADER_BYTES;
    if (body < 8ull * planes) return FELICS_E_IO;
    if (npix > 2 && (npix - 2) * planes > (body - 8ull * planes) * 8ull) return FELICS_E_IO;
    return FELICS_OK;
}

// ycocg_to_rgb (color_transform.rs:20-26) of the planes, range-checked like try_into::<u8>(): put(i, c, v) for sample c of pixel i, in
// pixel order, up to the first one out of range
template <typename Put>
int convert_rgb8(const std::vector<int32_t> (&ch)[3], unsigned planes, Put put) {
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
            if (v[c] < 0 || v[c] > 255) return FELICS_E_INVALID_VALUE;
            put(i, c, (uint8_t)v[c]);
        }
    }
    return FELICS_OK;
}

// ... to a dense interleaved frame; dst may be NULL (check only)
int store_rgb8(const std::vector<int32_t> (&ch)[3], unsigned planes, uint8_t *dst) {
    return convert_rgb8(ch, planes, [&](size_t i, unsigned c, uint8_t v) {
        if (dst) dst[i * planes + c] = v;
    });
}

// Everything a segment starts from but its bit position comes out of checkpoint (c, j) (K >= 1): the counters into `est`, and the 2 W
// samples in front of s0 = the segment's first pixel, range-checked, to the caller's samples (out[0] is pixel `base`, base <= s0 - 2 W
// where that is a pixel of the plane).  Window positions in front of the plane are never looked at.  0, or FELICS_E_INVALID_INDEX.
int load_checkpoint(const uint8_t *index, const IndexLayout &L, uint32_t color, uint32_t c, uint32_t j, uint32_t W, size_t s0, Estimator &est,
                    int32_t *out, size_t base) {
    const uint8_t *cp = index + INDEX_HEADER_BYTES + ((uint64_t)c * L.K + j) * L.cp_bytes;
    const uint32_t stored = (color ? OPT8.max_context + 1 : 256u) * 6;  // (gray has contexts 0 .. 255)
    for (uint32_t i = 0; i < (OPT8.max_context + 1) * 6; i++) est.row(0)[i] = i < stored ? idx_rd16(cp + CP_STATE_OFF + 2 * i) : 0u;
    for (uint64_t s = 0; s < 2ull * W; s++) {
        if (s0 + s < 2ull * W) continue;
        const int32_t v = color ? (int32_t)(int16_t)idx_rd16(cp + L.win_off + 2 * s) : (int32_t)cp[L.win_off + s];
        if (!in_plane_range(v, color, c)) return FELICS_E_INVALID_INDEX;
        out[s0 + s - 2ull * W - base] = v;
    }
    return FELICS_OK;
}

// The needed segments of the non-empty region r (inside the image) of an 8-bit stream whose two headers passed their checks, in
// (plane, segment) order, each from its checkpoint alone, walked up to min(segment end, the pixel behind the region's last one):
// the walk of felics_decompress_region_indexed and felics_decompress_region_indexed_view.  ch[c]: plane c of the crop (w * h samples);
// put(c, i, j, v): window sample (i, j) of plane c as it is decoded.  0 or the first failing segment's code.
template <typename Put>
int walk_region8(const uint8_t *in, size_t len, const uint8_t *index, const IndexLayout &L, const felics_header &hdr, const felics_region &r,
                 std::vector<int32_t> (&ch)[3], Put put) {
    const uint32_t W = hdr.width, H = hdr.height, color = hdr.color_type;
    const size_t npix = (size_t)W * H, cpix = (size_t)r.w * r.h;
    const uint32_t seg = idx_rd32(index + IDX_SEGPIX);
    const uint64_t last = region_last(W, r);
    uint32_t jfirst, jlast;
    region_span(W, seg, r, jfirst, jlast);
    std::vector<int32_t> buf;
    int rc;
    try {
        Estimator est(OPT8);
        for (uint32_t c = 0; c < L.planes; c++) {
            ch[c].assign(cpix, 0);
            for (uint32_t j = jfirst; j <= jlast; j++) {
                if (!region_needs(W, npix, seg, r, j)) continue;
                uint64_t start, end;
                if (index_segment_bounds(index, L, c, j, len, start, end)) return FELICS_E_INVALID_INDEX;
                BitReader br(in, len, start);
                const size_t s0 = (size_t)j * seg, s1 = std::min(npix, s0 + seg), stop = (size_t)std::min<uint64_t>(s1, last);
                // The walk's samples live in `buf`: whole rows from two rows above s0's on (the window's reach), up to `stop`.  The rows
                // dropped in front are an even count when s0's row is >= 2, none otherwise: the neighbour rule sees the same cases.
                const size_t y0 = s0 / W, base = y0 >= 2 ? (y0 - 2) * W : 0;
                buf.assign(stop - base, 0);
                int32_t *out = buf.data();
                if ((rc = load_checkpoint(index, L, color, c, j, W, s0, est, out, base)) != 0) return rc;
                if (j == 0) {
                    const int32_t p0 = (int32_t)br.bits(32), p1 = (int32_t)br.bits(32);
                    if (br.failed()) return FELICS_E_IO;
                    out[0] = p0;
                    if (stop > 1) out[1] = p1;
                }
                rc = decode_span(br, W, OPT8, est, out, std::max<size_t>(s0, 2) - base, std::max<size_t>(stop, 2) - base, nullptr);
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
            }
        }
    } catch (const std::bad_alloc &) {
        return FELICS_E_INVALID_DIMENSIONS;
    }
    return FELICS_OK;
}

}  // namespace

extern "C" {

size_t felics_index_size(uint32_t w, uint32_t h, int color, int depth, uint32_t segment_pixels) {
    if (depth != FELICS_DEPTH_8 || (color != FELICS_COLOR_GRAY && color != FELICS_COLOR_RGB) || !index_segment_ok(segment_pixels)) return 0;
    if ((uint64_t)w * h > 0xFFFFFFFFull) return 0;
    return (size_t)index_layout(w, h, (uint32_t)color, segment_pixels).total;
}

int felics_index_build(const uint8_t *in, size_t len, uint32_t segment_pixels, uint8_t *index, size_t cap, size_t *index_len) {
    if (!index_len || (!in && len) || (!index && cap)) return FELICS_E_INVALID_ARGUMENT;
    *index_len = 0;
    felics_header hdr;
    int rc = check_stream(in, len, hdr);
    if (rc) return rc;
    if (!index_segment_ok(segment_pixels)) return FELICS_E_INVALID_ARGUMENT;
    const uint32_t W = hdr.width, H = hdr.height, color = hdr.color_type;
    const IndexLayout L = index_layout(W, H, color, segment_pixels);
    *index_len = (size_t)L.total;
    if (L.total > cap) return FELICS_E_BUFFER_TOO_SMALL;
    memset(index, 0, (size_t)L.total);
    memcpy(index, "FLCX", 4);
    wr16(index + IDX_VERSION, INDEX_VERSION);
    index[IDX_COLOR] = (uint8_t)color;
    index[IDX_DEPTH] = FELICS_DEPTH_8;
    wr32(index + IDX_WIDTH, W);
    wr32(index + IDX_HEIGHT, H);
    wr32(index + IDX_SEGPIX, segment_pixels);
    wr32(index + IDX_K, L.K);
    const size_t npix = (size_t)W * H;
    BitReader br(in, len, STREAM_HEADER_BITS);
    std::vector<int32_t> ch[3];
    std::vector<uint32_t> last_event(OPT8.max_context + 1);
    const uint32_t nrows = color ? OPT8.max_context + 1 : 256u;  // contexts a plane of in-range samples can have (the stored row 511 stays zero)
    try {
        for (uint32_t c = 0; c < L.planes; c++) {
            const uint64_t plane_start = br.pos();
            const int32_t p0 = (int32_t)br.bits(32), p1 = (int32_t)br.bits(32);  // compression.rs:166-167
            if (br.failed()) return FELICS_E_IO;
            ch[c].assign(npix, 0);
            int32_t *out = ch[c].data();
            if (npix > 0) out[0] = p0;
            if (npix > 1) out[1] = p1;
            Estimator est(OPT8);
            std::fill(last_event.begin(), last_event.end(), 0u);  // (an event's pixel is never pixel 0)
            uint8_t *cps = index + INDEX_HEADER_BYTES + (uint64_t)c * L.K * L.cp_bytes;
            for (uint32_t j = 0; j < L.K; j++) {
                const size_t s0 = (size_t)j * segment_pixels, s1 = std::min(npix, s0 + segment_pixels);
                uint8_t *cp = cps + (uint64_t)j * L.cp_bytes;
                wr64(cp, j ? br.pos() : plane_start);
                if (j)
                    for (uint32_t ctx = 0; ctx < nrows; ctx++)
                        for (unsigned k = 0; k < 6; k++) {
                            const uint32_t v = est.row(ctx)[k];
                            if (v > 0xFFFFu) return FELICS_E_UNSUPPORTED;  // never truncated (no valid 8-bit plane gets here)
                            wr16(cp + CP_STATE_OFF + (ctx * 6 + k) * 2, v);
                        }
                for (uint64_t s = 0; s < 2ull * W; s++) {  // samples s0 - 2 W .. s0 - 1, zeros in front of the plane
                    if (s0 + s < 2ull * W) continue;
                    const int32_t v = out[s0 + s - 2ull * W];
                    if (color) wr16(cp + L.win_off + 2 * s, (uint32_t)v & 0xFFFFu);
                    else cp[L.win_off + s] = (uint8_t)v;
                }
                rc = decode_span(br, W, OPT8, est, out, std::max<size_t>(s0, 2), s1, last_event.data());
                if (rc) return rc;
                for (size_t i = s0; i < s1; i++)
                    if (!in_plane_range(out[i], color, c)) return FELICS_E_INVALID_VALUE;
            }
            // canonical form: a context with no event at or behind a checkpoint is never read again -- its state is stored as zeros
            for (uint32_t j = 1; j < L.K; j++)
                for (uint32_t ctx = 0; ctx < nrows; ctx++)
                    if ((uint64_t)last_event[ctx] < (uint64_t)j * segment_pixels)
                        memset(cps + (uint64_t)j * L.cp_bytes + CP_STATE_OFF + ctx * 12, 0, 12);
            wr64(index + IDX_PLANE_END + 8 * c, br.pos());
        }
    } catch (const std::bad_alloc &) {
        return FELICS_E_INVALID_DIMENSIONS;
    }
    if ((rc = store_rgb8(ch, L.planes, nullptr)) != 0) return rc;
    // the index names the stream's last byte: bytes behind the last code are not a stream this index can describe
    if ((br.pos() + 7u) / 8u != len) return FELICS_E_INVALID_ARGUMENT;
    return FELICS_OK;
}

int felics_decompress_indexed(const uint8_t *in, size_t len, const uint8_t *index, size_t index_len, void *pixels, size_t pixels_cap,
                              felics_header *hdr_out) {
    if ((!in && len) || (!index && index_len)) return FELICS_E_INVALID_ARGUMENT;
    felics_header hdr;
    int rc = check_stream(in, len, hdr);
    if (hdr_out && (rc == FELICS_OK || rc == FELICS_E_UNSUPPORTED)) *hdr_out = hdr;
    if (rc) return rc;
    const uint32_t W = hdr.width, H = hdr.height, color = hdr.color_type;
    const size_t npix = (size_t)W * H;
    const unsigned planes = color ? 3 : 1;
    if ((uint64_t)npix * planes > pixels_cap) return FELICS_E_BUFFER_TOO_SMALL;
    if (npix && !pixels) return FELICS_E_INVALID_ARGUMENT;
    IndexLayout L;
    if (index_len < INDEX_HEADER_BYTES || index_header_check(index, color, W, H, len, L) || L.total != index_len) return FELICS_E_INVALID_INDEX;
    const uint32_t seg = idx_rd32(index + IDX_SEGPIX);
    std::vector<int32_t> ch[3];
    try {
        Estimator est(OPT8);
        for (uint32_t c = 0; c < L.planes; c++) {
            ch[c].assign(npix, 0);
            int32_t *out = ch[c].data();
            for (uint32_t j = 0; j < std::max(L.K, 1u); j++) {
                uint64_t start, end;
                if (index_segment_bounds(index, L, c, j, len, start, end)) return FELICS_E_INVALID_INDEX;
                // everything a segment starts from comes out of its checkpoint: bit position, table, the 2 W samples in front of it
                BitReader br(in, len, start);
                const size_t s0 = (size_t)j * seg, s1 = std::min(npix, s0 + seg);
                if (L.K && (rc = load_checkpoint(index, L, color, c, j, W, s0, est, out, 0)) != 0) return rc;
                if (j == 0) {
                    const int32_t p0 = (int32_t)br.bits(32), p1 = (int32_t)br.bits(32);
                    if (br.failed()) return FELICS_E_IO;
                    if (npix > 0) out[0] = p0;
                    if (npix > 1) out[1] = p1;
                }
                if (s1 > s0) {
                    rc = decode_span(br, W, OPT8, est, out, std::max<size_t>(s0, 2), s1, nullptr);
                    if (rc) return rc;
                    for (size_t i = s0; i < s1; i++)
                        if (!in_plane_range(out[i], color, c)) return FELICS_E_INVALID_VALUE;
                }
                if (br.pos() != end) return FELICS_E_INVALID_INDEX;  // the end check: exactly on the next checkpoint
            }
        }
    } catch (const std::bad_alloc &) {
        return FELICS_E_INVALID_DIMENSIONS;
    }
    return store_rgb8(ch, planes, (uint8_t *)pixels);
}

int felics_decompress_indexed_view(const uint8_t *in, size_t len, const uint8_t *index, size_t index_len, const felics_view *view,
                                   felics_header *hdr_out) {
    if ((!in && len) || (!index && index_len) || !view) return FELICS_E_INVALID_ARGUMENT;
    int rc = view_writable_code(*view);
    if (rc) return rc;
    // the per-stream codes of felics_decompress_views_device_indexed, in its order
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
    if (hdr.pixel_depth != FELICS_DEPTH_8) return FELICS_E_UNSUPPORTED;
    if (index_lds_bytes(W, color) > INDEX_LDS_LIMIT) return FELICS_E_UNSUPPORTED;  // what the wave form cannot hold, the model refuses too
    if ((int)color != view->color || (int)hdr.pixel_depth != view->depth || W != view->width || H != view->height) return FELICS_E_INVALID_DIMENSIONS;
    IndexLayout L;
    if (index_len < INDEX_HEADER_BYTES || index_header_check(index, color, W, H, len, L) || L.total != index_len) return FELICS_E_INVALID_INDEX;
    const uint32_t seg = idx_rd32(index + IDX_SEGPIX);
    uint8_t *data = (uint8_t *)const_cast<void *>(view->data);
    const int64_t rs = view->row_stride, ps = view->pixel_stride, cs = color ? view->channel_stride : 0;
    std::vector<int32_t> ch[3];
    try {
        Estimator est(OPT8);
        for (uint32_t c = 0; c < L.planes; c++) {
            ch[c].assign(npix, 0);
            int32_t *out = ch[c].data();
            for (uint32_t j = 0; j < std::max(L.K, 1u); j++) {
                uint64_t start, end;
                if (index_segment_bounds(index, L, c, j, len, start, end)) return FELICS_E_INVALID_INDEX;
                BitReader br(in, len, start);
                const size_t s0 = (size_t)j * seg, s1 = std::min(npix, s0 + seg);
                if (L.K && (rc = load_checkpoint(index, L, color, c, j, W, s0, est, out, 0)) != 0) return rc;
                if (j == 0) {
                    const int32_t p0 = (int32_t)br.bits(32), p1 = (int32_t)br.bits(32);
                    if (br.failed()) return FELICS_E_IO;
                    if (npix > 0) out[0] = p0;
                    if (npix > 1) out[1] = p1;
                }
                if (s1 > s0) {
                    rc = decode_span(br, W, OPT8, est, out, std::max<size_t>(s0, 2), s1, nullptr);
                    if (rc) return rc;
                    for (size_t i = s0; i < s1; i++)
                        if (!in_plane_range(out[i], color, c)) return FELICS_E_INVALID_VALUE;
                    // gray: the segment's samples through the view, as the kernel's sink stores them (an RGB plane waits for the other two)
                    for (size_t i = s0; i < s1 && !color; i++) {
                        const uint32_t y = (uint32_t)(i / W), x = (uint32_t)(i - (size_t)y * W);
                        data[view_sample_offset(rs, ps, 0, x, y, 0)] = (uint8_t)out[i];
                    }
                }
                if (br.pos() != end) return FELICS_E_INVALID_INDEX;  // the end check: exactly on the next checkpoint
            }
        }
    } catch (const std::bad_alloc &) {
        return FELICS_E_INVALID_DIMENSIONS;
    }
    if (!color) return FELICS_OK;
    if ((rc = store_rgb8(ch, planes, nullptr)) != 0) return rc;  // (checked first: a stream that fails here leaves the view as it was)
    return convert_rgb8(ch, planes, [&](size_t i, unsigned c, uint8_t v) {
        const uint32_t y = (uint32_t)(i / W), x = (uint32_t)(i - (size_t)y * W);
        data[view_sample_offset(rs, ps, cs, x, y, c)] = v;
    });
}

int felics_region_segments(uint32_t W, uint32_t H, uint32_t segment_pixels, const felics_region *r, uint32_t *segs, size_t cap, size_t *count) {
    if (!r || !count || (!segs && cap)) return FELICS_E_INVALID_ARGUMENT;
    *count = 0;
    const uint64_t npix = (uint64_t)W * H;
    if (!index_segment_ok(segment_pixels) || npix > 0xFFFFFFFFull || !region_inside(W, H, *r)) return FELICS_E_INVALID_ARGUMENT;
    if (region_empty(*r)) return FELICS_OK;
    uint32_t first, last;
    region_span(W, segment_pixels, *r, first, last);
    size_t n = 0;
    for (uint32_t j = first; j <= last; j++)
        if (region_needs(W, npix, segment_pixels, *r, j)) {
            if (n < cap) segs[n] = j;
            n++;
        }
    *count = n;
    return n > cap ? FELICS_E_BUFFER_TOO_SMALL : FELICS_OK;
}

int felics_decompress_region_indexed(const uint8_t *in, size_t len, const uint8_t *index, size_t index_len, const felics_region *rp, void *pixels,
                                     size_t pixels_cap, felics_header *hdr_out) {
    if ((!in && len) || (!index && index_len) || !rp) return FELICS_E_INVALID_ARGUMENT;
    felics_header hdr;
    int rc = check_stream(in, len, hdr);
    if (hdr_out && (rc == FELICS_OK || rc == FELICS_E_UNSUPPORTED)) *hdr_out = hdr;
    if (rc) return rc;
    const uint32_t W = hdr.width, H = hdr.height, color = hdr.color_type;
    const felics_region r = *rp;
    if (!region_inside(W, H, r)) return FELICS_E_INVALID_ARGUMENT;
    const size_t cpix = (size_t)r.w * r.h;
    const unsigned planes = color ? 3 : 1;
    if ((uint64_t)cpix * planes > pixels_cap) return FELICS_E_BUFFER_TOO_SMALL;
    if (cpix && !pixels) return FELICS_E_INVALID_ARGUMENT;
    IndexLayout L;
    if (index_len < INDEX_HEADER_BYTES || index_header_check(index, color, W, H, len, L) || L.total != index_len) return FELICS_E_INVALID_INDEX;
    if (region_empty(r)) return FELICS_OK;
    std::vector<int32_t> ch[3];
    if ((rc = walk_region8(in, len, index, L, hdr, r, ch, [](uint32_t, uint32_t, uint32_t, int32_t) {})) != 0) return rc;
    return store_rgb8(ch, planes, (uint8_t *)pixels);
}

int felics_decompress_region_indexed_view(const uint8_t *in, size_t len, const uint8_t *index, size_t index_len, const felics_region *rp,
                                          const felics_view *view, felics_header *hdr_out) {
    if ((!in && len) || (!index && index_len) || !rp || !view) return FELICS_E_INVALID_ARGUMENT;
    int rc = view_writable_code(*view);
    if (rc) return rc;
    const felics_region r = *rp;
    if (view->width != r.w || view->height != r.h) return FELICS_E_INVALID_ARGUMENT;
    // the per-stream codes of felics_decompress_region_views_device_indexed, in its order; then the region's
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
    if (hdr.pixel_depth != FELICS_DEPTH_8) return FELICS_E_UNSUPPORTED;
    if (index_lds_bytes(W, color) > INDEX_LDS_LIMIT) return FELICS_E_UNSUPPORTED;  // what the wave form cannot hold, the model refuses too
    IndexLayout L;
    if (index_len < INDEX_HEADER_BYTES || index_header_check(index, color, W, H, len, L) || L.total != index_len) return FELICS_E_INVALID_INDEX;
    if (!region_inside(W, H, r)) return FELICS_E_INVALID_ARGUMENT;
    if ((int)color != view->color || (int)hdr.pixel_depth != view->depth) return FELICS_E_INVALID_DIMENSIONS;
    if (region_empty(r)) return FELICS_OK;
    uint8_t *data = (uint8_t *)const_cast<void *>(view->data);
    const int64_t rs = view->row_stride, ps = view->pixel_stride, cs = color ? view->channel_stride : 0;
    std::vector<int32_t> ch[3];
    // gray: a window sample through the view, as the kernel's sink stores it (an RGB plane waits for the other two)
    rc = walk_region8(in, len, index, L, hdr, r, ch, [&](uint32_t, uint32_t i, uint32_t j, int32_t v) {
        if (!color) data[view_sample_offset(rs, ps, 0, i, j, 0)] = (uint8_t)v;
    });
    if (rc || !color) return rc;
    if ((rc = store_rgb8(ch, planes, nullptr)) != 0) return rc;  // (checked first: a region that fails here leaves the view as it was)
    return convert_rgb8(ch, planes, [&](size_t i, unsigned c, uint8_t v) {
        const uint32_t j = (uint32_t)(i / r.w), k = (uint32_t)(i - (size_t)j * r.w);
        data[view_sample_offset(rs, ps, cs, k, j, c)] = v;
    });
}

}  // extern "C"
