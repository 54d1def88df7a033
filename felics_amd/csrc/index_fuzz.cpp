// index_fuzz -- sanitizer driver for the restart index's host functions (CPU only: felics_index.cpp + felics_decode.cpp, nothing
// of HIP).  Every file NAME of a directory that does not end in ".idx" is taken as a stream:
//   * felics_index_build at two segment sizes; where it succeeds, felics_decompress_indexed must give felics_decompress's pixels,
//     and the index then goes through a few hundred byte mutations of its own (header fields, bit offsets, counters, window
//     samples), each of which must be accepted or refused with a code;
//   * if NAME.idx exists it is used as the index of NAME as it is (an index of the unmutated stream beside a mutated stream, a
//     mutated index beside a good stream): any code, no crash;
//   * felics_decompress_region_indexed with random regions on all of these pairs: on a good pair every crop must equal the same
//     window of felics_decompress's pixels and felics_region_segments must name what a pixel-by-pixel marking names; on a mutated
//     or foreign pair any code, no crash;
//   * felics_decompress_indexed_view, the host model of the indexed views call, on all of these pairs too, each time into a random
//     admissible view (a pitch, pixel stride 1 or 2, a flipped row or channel axis, interleaved or planar) whose target buffer is
//     EXACTLY the size of the view's hull, so a store outside it is the sanitizer's to report: on a good pair every sample must be
//     felics_decompress's and every other byte of the hull untouched; on a mutated or foreign pair any code, no crash.
//   * felics_decompress_region_indexed_view (and, in the 16-bit mode, felics_decompress_region_indexed16_view), the host models of
//     the region views calls, on all of these pairs as well: random regions into random admissible views of the window's size whose
//     hull lies between guard bytes (region_view_leg below).  On a good pair the samples must equal the dense region call's, every
//     other byte of the hull and both guards must be untouched; on a mutated or foreign pair any code, guards intact, no crash.
// In both modes every stream with a valid header also has the device region calls' plan made for its shape (felics_index.h:
// region_plan) and checked against felics_region_segments: plan_leg below.
// `index_fuzz --index16 DIR` runs the 16-bit index's host functions instead (felics_index16.cpp): felics_index16_build at the same
// two segment sizes; where it succeeds the size is within felics_index16_size_max, the two-call pattern holds,
// felics_decompress_indexed16 gives felics_decompress's pixels, felics_decompress_region_indexed16 gives the full frame, a seeded
// interior window and an empty one, felics_decompress_indexed16_view gives felics_decompress's samples in two random admissible views
// (as in the 8-bit mode: a target of exactly the hull, every other byte untouched), and the index goes through byte mutations (header,
// directory, rows' context words, anywhere) and cuts, each with the same three windows and every other one with a view; NAME.idx beside
// NAME is used as it is: any code, no crash.
// Built with -fsanitize=address,undefined by `make asan`; tests/test_index_cpu.py and tests/test_index16_cpu.py feed it mutated corpora.
// Exit code 0 = every input was handled without a sanitizer report and every accepted pair decoded to the right pixels.
#include <dirent.h>

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/felics.h"
#include "felics_index.h"

static bool slurp(const std::string &p, std::vector<uint8_t> &b) {
    FILE *f = fopen(p.c_str(), "rb");
    if (!f) return false;
    uint8_t chunk[1 << 16];
    size_t got;
    b.clear();
    while ((got = fread(chunk, 1, sizeof chunk, f)) > 0) b.insert(b.end(), chunk, chunk + got);
    fclose(f);
    return true;
}

static bool ends_with(const std::string &s, const char *suffix) {
    const size_t n = strlen(suffix);
    return s.size() >= n && s.compare(s.size() - n, n, suffix) == 0;
}

// The region calls' plan (felics_index.h: region_plan, what both device calls upload) for an image of h's shape at segment size seg
// and `sample_bytes` per output sample, on seeded random regions among which are empty ones, one-pixel ones, the whole image and ones
// that end on the last pixel: every non-empty region must name exactly felics_region_segments' segments, once per plane, in (plane,
// segment) order, contiguously; an empty one the single header-only item; the crops back to back in bytes of the sample; `walked` the
// items that are not header-only.  Returns the regions planned, 0 where the plan is wrong.
template <typename Next>
static size_t plan_leg(const felics_header &h, uint32_t seg, uint32_t sample_bytes, Next next) {
    using namespace felics;
    const uint32_t W = h.width, H = h.height, planes = h.color_type ? 3 : 1;
    if ((uint64_t)W * H > 0xFFFFFFFFull) return 1;  // (no call plans such a shape)
    std::vector<felics_region> regs;
    regs.push_back(felics_region{0, 0, 0, W, H});            // the whole image (empty if the image is)
    regs.push_back(felics_region{0, W / 2, H / 2, 0, 0});    // empty
    regs.push_back(felics_region{0, 0, 0, W, 0});            // empty, one side only
    if (W && H) {
        regs.push_back(felics_region{0, W - 1, H - 1, 1, 1});  // the last pixel
        regs.push_back(felics_region{0, 0, 0, 1, 1});
        for (int k = 0; k < 8; k++) {
            felics_region r = {0, (uint32_t)(next() % W), (uint32_t)(next() % H), 0, 0};
            const bool to_end = k % 4 == 3;  // ends on the last pixel
            r.w = to_end ? W - r.x : (uint32_t)(1 + next() % std::min<uint64_t>(W - r.x, 300));
            r.h = to_end ? H - r.y : (uint32_t)(1 + next() % std::min<uint64_t>(H - r.y, 40));
            if (k == 5) r.w = r.h = 1;
            regs.push_back(r);
        }
    }
    std::vector<uint64_t> out(regs.size(), ~0ull);
    RegionPlan P;
    if (region_plan(W, H, seg, planes, sample_bytes, regs.data(), regs.size(), out.data(), P) != FELICS_OK || P.rows.size() != regs.size()) return 0;
    const size_t K = (size_t)(((uint64_t)W * H + seg - 1) / seg);
    std::vector<uint32_t> want(K + 1);
    uint64_t at = 0, plane_at = 0, header_only = 0, item = 0, max_crop = 0;
    for (size_t r = 0; r < regs.size(); r++) {
        const felics_region &g = regs[r];
        const RegionRow &row = P.rows[r];
        size_t cnt = 0;
        if (felics_region_segments(W, H, seg, &g, want.data(), K, &cnt) != FELICS_OK) return 0;
        const bool empty = g.w == 0 || g.h == 0;
        if (empty != (cnt == 0) || row.item0 != item || row.nitems != (empty ? 1 : planes * cnt) || out[r] != at || row.out_off != at ||
            row.plane_off != plane_at || row.stream != g.stream || row.x != g.x || row.y != g.y || row.w != g.w || row.h != g.h)
            return 0;
        if (item + row.nitems > P.items.size()) return 0;
        if (empty) {
            const RegionItem &it = P.items[item];
            if (it.region != r || it.plane != 0 || it.seg != REGION_HEADER_ONLY) return 0;
            header_only++;
        }
        for (uint32_t c = 0; !empty && c < planes; c++)
            for (size_t j = 0; j < cnt; j++) {
                const RegionItem &it = P.items[item + c * cnt + j];
                if (it.region != r || it.plane != c || it.seg != want[j]) return 0;
            }
        item += row.nitems;
        at += (uint64_t)g.w * g.h * planes * sample_bytes;
        if (planes == 3) plane_at += (uint64_t)g.w * g.h * 3, max_crop = std::max(max_crop, (uint64_t)g.w * g.h);
    }
    if (item != P.items.size() || P.walked != item - header_only || P.skipped != regs.size() * planes * K - P.walked || P.plane_samples != plane_at ||
        P.max_crop != max_crop || P.pixels_walked > P.walked * seg)
        return 0;
    return regs.size();
}

// The host models of the region views calls (S = 1: felics_decompress_region_indexed_view, S = 2: felics_decompress_region_indexed16_view)
// on one pair: window r of the image of header h into a random admissible view of r's size (a pitch, every sample or every other, a
// flipped row or channel axis, interleaved or planar) whose hull lies between GUARD bytes of 0xA5 on either side.  Whatever the pair:
// both guards intact.  `good`: the model and the dense region call (its code rc_dense, its crop `crop`) must both have succeeded, every
// sample must be the dense crop's and every other byte of the hull untouched.  False where any of that does not hold.
template <int S, typename Next>
static bool region_view_leg(const std::vector<uint8_t> &stream, const uint8_t *index, size_t index_len, const felics_header &h, const felics_region &r,
                            const uint8_t *crop, int rc_dense, bool good, Next next) {
    constexpr size_t GUARD = 64;
    static std::vector<uint8_t> target, expect;
    const int64_t W = r.w, H = r.h, C = h.color_type ? 3 : 1;
    if ((uint64_t)W * H * C * S * 4 > (32u << 20)) return true;  // (targets are this driver's to allocate)
    felics_view v = {nullptr, r.w, r.h, h.color_type, S == 2 ? FELICS_DEPTH_16 : FELICS_DEPTH_8, 0, 0, 0};
    const int64_t ps = S * (1 + (int64_t)(next() % 2)), pad = S * (int64_t)(next() % 8);
    const bool planar = C == 3 && next() % 2, flip_rows = next() % 2, flip_ch = C == 3 && next() % 2;
    if (C == 1 || planar) {
        v.pixel_stride = ps;
        v.row_stride = W * ps + pad;
        v.channel_stride = C == 3 ? H * v.row_stride + pad : 0;
    } else {
        v.channel_stride = S;
        v.pixel_stride = (3 + (int64_t)(next() % 2)) * ps;  // RGB or RGBA pixels, every one or every other
        v.row_stride = W * v.pixel_stride + pad;
    }
    if (flip_rows) v.row_stride = -v.row_stride;
    if (flip_ch) v.channel_stride = -v.channel_stride;
    int64_t lo = 0, hi = W && H ? S : 0;
    const int64_t spans[3] = {(H - 1) * v.row_stride, (W - 1) * v.pixel_stride, (C - 1) * v.channel_stride};
    for (int d = 0; d < 3 && W && H; d++) (spans[d] < 0 ? lo : hi) += spans[d];
    target.assign(GUARD + (size_t)(hi - lo) + GUARD, 0xA5);
    uint8_t *hull = target.data() + GUARD;
    if (W && H) v.data = hull - lo;
    felics_header hv;
    const int rc = S == 2 ? felics_decompress_region_indexed16_view(stream.data(), stream.size(), index, index_len, &r, &v, &hv)
                          : felics_decompress_region_indexed_view(stream.data(), stream.size(), index, index_len, &r, &v, &hv);
    for (size_t i = 0; i < GUARD; i++)
        if (target[i] != 0xA5 || target[target.size() - 1 - i] != 0xA5) return false;
    if (!good) return true;
    if (rc != FELICS_OK || rc_dense != FELICS_OK) return false;
    expect.assign(target.size(), 0xA5);
    for (int64_t y = 0; y < H; y++)
        for (int64_t x = 0; x < W; x++)
            for (int64_t c = 0; c < C; c++)
                memcpy(&expect[GUARD + (size_t)(y * v.row_stride + x * v.pixel_stride + c * v.channel_stride - lo)], &crop[(size_t)((y * W + x) * C + c) * S], S);
    return target == expect;
}

// the --index16 mode
static int fuzz16(const char *dir) {
    {  // argument checks
        size_t n = 7;
        uint8_t b[64] = {0};
        int bad = 0;
        bad += felics_index16_build(nullptr, 5, 4096, b, sizeof b, &n) != FELICS_E_INVALID_ARGUMENT;
        bad += felics_index16_build(b, sizeof b, 4096, b, sizeof b, nullptr) != FELICS_E_INVALID_ARGUMENT;
        bad += felics_decompress_indexed16(nullptr, 5, b, sizeof b, b, sizeof b, nullptr) != FELICS_E_INVALID_ARGUMENT;
        bad += felics_decompress_indexed16(b, sizeof b, nullptr, 5, b, sizeof b, nullptr) != FELICS_E_INVALID_ARGUMENT;
        const felics_region one{0, 0, 0, 1, 1};
        const felics_view px1{b, 1, 1, FELICS_COLOR_GRAY, FELICS_DEPTH_16, 2, 2, 0};
        bad += felics_decompress_region_indexed16_view(b, sizeof b, b, sizeof b, nullptr, &px1, nullptr) != FELICS_E_INVALID_ARGUMENT;
        bad += felics_decompress_region_indexed16_view(b, sizeof b, b, sizeof b, &one, nullptr, nullptr) != FELICS_E_INVALID_ARGUMENT;
        bad += felics_decompress_region_indexed16_view(nullptr, 5, b, sizeof b, &one, &px1, nullptr) != FELICS_E_INVALID_ARGUMENT;
        bad += felics_index16_size_max(1, 1, 0, 4095) != 0 || felics_index16_size_max(1, 1, 2, 4096) != 0 || felics_index16_size_max(1, 1, 0, 4096) != 192;  // (header, one entry, one window)
        bad += felics_index16_size_max(0xFFFFFFFFu, 0xFFFFFFFFu, 1, 4096) != 0 || felics_index16_size_max(0, 5, 1, 4096) != 64;
        if (bad) {
            fprintf(stderr, "argument checks (16-bit): %d unexpected results\n", bad);
            return 1;
        }
    }
    DIR *d = opendir(dir);
    if (!d) return 2;
    std::vector<std::string> names;
    while (dirent *e = readdir(d))
        if (e->d_name[0] != '.' && !ends_with(e->d_name, ".idx")) names.push_back(e->d_name);
    closedir(d);
    size_t built = 0, refused = 0, mutations = 0, mut_accepted = 0, pairs = 0, pairs_ok = 0, plan_streams = 0, plan_regions = 0;
    const size_t cap = 32u << 20;
    std::vector<uint8_t> buf, given, px(cap), ref(cap), index(cap);
    uint64_t rng = 0x9E3779B97F4A7C15ull;
    auto next = [&]() {
        rng ^= rng << 13;
        rng ^= rng >> 7;
        rng ^= rng << 17;
        return rng;
    };
    // felics_decompress_region_indexed16 on a pair, for three windows of the header's shape -- the full frame, a seeded interior
    // window, an empty one --, each into a crop of exactly its size (a store behind it is the sanitizer's to report).  `good`: every
    // call must succeed, the full-frame crop must be px's frame (the caller has felics_decompress_indexed16's output there) and the interior one
    // ref's window (ref holds h's image).
    std::vector<uint8_t> crop;
    auto regions16_on = [&](const uint8_t *index_bytes, size_t index_len, const felics_header &h, bool good) {
        const size_t planes = h.color_type ? 3 : 1;
        felics_region inner = {0, 0, 0, 0, 0};
        if (h.width && h.height) {
            inner.x = (uint32_t)(next() % h.width);
            inner.y = (uint32_t)(next() % h.height);
            inner.w = (uint32_t)(1 + next() % std::min<uint64_t>(h.width - inner.x, 96));
            inner.h = (uint32_t)(1 + next() % std::min<uint64_t>(h.height - inner.y, 48));
        }
        const felics_region wins[3] = {{0, 0, 0, h.width, h.height}, inner, {0, h.width / 2, h.height / 2, 0, h.height ? 1u : 0u}};
        for (int k = 0; k < 3; k++) {
            const felics_region &r = wins[k];
            const size_t bytes = (size_t)r.w * r.h * planes * 2;
            if (bytes > cap) continue;  // (crops are this driver's to allocate)
            crop.assign(bytes, 0xA5);
            felics_header hr;
            const int rc = felics_decompress_region_indexed16(buf.data(), buf.size(), index_bytes, index_len, &r, crop.data(), bytes, &hr);
            // the same window into a view (a mutated pair: the seeded window only -- every call clears a 7.9 MB table)
            if ((good || k == 1) && !region_view_leg<2>(buf, index_bytes, index_len, h, r, crop.data(), rc, good, next)) return false;
            if (!good) continue;
            if (rc != FELICS_OK) return false;
            if (k == 0 && memcmp(crop.data(), px.data(), bytes) != 0) return false;  // (px: felics_decompress_indexed16's frame)
            for (uint32_t yy = 0; k == 1 && yy < r.h; yy++)
                if (memcmp(&crop[(size_t)yy * r.w * planes * 2], &ref[((size_t)(r.y + yy) * h.width + r.x) * planes * 2], (size_t)r.w * planes * 2) != 0)
                    return false;
        }
        return true;
    };
    // felics_decompress_indexed16_view, the host model of the indexed views call for 16-bit streams, on a pair: into a random
    // admissible view of the header's shape (a pitch, pixel stride 2 or 4 bytes, a flipped row or channel axis, interleaved or planar)
    // whose target buffer is EXACTLY the size of the view's hull, so a store outside it is the sanitizer's to report.  `good`: the call
    // must succeed, every sample must be ref's (h's image) and every other byte of the hull untouched.
    std::vector<uint8_t> target, expect;
    auto view16_on = [&](const uint8_t *index_bytes, size_t index_len, const felics_header &h, bool good) {
        const int64_t W = h.width, H = h.height, C = h.color_type ? 3 : 1;
        if ((uint64_t)W * H * C * 2 * 3 > cap) return true;  // (targets are this driver's to allocate)
        felics_view v{nullptr, h.width, h.height, h.color_type, FELICS_DEPTH_16, 0, 0, 0};
        const int64_t gap = 2 * (int64_t)(next() % 2);
        if (C == 3 && next() % 2) {  // planar
            v.pixel_stride = 2 + gap;
            v.row_stride = W * v.pixel_stride + 2 * (int64_t)(next() % 5);
            v.channel_stride = H * v.row_stride + 2 * (int64_t)(next() % 7);
        } else {
            v.channel_stride = 2;
            v.pixel_stride = 2 * C + gap * C;
            v.row_stride = W * v.pixel_stride + 2 * (int64_t)(next() % 5);
        }
        if (next() % 2) v.row_stride = -v.row_stride;
        if (C == 3 && next() % 2) v.channel_stride = -v.channel_stride;
        int64_t lo = 0, hi = W && H ? 2 : 0;
        const int64_t spans[3] = {(H - 1) * v.row_stride, (W - 1) * v.pixel_stride, (C - 1) * v.channel_stride};
        for (int k = 0; k < 3 && W && H; k++) (spans[k] < 0 ? lo : hi) += spans[k];
        target.assign((size_t)(hi - lo), 0xA5);
        if (W && H) v.data = target.data() - lo;
        felics_header hv;
        const int rc = felics_decompress_indexed16_view(buf.data(), buf.size(), index_bytes, index_len, &v, &hv);
        if (!good) return true;
        if (rc != FELICS_OK) return false;
        expect.assign(target.size(), 0xA5);
        for (int64_t y = 0; y < H; y++)
            for (int64_t x = 0; x < W; x++)
                for (int64_t c = 0; c < C; c++)
                    memcpy(&expect[(size_t)(y * v.row_stride + x * v.pixel_stride + c * v.channel_stride - lo)], &ref[(size_t)((y * W + x) * C + c) * 2], 2);
        return target == expect;
    };
    for (const std::string &n : names) {
        const std::string path = std::string(dir) + "/" + n;
        if (!slurp(path, buf)) continue;
        felics_header h, h2;
        if (felics_read_header(buf.data(), buf.size(), &h) == FELICS_OK) {  // the region plan, whatever else the stream is good for
            for (uint32_t seg : {4096u, 12288u}) {
                const size_t got = plan_leg(h, seg, h.pixel_depth ? 2 : 1, next);
                if (!got) {
                    fprintf(stderr, "%s: the region plan at segment %u differs from felics_region_segments or from its own layout rules\n", n.c_str(), seg);
                    return 1;
                }
                plan_regions += got;
            }
            plan_streams++;
        }
        const int rc_plain = felics_decompress(buf.data(), buf.size(), ref.data(), ref.size(), &h);
        if (rc_plain == FELICS_E_BUFFER_TOO_SMALL) continue;  // (larger than this driver's buffers)
        const size_t frame = rc_plain == FELICS_OK ? (size_t)h.width * h.height * (h.color_type ? 3 : 1) * (h.pixel_depth ? 2 : 1) : 0;
        if (slurp(path + ".idx", given)) {
            pairs++;
            if (rc_plain == FELICS_OK && h.pixel_depth) view16_on(given.data(), given.size(), h, false);
            if (felics_decompress_indexed16(buf.data(), buf.size(), given.data(), given.size(), px.data(), px.size(), &h2) == FELICS_OK) pairs_ok++;
        }
        for (uint32_t seg : {4096u, 12288u}) {
            size_t ilen = 0;
            const int rb = felics_index16_build(buf.data(), buf.size(), seg, index.data(), index.size(), &ilen);
            if (rb != FELICS_OK) {
                refused++;
                continue;
            }
            built++;
            if (rc_plain != FELICS_OK || !h.pixel_depth) {
                fprintf(stderr, "%s: an index was built of a stream felics_decompress refuses (%d) or of an 8-bit stream\n", n.c_str(), rc_plain);
                return 1;
            }
            if (ilen > felics_index16_size_max(h.width, h.height, h.color_type, seg) || ilen % 64) {
                fprintf(stderr, "%s: index of %zu bytes, felics_index16_size_max says less\n", n.c_str(), ilen);
                return 1;
            }
            size_t need = 0;  // a short buffer: refused with the size, nothing written behind it
            if (felics_index16_build(buf.data(), buf.size(), seg, index.data() + ilen, ilen - 1, &need) != FELICS_E_BUFFER_TOO_SMALL || need != ilen) {
                fprintf(stderr, "%s: short buffer not refused with the size\n", n.c_str());
                return 1;
            }
            const int rc = felics_decompress_indexed16(buf.data(), buf.size(), index.data(), ilen, px.data(), px.size(), &h2);
            if (rc != FELICS_OK || memcmp(px.data(), ref.data(), frame) != 0) {
                fprintf(stderr, "%s: indexed decode %d, or other pixels than felics_decompress\n", n.c_str(), rc);
                return 1;
            }
            if (!regions16_on(index.data(), ilen, h, true)) {
                fprintf(stderr, "%s: a region of a good pair failed or differs from felics_decompress_indexed16's window, or its view differs from the crop\n", n.c_str());
                return 1;
            }
            if (!view16_on(index.data(), ilen, h, true) || !view16_on(index.data(), ilen, h, true)) {
                fprintf(stderr, "%s: a view of a good pair failed, differs from felics_decompress's samples or lost a byte between them\n", n.c_str());
                return 1;
            }
            const std::vector<uint8_t> idx(index.begin(), index.begin() + ilen);
            const size_t entries = (size_t)(h.color_type ? 3 : 1) * (((size_t)h.width * h.height + seg - 1) / seg);
            const int rounds = ilen > (1u << 20) ? 4 : 10;  // (a call clears a table of 7.9 MB: fewer rounds than the 8-bit mode's)
            for (int m = 0; m < rounds; m++) {
                std::vector<uint8_t> bad = idx;
                const int flips = 1 + (int)(next() % 3);
                for (int f = 0; f < flips; f++) {
                    // header fields, a directory entry, the context word of a row from the end, or anywhere
                    const uint64_t r = next() & 3;
                    size_t pos = (size_t)(next() % ilen);
                    if (r == 0) pos = (size_t)(next() % 64);
                    else if (r == 1 && entries) pos = 64 + (size_t)(next() % (32 * entries));
                    else if (r == 2 && ilen >= 128) pos = ilen - 64 * (1 + (size_t)(next() % std::min<size_t>(8, ilen / 64 - 1))) + 60 + (size_t)(next() % 4);
                    bad[pos % ilen] ^= (uint8_t)(1u << (next() % 8));
                }
                mutations++;
                if (felics_decompress_indexed16(buf.data(), buf.size(), bad.data(), bad.size(), px.data(), px.size(), &h2) == FELICS_OK) mut_accepted++;
                if (!regions16_on(bad.data(), bad.size(), h, false)) {
                    fprintf(stderr, "%s: a region view of a mutated index wrote into its guard bytes\n", n.c_str());
                    return 1;
                }
                if (m % 2 == 0) view16_on(bad.data(), bad.size(), h, false);  // (every call clears a 7.9 MB table: every other mutation)
                if (m % 5 == 0) {  // and cut short
                    const size_t cut = (size_t)(next() % ilen);
                    if (felics_decompress_indexed16(buf.data(), buf.size(), bad.data(), cut, px.data(), px.size(), &h2) == FELICS_OK) {
                        fprintf(stderr, "%s: an index cut to %zu of %zu bytes was accepted\n", n.c_str(), cut, ilen);
                        return 1;
                    }
                }
            }
        }
    }
    printf("index_fuzz --index16: %zu files, %zu indexes built, %zu refused, %zu pairs (%zu accepted), %zu mutations (%zu accepted)\n", names.size(), built,
           refused, pairs, pairs_ok, mutations, mut_accepted);
    printf("index_fuzz --index16: region plans of %zu streams with a valid header, %zu regions planned as felics_region_segments names them\n", plan_streams,
           plan_regions);
    return 0;
}

int main(int argc, char **argv) {
    if (argc >= 3 && strcmp(argv[1], "--index16") == 0) return fuzz16(argv[2]);
    if (argc < 2) {
        fprintf(stderr, "usage: index_fuzz DIR\n");
        return 2;
    }
    {  // argument checks
        size_t n = 7;
        uint8_t b[64] = {0};
        int bad = 0;
        bad += felics_index_build(nullptr, 5, 4096, b, sizeof b, &n) != FELICS_E_INVALID_ARGUMENT;
        bad += felics_index_build(b, sizeof b, 4096, b, sizeof b, nullptr) != FELICS_E_INVALID_ARGUMENT;
        bad += felics_decompress_indexed(nullptr, 5, b, sizeof b, b, sizeof b, nullptr) != FELICS_E_INVALID_ARGUMENT;
        bad += felics_decompress_indexed(b, sizeof b, nullptr, 5, b, sizeof b, nullptr) != FELICS_E_INVALID_ARGUMENT;
        bad += felics_index_size(1, 1, 0, 1, 4096) != 0 || felics_index_size(1, 1, 0, 0, 4095) != 0 || felics_index_size(1, 1, 2, 0, 4096) != 0;
        bad += felics_index_size(0xFFFFFFFFu, 0xFFFFFFFFu, 1, 0, 4096) != 0;
        const felics_region in{0, 1, 1, 2, 2}, out{0, 0xFFFFFFFFu, 0, 2, 1};
        uint32_t segs[4];
        bad += felics_region_segments(8, 8, 4096, nullptr, segs, 4, &n) != FELICS_E_INVALID_ARGUMENT;
        bad += felics_region_segments(8, 8, 4096, &in, segs, 4, nullptr) != FELICS_E_INVALID_ARGUMENT;
        bad += felics_region_segments(8, 8, 4095, &in, segs, 4, &n) != FELICS_E_INVALID_ARGUMENT;
        bad += felics_region_segments(8, 8, 4096, &out, segs, 4, &n) != FELICS_E_INVALID_ARGUMENT;  // x + w wraps in 32 bits
        bad += felics_region_segments(8, 8, 4096, &in, nullptr, 0, &n) != FELICS_E_BUFFER_TOO_SMALL || n != 1;
        bad += felics_region_segments(8, 8, 4096, &in, segs, 4, &n) != FELICS_OK || n != 1 || segs[0] != 0;
        bad += felics_decompress_region_indexed(b, sizeof b, b, sizeof b, nullptr, b, sizeof b, nullptr) != FELICS_E_INVALID_ARGUMENT;
        const felics_view ok{b, 8, 8, FELICS_COLOR_GRAY, FELICS_DEPTH_8, 8, 1, 0}, alias{b, 8, 8, FELICS_COLOR_GRAY, FELICS_DEPTH_8, 4, 1, 0};
        bad += felics_decompress_indexed_view(b, sizeof b, b, sizeof b, nullptr, nullptr) != FELICS_E_INVALID_ARGUMENT;
        bad += felics_decompress_indexed_view(nullptr, 5, b, sizeof b, &ok, nullptr) != FELICS_E_INVALID_ARGUMENT;
        bad += felics_decompress_indexed_view(b, sizeof b, b, sizeof b, &alias, nullptr) != FELICS_E_INVALID_ARGUMENT;  // rows that share bytes
        const felics_view win{b, 2, 2, FELICS_COLOR_GRAY, FELICS_DEPTH_8, 8, 1, 0};
        bad += felics_decompress_region_indexed_view(b, sizeof b, b, sizeof b, nullptr, &win, nullptr) != FELICS_E_INVALID_ARGUMENT;
        bad += felics_decompress_region_indexed_view(b, sizeof b, b, sizeof b, &in, nullptr, nullptr) != FELICS_E_INVALID_ARGUMENT;
        bad += felics_decompress_region_indexed_view(nullptr, 5, b, sizeof b, &in, &win, nullptr) != FELICS_E_INVALID_ARGUMENT;
        bad += felics_decompress_region_indexed_view(b, sizeof b, b, sizeof b, &in, &ok, nullptr) != FELICS_E_INVALID_ARGUMENT;  // an 8 x 8 view of a 2 x 2 window
        if (bad) {
            fprintf(stderr, "argument checks: %d unexpected results\n", bad);
            return 1;
        }
    }
    DIR *d = opendir(argv[1]);
    if (!d) return 2;
    std::vector<std::string> names;
    while (dirent *e = readdir(d))
        if (e->d_name[0] != '.' && !ends_with(e->d_name, ".idx")) names.push_back(e->d_name);
    closedir(d);
    size_t regions = 0, views = 0, built = 0, refused = 0, mutations = 0, mut_accepted = 0, pairs = 0, pairs_ok = 0, plan_streams = 0, plan_regions = 0;
    const size_t cap = 32u << 20;  // decoders and the builder get bounded buffers whatever a header claims
    std::vector<uint8_t> buf, idx, given, px(cap), ref(cap), index(cap);
    uint64_t rng = 0x9E3779B97F4A7C15ull;
    auto next = [&]() {
        rng ^= rng << 13;
        rng ^= rng >> 7;
        rng ^= rng << 17;
        return rng;
    };
    // a random region of a w x h image: mostly small windows, now and then whole rows, whole columns or nothing
    auto region_of = [&](uint32_t w, uint32_t h) {
        felics_region r = {0, 0, 0, 0, 0};
        if (!w || !h) return r;
        r.x = (uint32_t)(next() % w);
        r.y = (uint32_t)(next() % h);
        const uint64_t kind = next() % 8;
        r.w = kind == 0 ? w - r.x : (uint32_t)(next() % std::min<uint64_t>(w - r.x, 64) + (kind != 1));
        r.h = kind == 2 ? h - r.y : (uint32_t)(next() % std::min<uint64_t>(h - r.y, 64) + (kind != 3));
        r.w = std::min(r.w, w - r.x);
        r.h = std::min(r.h, h - r.y);
        return r;
    };
    std::vector<uint8_t> crop, mark;
    std::vector<uint32_t> segs;
    // the region decoder on a pair; `good`: the crop must then be ref's window (ref holds h's image)
    auto regions_on = [&](const std::vector<uint8_t> &index_bytes, size_t index_len, const felics_header &h, bool good, int count) {
        const size_t planes = h.color_type ? 3 : 1;
        for (int k = 0; k < count; k++) {
            const felics_region r = region_of(h.width, h.height);
            crop.assign((size_t)r.w * r.h * planes + 1, 0xA5);
            felics_header hr;
            const int rc = felics_decompress_region_indexed(buf.data(), buf.size(), index_bytes.data(), index_len, &r, crop.data(), crop.size() - 1, &hr);
            regions++;
            if (crop.back() != 0xA5) return false;
            if (!region_view_leg<1>(buf, index_bytes.data(), index_len, h, r, crop.data(), rc, good, next)) return false;  // the same window into a view
            if (!good) continue;
            if (rc != FELICS_OK) return false;
            for (uint32_t yy = 0; yy < r.h; yy++)
                if (memcmp(&crop[(size_t)yy * r.w * planes], &ref[((size_t)(r.y + yy) * h.width + r.x) * planes], (size_t)r.w * planes) != 0) return false;
        }
        return true;
    };
    // the host model of the views call on a pair, into a random admissible view of the header's shape over a buffer that is exactly
    // the view's hull; `good`: it must succeed, the samples must be ref's and the bytes between them must keep their pattern
    std::vector<uint8_t> target, expect;
    auto view_on = [&](const std::vector<uint8_t> &index_bytes, size_t index_len, const felics_header &h, bool good) {
        const int64_t W = h.width, H = h.height, C = h.color_type ? 3 : 1;
        if ((uint64_t)W * H > (1u << 22)) return true;  // (targets are this driver's to allocate: larger ones are left out)
        felics_view v = {nullptr, h.width, h.height, h.color_type, FELICS_DEPTH_8, 0, 0, 0};
        const int64_t ps = 1 + (int64_t)(next() % 2), pad = (int64_t)(next() % 16);
        const bool planar = C == 3 && next() % 2, flip_rows = next() % 2, flip_ch = C == 3 && next() % 2;
        if (C == 1 || planar) {
            v.pixel_stride = ps;
            v.row_stride = W * ps + pad;
            v.channel_stride = C == 3 ? H * v.row_stride + pad : 0;
        } else {
            v.channel_stride = 1;
            v.pixel_stride = (3 + (int64_t)(next() % 2)) * ps;  // RGB or RGBA pixels, every one or every other
            v.row_stride = W * v.pixel_stride + pad;
        }
        if (flip_rows) v.row_stride = -v.row_stride;
        if (flip_ch) v.channel_stride = -v.channel_stride;
        int64_t lo = 0, hi = W && H ? 1 : 0;
        const int64_t spans[3] = {(H - 1) * v.row_stride, (W - 1) * v.pixel_stride, (C - 1) * v.channel_stride};
        for (int d = 0; d < 3 && W && H; d++) (spans[d] < 0 ? lo : hi) += spans[d];
        target.assign((size_t)(hi - lo), 0xA5);
        if (W && H) v.data = target.data() - lo;
        felics_header hv;
        const int rc = felics_decompress_indexed_view(buf.data(), buf.size(), index_bytes.data(), index_len, &v, &hv);
        views++;
        if (!good) return true;
        if (rc != FELICS_OK) return false;
        expect.assign(target.size(), 0xA5);
        for (int64_t y = 0; y < H; y++)
            for (int64_t x = 0; x < W; x++)
                for (int64_t c = 0; c < C; c++) expect[(size_t)(y * v.row_stride + x * v.pixel_stride + c * v.channel_stride - lo)] = ref[(size_t)((y * W + x) * C + c)];
        return target == expect;
    };
    for (const std::string &n : names) {
        const std::string path = std::string(argv[1]) + "/" + n;
        if (!slurp(path, buf)) continue;
        felics_header h, h2;
        if (felics_read_header(buf.data(), buf.size(), &h) == FELICS_OK) {  // the region plan, whatever else the stream is good for
            for (uint32_t seg : {4096u, 12288u}) {
                const size_t got = plan_leg(h, seg, h.pixel_depth ? 2 : 1, next);
                if (!got) {
                    fprintf(stderr, "%s: the region plan at segment %u differs from felics_region_segments or from its own layout rules\n", n.c_str(), seg);
                    return 1;
                }
                plan_regions += got;
            }
            plan_streams++;
        }
        const int rc_plain = felics_decompress(buf.data(), buf.size(), ref.data(), ref.size(), &h);
        if (rc_plain == FELICS_E_BUFFER_TOO_SMALL) continue;  // (larger than this driver's buffers)
        const size_t frame = rc_plain == FELICS_OK ? (size_t)h.width * h.height * (h.color_type ? 3 : 1) * (h.pixel_depth ? 2 : 1) : 0;
        if (slurp(path + ".idx", given)) {
            pairs++;
            // (any code: a flipped bit that keeps a segment's length decodes through the index -- the damage ends at the next
            // checkpoint -- where the plain decoder carries it on and fails; the checks do not prove the pairing, felics.h)
            if (felics_decompress_indexed(buf.data(), buf.size(), given.data(), given.size(), px.data(), px.size(), &h2) == FELICS_OK) pairs_ok++;
            felics_header hh;  // (a stream felics_decompress refuses is walked too, as far as its header names a shape)
            if (felics_read_header(buf.data(), buf.size(), &hh) == FELICS_OK && (uint64_t)hh.width * hh.height <= (1u << 22) &&  // (crops are this driver's to allocate)
                !regions_on(given, given.size(), hh, false, 8)) {
                fprintf(stderr, "%s: a region of a given pair wrote past its crop\n", n.c_str());
                return 1;
            }
            if (felics_read_header(buf.data(), buf.size(), &hh) == FELICS_OK) view_on(given, given.size(), hh, false);
        }
        for (uint32_t seg : {4096u, 12288u}) {
            size_t ilen = 0;
            const int rb = felics_index_build(buf.data(), buf.size(), seg, index.data(), index.size(), &ilen);
            if (rb != FELICS_OK) {
                refused++;
                continue;
            }
            built++;
            if (rc_plain != FELICS_OK) {
                fprintf(stderr, "%s: an index was built of a stream felics_decompress refuses (%d)\n", n.c_str(), rc_plain);
                return 1;
            }
            if (ilen != felics_index_size(h.width, h.height, h.color_type, h.pixel_depth, seg)) {
                fprintf(stderr, "%s: index of %zu bytes, felics_index_size says otherwise\n", n.c_str(), ilen);
                return 1;
            }
            size_t need = 0;  // a short buffer: refused with the size, nothing written behind it
            if (ilen && (felics_index_build(buf.data(), buf.size(), seg, index.data() + ilen, ilen - 1, &need) != FELICS_E_BUFFER_TOO_SMALL || need != ilen)) {
                fprintf(stderr, "%s: short buffer not refused with the size\n", n.c_str());
                return 1;
            }
            const int rc = felics_decompress_indexed(buf.data(), buf.size(), index.data(), ilen, px.data(), px.size(), &h2);
            if (rc != FELICS_OK || memcmp(px.data(), ref.data(), frame) != 0) {
                fprintf(stderr, "%s: indexed decode %d, or other pixels than felics_decompress\n", n.c_str(), rc);
                return 1;
            }
            if (!regions_on(index, ilen, h, true, 24)) {
                fprintf(stderr, "%s: a region of a good pair failed, differs from felics_decompress's window or wrote past its crop\n", n.c_str());
                return 1;
            }
            for (int k = 0; k < 4; k++)
                if (!view_on(index, ilen, h, true)) {
                    fprintf(stderr, "%s: the view model failed on a good pair, wrote other samples than felics_decompress's or a byte that is no sample\n",
                            n.c_str());
                    return 1;
                }
            for (int k = 0; k < 8; k++) {  // the planner against a marking of the region's pixels
                const felics_region r = region_of(h.width, h.height);
                const size_t K = ((size_t)h.width * h.height + seg - 1) / seg;
                size_t cnt = 0;
                segs.assign(K + 1, 0);
                mark.assign(K + 1, 0);
                for (uint32_t yy = 0; yy < r.h; yy++)
                    for (uint32_t xx = 0; xx < r.w; xx++) mark[((size_t)(r.y + yy) * h.width + r.x + xx) / seg] = 1;
                bool same = felics_region_segments(h.width, h.height, seg, &r, segs.data(), K, &cnt) == FELICS_OK;
                size_t at = 0;
                for (size_t j = 0; same && j < K; j++)
                    if (mark[j]) same = at < cnt && segs[at++] == j;
                if (!same || at != cnt) {
                    fprintf(stderr, "%s: felics_region_segments differs from the marking\n", n.c_str());
                    return 1;
                }
            }
            idx.assign(index.begin(), index.begin() + ilen);
            const int rounds = ilen > (1u << 20) ? 10 : 60;
            for (int m = 0; m < rounds; m++) {
                std::vector<uint8_t> bad = idx;
                const int flips = 1 + (int)(next() % 3);
                for (int f = 0; f < flips; f++) {
                    // header fields, the first checkpoints' offsets, or anywhere
                    const uint64_t r = next();
                    const size_t pos = (r & 3) == 0 ? (size_t)(next() % 64) : ((r & 3) == 1 && ilen > 64 ? 64 + (size_t)(next() % 8) : (size_t)(next() % ilen));
                    bad[pos] ^= (uint8_t)(1u << (next() % 8));
                }
                mutations++;
                if (felics_decompress_indexed(buf.data(), buf.size(), bad.data(), bad.size(), px.data(), px.size(), &h2) == FELICS_OK) mut_accepted++;
                if (!regions_on(bad, bad.size(), h, false, 2)) {
                    fprintf(stderr, "%s: a region of a mutated index wrote past its crop\n", n.c_str());
                    return 1;
                }
                view_on(bad, bad.size(), h, false);
                if (m % 10 == 0) {  // and cut short
                    const size_t cut = (size_t)(next() % ilen);
                    if (felics_decompress_indexed(buf.data(), buf.size(), bad.data(), cut, px.data(), px.size(), &h2) == FELICS_OK) {
                        fprintf(stderr, "%s: an index cut to %zu of %zu bytes was accepted\n", n.c_str(), cut, ilen);
                        return 1;
                    }
                }
            }
        }
    }
    printf("index_fuzz: %zu files, %zu indexes built, %zu refused, %zu pairs (%zu accepted), %zu mutations (%zu accepted), %zu regions, %zu views\n", names.size(),
           built, refused, pairs, pairs_ok, mutations, mut_accepted, regions, views);
    printf("index_fuzz: region plans of %zu streams with a valid header, %zu regions planned as felics_region_segments names them\n", plan_streams,
           plan_regions);
    return 0;
}
