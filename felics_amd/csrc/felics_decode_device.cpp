// felics_decode_device.cpp -- host side of the GPU decoder: streams of one shape (felics_decompress_batch_device), of any shapes
// (felics_decompress_images_device), into views (felics_decompress_views_device), through restart indexes (the dense, the region and
// the views call), and their headers (felics_read_headers_device).
#include "felics_host.h"
#include "felics_index.h"
#include "felics_viewcheck.h"

namespace felics {

namespace {

// ---- GPU decoder helpers shared by felics_decompress_batch_device and felics_decompress_images_device -----------------------

// Every stream gets a status on every path out of a decode call (felics.h): a call that ends before the streams are decoded reports
// its own error for all of them, and counts them as undecoded.
int fail_decode(felics_ctx *ctx, size_t n, int *status, int code) {
    for (size_t i = 0; i < n; i++) status[i] = code;
    ctx->dstats.undecoded += n;
    return code;
}

// The same before a call has counted its streams, for the entry points that also hand out headers and frame offsets.
int fail_call(size_t n, int *status, felics_header *hdrs, uint64_t *pix_offsets, int code) {
    for (size_t i = 0; i < n; i++) {
        status[i] = code;
        if (hdrs) hdrs[i] = felics_header{};
        if (pix_offsets) pix_offsets[i] = 0;
    }
    return code;
}

// 16-bit streams: estimator tables for passes of `per` <= n streams (at most DEC16_PASS, a stream's table is 8.4 MB of HBM, and at
// most a quarter of the free HBM; an allocation that fails all the same halves the pass)
int dec16_tables(felics_ctx *ctx, size_t n, size_t &per) {
    constexpr size_t DEC16_PASS = 1024;
    per = std::min(n, DEC16_PASS);
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && ctx->dec_table.cap < decode16_table_bytes((uint32_t)per))
        per = std::max<size_t>(1, std::min(per, (free_b / 4 + ctx->dec_table.cap) / decode16_table_bytes(1)));
    for (;;) {
        const size_t table_bytes = decode16_table_bytes((uint32_t)per);
        if (table_bytes > ctx->dec_table.cap) ctx->dec_epoch = ctx->dec_epoch_start;  // a fresh (zeroed) buffer: epochs start over
        const int rc = reserve_zeroed(ctx, ctx->dec_table, table_bytes);
        if (rc == 0) return FELICS_OK;
        (void)hipGetLastError();
        if (per == 1) return rc;
        per = (per + 1) / 2;
    }
}

// the first of the three epochs (one per plane) of the next pass on stream s
int dec16_epoch(felics_ctx *ctx, hipStream_t s, uint32_t &epoch0) {
    const EpochStep e = dec16_epoch_next(ctx->dec_epoch);  // (felics_epochs.h)
    if (e.clear) HIP_TRY(ctx, hipMemsetAsync(ctx->dec_table.p, 0, ctx->dec_table.cap, s));  // epochs used up: clear the tables, start over
    epoch0 = e.epoch;
    ctx->dec_epoch = e.epoch + 2;
    if (ctx->trace_epochs) fprintf(stderr, "[felics] decode16 epoch 0x%x clear %d\n", e.epoch, (int)e.clear);
    return FELICS_OK;
}

// FELICS_TEST_DECODE16_LANES, read per call: 1 = 16-bit streams take the lane form wherever the shape allows it (W >= 8; in a mixed
// call: whole waves of 64 streams of one shape), 0 = never, unset (-1) = from the measured thresholds on
int dec16_lanes_forced() {
    const char *e = getenv("FELICS_TEST_DECODE16_LANES");
    return e ? (atoi(e) != 0 ? 1 : 0) : -1;
}

// FELICS_TEST_DECODE16_LANES_PASS=k: at most k streams (rounded down to whole waves, at least one) in a pass of the 16-bit lane form (tests)
size_t dec16_lanes_pass_cap() {
    const char *e = getenv("FELICS_TEST_DECODE16_LANES_PASS");
    if (!e || atoll(e) <= 0) return SIZE_MAX / 2;
    return std::max<size_t>(64, (size_t)atoll(e) / 64 * 64);
}

// 16-bit lane form: the table buffer for passes of `bytes` <= want bytes (what the whole call would like), at least `least` (one
// wave's tables).  Bounded as dec16_tables bounds the wave form's: at most a quarter of the free HBM, and an allocation that fails
// all the same halves the pass.  "Free" counts the buffer the context already holds, so the bound is the same call after call: with
// free / 4 + cap a buffer of tens of GB grew a little with every call, and every growth is a free, an allocation and a memset
// (seconds: profiles/decode16_lanes.txt, first run).
int dec16_lanes_tables(felics_ctx *ctx, size_t want, size_t least, size_t &bytes) {
    bytes = want;
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && ctx->dec_lane16_table.cap < bytes)
        bytes = std::max(least, std::min(bytes, std::max(ctx->dec_lane16_table.cap, (free_b + ctx->dec_lane16_table.cap) / 4)));
    for (;;) {
        if (bytes > ctx->dec_lane16_table.cap) ctx->dec_lane16_epoch = ctx->dec_lane16_epoch_start;  // a fresh (zeroed) buffer: epochs start over
        const int rc = reserve_zeroed(ctx, ctx->dec_lane16_table, bytes);
        if (rc == 0) return FELICS_OK;
        (void)hipGetLastError();
        if (bytes <= least) return rc;
        bytes = std::max(least, bytes / 2);
    }
}

// the first of the three epochs (one per plane) of the next lane-form launch on stream s
int dec16_lanes_epoch(felics_ctx *ctx, hipStream_t s, uint32_t &epoch0) {
    const EpochStep e = dec16_lanes_epoch_next(ctx->dec_lane16_epoch);  // (felics_epochs.h)
    if (e.clear) HIP_TRY(ctx, hipMemsetAsync(ctx->dec_lane16_table.p, 0, ctx->dec_lane16_table.cap, s));  // epochs used up: clear the tables, start over
    epoch0 = e.epoch;
    ctx->dec_lane16_epoch = e.epoch + 2;
    if (ctx->trace_epochs) fprintf(stderr, "[felics] decode16 lanes epoch 0x%x clear %d\n", e.epoch, (int)e.clear);
    return FELICS_OK;
}

// FELICS_TEST_INDEX_LANES_PASS=k: at most k items (rounded down to whole waves, at least one) in a pass of the indexed lane form (tests)
uint64_t index_lanes_pass_cap() {
    const char *e = getenv("FELICS_TEST_INDEX_LANES_PASS");
    if (!e || atoll(e) <= 0) return UINT64_MAX;
    return std::max<uint64_t>(64, (uint64_t)atoll(e) / 64 * 64);
}

// Indexed lane form: dec_lane_table for passes of `bytes` <= want bytes (what the whole call would like), at least `least` (one
// wave's tables), bounded as dec16_lanes_tables bounds the 16-bit lane tables: at most a quarter of the free HBM, counting what the
// context already holds, and an allocation that fails all the same halves the pass.  (Nothing to zero: the kernel loads the rows.)
int index_lanes_tables(felics_ctx *ctx, size_t want, size_t least, size_t &bytes) {
    bytes = want;
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && ctx->dec_lane_table.cap < bytes)
        bytes = std::max(least, std::min(bytes, std::max(ctx->dec_lane_table.cap, (free_b + ctx->dec_lane_table.cap) / 4)));
    for (;;) {
        const int rc = reserve(ctx, ctx->dec_lane_table, bytes);
        if (rc == 0) return FELICS_OK;
        (void)hipGetLastError();
        if (bytes <= least) return rc;
        bytes = std::max(least, bytes / 2);
    }
}

constexpr int HOST_DECODE_NO_MEMORY = 1;  // (not a status: the host could not hold the stream)

// One stream through the host decoder (rows too wide for the LDS): copied to the host, decoded, the frame copied to d_dst.  A stream
// longer than max_len is FELICS_E_INVALID_VALUE before anything is sized by it; a header other than `want`,
// FELICS_E_INVALID_DIMENSIONS.  Returns the stream's status, FELICS_E_HIP (HIP error, ctx->err set) or HOST_DECODE_NO_MEMORY.
int host_decode(felics_ctx *ctx, const uint8_t *d_src, uint64_t len, uint64_t max_len, const felics_header &want, uint8_t *d_dst,
                std::vector<uint8_t> &sbuf, std::vector<uint8_t> &pbuf) {
    if (len > max_len) return FELICS_E_INVALID_VALUE;
    const uint64_t frame_bytes = (uint64_t)want.width * want.height * (want.color_type ? 3 : 1) * (want.pixel_depth ? 2 : 1);
    try {
        sbuf.resize((size_t)len);
        pbuf.resize((size_t)frame_bytes);
    } catch (const std::bad_alloc &) {
        return HOST_DECODE_NO_MEMORY;
    }
    if (len && hipMemcpy(sbuf.data(), d_src, (size_t)len, hipMemcpyDeviceToHost) != hipSuccess)
        return hip_fail(ctx, hipGetLastError(), "copying a stream to the host decoder");
    felics_header hi;
    int r = felics_read_header(sbuf.data(), sbuf.size(), &hi);
    if (!r && (hi.width != want.width || hi.height != want.height || hi.color_type != want.color_type || hi.pixel_depth != want.pixel_depth))
        r = FELICS_E_INVALID_DIMENSIONS;
    if (!r) r = felics_decompress(sbuf.data(), sbuf.size(), pbuf.data(), pbuf.size(), nullptr);
    if (!r && frame_bytes && hipMemcpy(d_dst, pbuf.data(), (size_t)frame_bytes, hipMemcpyHostToDevice) != hipSuccess)
        return hip_fail(ctx, hipGetLastError(), "copying decoded pixels to the device");
    return r;
}

// k_read_headers over n streams: offsets | lens | records in ctx->dec_meta (`extra` more bytes reserved behind them), the records
// copied back to `rec`; d_off / d_len stay on the device
int read_headers(felics_ctx *ctx, size_t n, const void *d_streams, const uint64_t *offsets, const uint64_t *lens, std::vector<DecodeHeader> &rec,
                 hipStream_t s) {
    int rc = reserve(ctx, ctx->dec_meta, n * 16 + n * sizeof(DecodeHeader));
    if (rc) return rc;
    try {
        rec.resize(n);
    } catch (const std::bad_alloc &) {
        return FELICS_E_IO;
    }
    uint64_t *d_off = (uint64_t *)ctx->dec_meta.p, *d_len = d_off + n;
    DecodeHeader *d_rec = (DecodeHeader *)(d_len + n);
    HIP_TRY(ctx, hipMemcpyAsync(d_off, offsets, n * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(ctx, hipMemcpyAsync(d_len, lens, n * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(ctx, launch_read_headers(s, (const uint8_t *)d_streams, d_off, d_len, (uint32_t)n, d_rec));
    HIP_TRY(ctx, hipMemcpyAsync(rec.data(), d_rec, n * sizeof(DecodeHeader), hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipStreamSynchronize(s));
    return FELICS_OK;
}

// Streams `idx` grouped by (colour, W, H), stream order kept within a group: of every group the first take(header, count) streams
// become a lane group of their colour, the others are appended to `rest`.
template <typename Take>
void same_shape_groups(const std::vector<DecodeHeader> &rec, std::vector<size_t> idx, std::vector<std::vector<size_t>> (&groups)[2],
                       std::vector<size_t> &rest, Take take) {
    auto shape = [&](size_t i) { return std::make_tuple(rec[i].color, rec[i].W, rec[i].H); };
    std::stable_sort(idx.begin(), idx.end(), [&](size_t a, size_t b) { return shape(a) < shape(b); });
    for (size_t k = 0; k < idx.size();) {
        size_t e = k;
        while (e < idx.size() && shape(idx[e]) == shape(idx[k])) e++;
        const size_t lanes = take(rec[idx[k]], e - k);
        if (lanes) groups[rec[idx[k]].color].emplace_back(idx.begin() + k, idx.begin() + k + lanes);
        rest.insert(rest.end(), idx.begin() + k + lanes, idx.begin() + e);
        k = e;
    }
}

// felics_decompress_views_device: where the streams of one pass of the call write.  cls[i] is view i's class, worked out from the
// view alone (a stream whose header differs from its view is not decoded at all); stage[i] is the offset of a scattered stream's
// dense frame in ctx->view_stage.
enum : uint8_t { VIEW_DENSE = 0, VIEW_IN_PLACE, VIEW_SCATTERED };
struct ViewPlan {
    const felics_view *views;
    const uint8_t *cls;
    const uint64_t *stage;
};

// rows too wide for the LDS of either wave form: the host decoder's
bool rows_for_host(uint32_t W, uint32_t color, uint32_t depth) {
    return depth ? decode16_lds_bytes(W) > DECODE_LDS_LIMIT : decode8_lds_bytes(W, color) > DECODE_LDS_LIMIT;
}

// felics_decompress_images_device after the argument checks.  Every stream's header is read on the device (k_read_headers); the
// frames are laid out in stream order; each stream then takes one of five forms:
//   - 8-bit, 64 streams of one shape per wave (k_decode8_lanes) -- groups of >= 64 streams of one shape, W >= 8, in a call with
//     as many 8-bit streams as the same-shape entry point wants for that form;
//   - 8-bit, a wave per stream (k_decode8), rows in LDS classes, longest streams first, a class per launch and stream;
//   - 16-bit, 64 streams of one shape per wave (k_decode16_lanes) -- whole waves out of groups of >= 64 streams of one shape and colour,
//     W >= 8, in a call with as many 16-bit streams as the same-shape entry point wants for that form; passes bounded by the
//     hashed tables' memory;
//   - 16-bit, a wave per stream (k_decode16), passes bounded by the estimator tables' memory;
//   - the host decoder, stream by stream (rows wider than the LDS holds).
// The GPU forms run on distinct streams of the context, joined with events before the statuses come back.
//
// With a ViewPlan (felics_decompress_views_device) the same call writes views: d_pixels is nullptr and pix_offsets[i] becomes the
// ADDRESS of stream i's dense frame (the view itself if it is dense, its frame in view_stage if it is scattered) or of its view's
// first sample, so the tables' out_off are absolute; a table of ViewRow runs beside the rows and one beside the slots, and a launch
// that holds a pitched gray view or a strided RGB one takes the kernels' pitched / strided policies.  Behind the join, one kernel
// per sample type writes the staged frames through their views.  The caller's ready event goes in front of everything (wait_ready).
int decompress_images(felics_ctx *ctx, size_t n, const void *d_streams, const uint64_t *offsets, const uint64_t *lens, uint8_t *d_pixels,
                      size_t cap, uint64_t *pix_offsets, felics_header *hdrs, int *status, const ViewPlan *vp = nullptr) {
    Lane &l0 = ctx->lanes[0];
    hipStream_t s = l0.stream;
    felics_decode_stats &ds = ctx->dstats;
    ds.streams += n;
    ds.lanes16_table_bytes = 0;
    auto fail_all = [&](int code) { return fail_decode(ctx, n, status, code); };
    std::vector<DecodeHeader> rec;
    int rc = vp ? wait_ready(ctx, s) : FELICS_OK;  // (the header kernel reads stream bytes)
    if (!rc) rc = read_headers(ctx, n, d_streams, offsets, lens, rec, s);
    if (rc) return fail_all(rc);
    // layout in stream order; a stream that will not be decoded gets no bytes
    uint64_t at = 0;
    std::vector<uint64_t> npix(n, 0);
    for (size_t i = 0; i < n; i++) {
        const DecodeHeader &h = rec[i];
        if (hdrs) hdrs[i] = h.status == FELICS_OK ? felics_header{h.color, h.depth, h.W, h.H} : felics_header{};
        status[i] = h.dstatus;
        pix_offsets[i] = at;
        if (h.dstatus != FELICS_OK) continue;
        if (vp) {  // the view names the shape: another one is not decoded, and nothing of the view is written
            const felics_view &w = vp->views[i];
            if ((int)h.color != w.color || (int)h.depth != w.depth || h.W != w.width || h.H != w.height) {
                status[i] = FELICS_E_INVALID_DIMENSIONS;
                continue;
            }
            npix[i] = (uint64_t)h.W * h.H;
            const bool staged = vp->cls[i] == VIEW_SCATTERED;
            pix_offsets[i] = staged ? (uint64_t)(uintptr_t)ctx->view_stage.p + vp->stage[i] : (uint64_t)(uintptr_t)w.data;
            if (staged) ctx->dvstats.bytes_staged += npix[i] * (h.color ? 3 : 1) * (h.depth ? 2 : 1);
            continue;
        }
        npix[i] = (uint64_t)h.W * h.H;
        at = (at + npix[i] * (h.color ? 3 : 1) * (h.depth ? 2 : 1) + 15) & ~15ull;
    }
    const uint64_t needed = at;
    if (needed > cap) {
        for (size_t i = 0; i < n; i++)
            if (status[i] == FELICS_OK) status[i] = FELICS_E_BUFFER_TOO_SMALL;
        pix_offsets[0] = needed;
        ds.undecoded += n;
        return FELICS_E_BUFFER_TOO_SMALL;
    }
    if (needed && !d_pixels) return fail_all(FELICS_E_INVALID_ARGUMENT);
    // forms
    int forced = -1;  // FELICS_TEST_DECODE_LANES=1 / =0: every same-shape group with W >= 8 / none in the lane form (tests)
    if (const char *e = getenv("FELICS_TEST_DECODE_LANES")) forced = atoi(e) != 0;
    std::vector<size_t> idx8, wave8, rows16, host;
    for (size_t i = 0; i < n; i++) {
        const DecodeHeader &h = rec[i];
        if (status[i] != FELICS_OK) continue;
        if (rows_for_host(h.W, h.color, h.depth)) host.push_back(i);
        else if (!h.depth) idx8.push_back(i);
        else rows16.push_back(i);
    }
    const size_t n8 = idx8.size(), n16 = rows16.size();
    // lane groups [colour]: GPU streams of one shape, in stream order within a group.  8-bit: in a call with as many 8-bit streams as
    // the same-shape entry point wants for that form, the whole waves of every group with W >= 8 (FELICS_TEST_DECODE_LANES=1: all of
    // it, =0: none).  16-bit: the same rule over the 16-bit GPU streams (FELICS_TEST_DECODE16_LANES=1: in any call; =0: none).  The
    // rest of a group and every other stream keep the wave form.
    std::vector<std::vector<size_t>> lane_groups[2], lane16_groups[2];
    same_shape_groups(rec, idx8, lane_groups, wave8, [&](const DecodeHeader &h, size_t cnt) -> size_t {
        if (h.W < 8) return 0;
        if (forced >= 0) return forced ? cnt : 0;
        return n8 >= (h.color ? DECODE8_LANES_MIN_STREAMS_RGB : DECODE8_LANES_MIN_STREAMS) ? cnt / 64 * 64 : 0;
    });
    const int forced16 = dec16_lanes_forced();
    if (forced16 != 0 && n16 >= 64) {
        std::vector<size_t> rest;
        same_shape_groups(rec, rows16, lane16_groups, rest, [&](const DecodeHeader &h, size_t cnt) -> size_t {
            const bool enough = forced16 == 1 || n16 >= (h.color ? DECODE16_LANES_MIN_STREAMS_RGB : DECODE16_LANES_MIN_STREAMS);
            return h.W >= 8 && enough ? cnt / 64 * 64 : 0;
        });
        std::sort(rest.begin(), rest.end());  // (stream order again, as without this form)
        rows16.swap(rest);
    }
    auto longest_first = [&](std::vector<size_t> &v) {
        std::stable_sort(v.begin(), v.end(), [&](size_t a, size_t b) { return npix[a] > npix[b]; });
    };
    longest_first(wave8);
    longest_first(rows16);
    // RGB8 planes (int16) of the wave rows and the lane slots
    uint64_t planes8 = 0;
    auto plane8_of = [&](size_t i) {
        const uint64_t o = planes8;
        planes8 += 3 * npix[i];
        return o;
    };
    // wave-form rows in LDS classes: a class's launch asks for its widest row's LDS, so a thin image does not share a
    // launch (and its residency) with a very wide one
    constexpr uint32_t LDS_CLASS[] = {16u << 10, 32u << 10, 64u << 10, DECODE_LDS_LIMIT};
    constexpr int NCLASS = 4;
    std::vector<DecodeRow> rows;
    std::vector<LaneWave> waves;
    std::vector<LaneSlot> slots;
    // views: a ViewRow beside every row and every slot (felics_kernels.h, DecodeViews)
    std::vector<ViewRow> rviews, sviews;
    auto pitched = [&](size_t i) { return vp && !rec[i].color && vp->cls[i] == VIEW_IN_PLACE; };
    auto strided = [&](size_t i) { return vp && rec[i].color && vp->cls[i] == VIEW_IN_PLACE; };
    auto view_row = [&](size_t i) {
        const felics_view &w = vp->views[i];
        if (w.color) return ViewRow{w.data, w.row_stride, w.pixel_stride, w.channel_stride};
        const int64_t size = w.depth ? 2 : 1;  // gray: the view's pitch, or the dense frame's (the view's own or the staged one)
        if (pitched(i)) return ViewRow{w.data, w.row_stride, size, 0};
        return ViewRow{(const void *)(uintptr_t)pix_offsets[i], (int64_t)w.width * size, size, 0};
    };
    auto push_row = [&](const DecodeRow &r) {
        rows.push_back(r);
        if (vp) rviews.push_back(view_row(r.stream));
    };
    auto push_slot = [&](const LaneSlot &sl) {
        slots.push_back(sl);
        if (vp) sviews.push_back(view_row(sl.stream));
    };
    struct Launch {
        size_t first, cnt;
        uint32_t lds;
        uint64_t max_npix;
        bool rgb;
        bool pitched = false, strided = false;  // (views) it holds a pitched gray view / a strided RGB one
    };
    std::vector<Launch> classes;
    for (int c = 0; c < NCLASS; c++) {
        Launch L{rows.size(), 0, 0, 0, false};
        for (size_t i : wave8) {
            const uint32_t lds = decode8_lds_bytes(rec[i].W, rec[i].color);
            if (lds > LDS_CLASS[c] || (c > 0 && lds <= LDS_CLASS[c - 1])) continue;
            const uint64_t poff = rec[i].color ? plane8_of(i) : 0;
            push_row(DecodeRow{(uint32_t)i, rec[i].W, rec[i].H, rec[i].color, pix_offsets[i], poff});
            L.pitched = L.pitched || pitched(i);
            L.strided = L.strided || strided(i);
            L.cnt++;
            L.lds = std::max(L.lds, lds);
            L.max_npix = std::max(L.max_npix, npix[i]);
            L.rgb = L.rgb || rec[i].color;
        }
        if (L.cnt) classes.push_back(L);
    }
    // lane form: waves of up to 64 slots of one shape; gray slots first, then RGB (each colour one launch, its tables behind the other's)
    Launch lanes[2] = {};  // first / cnt index waves; max_npix; conversion rows of the RGB slots: `conv`
    size_t slot0[2] = {0, 0};
    Launch conv{0, 0, 0, 0, true};
    for (int col = 0; col < 2; col++) {
        lanes[col].first = waves.size();
        slot0[col] = slots.size();
        for (const auto &g : lane_groups[col]) {
            for (size_t k = 0; k < g.size(); k += 64) {
                const uint32_t cnt = (uint32_t)std::min<size_t>(64, g.size() - k);
                waves.push_back(LaneWave{rec[g[k]].W, rec[g[k]].H, (uint32_t)(slots.size() - slot0[col]), cnt});
                for (uint32_t j = 0; j < cnt; j++) {
                    const size_t i = g[k + j];
                    const uint64_t poff = col ? plane8_of(i) : 0;
                    push_slot(LaneSlot{(uint32_t)i, 0, col ? poff : pix_offsets[i]});
                    lanes[col].pitched = lanes[col].pitched || pitched(i);
                    if (col) {
                        if (!conv.cnt) conv.first = rows.size();
                        push_row(DecodeRow{(uint32_t)i, rec[i].W, rec[i].H, 1, pix_offsets[i], poff});
                        conv.strided = conv.strided || strided(i);
                        conv.cnt++;
                    }
                    lanes[col].max_npix = std::max(lanes[col].max_npix, npix[i]);
                }
            }
        }
        lanes[col].cnt = waves.size() - lanes[col].first;
    }
    const size_t nslots8 = slots.size();  // (the 16-bit lane form's slots and waves follow)
    // 16-bit lane form: passes of whole waves of one colour, each within the table memory dec16_lanes_tables grants; a pass's slots
    // name their tables by row (LaneSlot::table_row) and its RGB planes start over at the front of dec_planes16
    struct LanePass16 {
        int col;
        size_t wave_first, wave_cnt, slot_first, conv_first, conv_cnt;
        uint64_t max_npix;
        bool pitched = false, strided = false;
    };
    std::vector<LanePass16> passes16;
    uint64_t lane_planes16 = 0;  // int32 samples of the largest lane pass's RGB planes
    size_t nlanes16 = 0;
    {
        uint64_t want_rows = 0, least_rows = 0;
        auto slot_rows = [&](size_t i) { return (uint64_t)(rec[i].color ? 3 : 1) * dec16l_rows(npix[i], rec[i].color ? 3 : 1); };
        for (int col = 0; col < 2; col++)
            for (const auto &g : lane16_groups[col]) {
                want_rows += slot_rows(g[0]) * g.size();
                least_rows = std::max(least_rows, slot_rows(g[0]) * 64);
                nlanes16 += g.size();
            }
        size_t tbytes = 0;
        if (nlanes16 && (rc = dec16_lanes_tables(ctx, (size_t)want_rows * DEC16L_ROW_BYTES, (size_t)least_rows * DEC16L_ROW_BYTES, tbytes)) != 0)
            return fail_all(rc);
        const uint64_t pass_rows = tbytes / DEC16L_ROW_BYTES;
        const size_t pass_streams = dec16_lanes_pass_cap();
        uint64_t used_rows = 0, poff = 0, most_rows = 0;
        size_t in_pass = 0;
        for (int col = 0; col < 2; col++)
            for (const auto &g : lane16_groups[col])
                for (size_t k = 0; k < g.size(); k += 64) {
                    const uint64_t wave_rows = slot_rows(g[k]) * 64;
                    if (passes16.empty() || passes16.back().col != col || used_rows + wave_rows > pass_rows || in_pass + 64 > pass_streams) {
                        passes16.push_back(LanePass16{col, waves.size(), 0, slots.size(), rows.size(), 0, 0});
                        used_rows = poff = 0;
                        in_pass = 0;
                    }
                    LanePass16 &P = passes16.back();
                    waves.push_back(LaneWave{rec[g[k]].W, rec[g[k]].H, (uint32_t)(slots.size() - P.slot_first), 64});
                    P.wave_cnt++;
                    for (uint32_t j = 0; j < 64; j++) {
                        const size_t i = g[k + j];
                        push_slot(LaneSlot{(uint32_t)i, (uint32_t)used_rows, col ? poff : pix_offsets[i] / 2});
                        P.pitched = P.pitched || pitched(i);
                        P.strided = P.strided || strided(i);
                        if (col) {
                            push_row(DecodeRow{(uint32_t)i, rec[i].W, rec[i].H, 1, pix_offsets[i], poff});
                            P.conv_cnt++;
                            poff += 3 * npix[i];
                        }
                        used_rows += slot_rows(i);
                        P.max_npix = std::max(P.max_npix, npix[i]);
                    }
                    in_pass += 64;
                    lane_planes16 = std::max(lane_planes16, poff);
                    most_rows = std::max(most_rows, used_rows);
                }
        ds.lanes16_table_bytes = most_rows * DEC16L_ROW_BYTES;
    }
    // 16-bit rows (passes below) behind the others
    const size_t rows16_first = rows.size();
    size_t per16 = 0;
    uint64_t planes16 = lane_planes16;  // int32 samples: the lane passes' RGB planes, the largest wave pass's behind them
    if (!rows16.empty()) {
        if ((rc = dec16_tables(ctx, rows16.size(), per16)) != 0) return fail_all(rc);
        for (size_t p = 0; p < rows16.size(); p += per16) {
            uint64_t poff = lane_planes16;
            for (size_t k = p; k < std::min(rows16.size(), p + per16); k++) {
                const size_t i = rows16[k];
                push_row(DecodeRow{(uint32_t)i, rec[i].W, rec[i].H, rec[i].color, pix_offsets[i], poff});
                if (rec[i].color) poff += 3 * npix[i];
            }
            planes16 = std::max(planes16, poff);
        }
    }
    // views: the scattered streams that may be decoded -- their frames are written through the views behind the join
    size_t nscat = 0;
    for (size_t i = 0; vp && i < n; i++) nscat += status[i] == FELICS_OK && vp->cls[i] == VIEW_SCATTERED;
    // device side: offsets | lens | status | rows | waves | slots (offsets and lens again: the buffer may have moved); views: | the
    // rows' views | the slots' views | the scatter table
    auto al = [](size_t b) { return (b + 15) & ~(size_t)15; };
    const size_t o_status = n * 16, o_rows = o_status + al(n * 4), o_waves = o_rows + al(rows.size() * sizeof(DecodeRow)),
                 o_slots = o_waves + al(waves.size() * sizeof(LaneWave)), o_rviews = o_slots + al(slots.size() * sizeof(LaneSlot)),
                 o_sviews = o_rviews + al(rviews.size() * sizeof(ViewRow)), o_scat = o_sviews + al(sviews.size() * sizeof(ViewRow)),
                 o_end = o_scat + nscat * sizeof(ScatterRow);
    if ((rc = reserve(ctx, ctx->dec_meta, o_end)) != 0) return fail_all(rc);
    uint8_t *meta = (uint8_t *)ctx->dec_meta.p;
    uint64_t *d_off = (uint64_t *)meta, *d_len = d_off + n;
    int *d_status = (int *)(meta + o_status);
    DecodeRow *d_rows = (DecodeRow *)(meta + o_rows);
    LaneWave *d_waves = (LaneWave *)(meta + o_waves);
    LaneSlot *d_slots = (LaneSlot *)(meta + o_slots);
    ViewRow *d_rviews = (ViewRow *)(meta + o_rviews), *d_sviews = (ViewRow *)(meta + o_sviews);
    ScatterRow *d_scat = (ScatterRow *)(meta + o_scat);
    std::vector<ScatterRow> scat[2];  // [depth]
    if (planes8 && (rc = reserve(ctx, ctx->dec_planes, planes8 * 2 + 64)) != 0) return fail_all(rc);
    if (planes16 && (rc = reserve(ctx, ctx->dec_planes16, planes16 * 4 + 64)) != 0) return fail_all(rc);
    const size_t lt_gray = decode8_lanes_table_bytes((uint32_t)(slot0[1] - slot0[0]), 0);
    const size_t lt_bytes = lt_gray + decode8_lanes_table_bytes((uint32_t)(nslots8 - slot0[1]), 1);
    if (nslots8 && (rc = reserve(ctx, ctx->dec_lane_table, lt_bytes)) != 0) return fail_all(rc);
    std::vector<int> dev_status(status, status + n);
    for (size_t i = 0; i < n; i++)
        if (dev_status[i] == FELICS_OK) dev_status[i] = FELICS_E_HIP;  // until the kernel's own word arrives
    for (size_t i : host) dev_status[i] = FELICS_OK;
    for (size_t i = 0; i < n; i++) ds.undecoded += status[i] != FELICS_OK;
    ds.wave8 += wave8.size();
    ds.lanes8 += n8 - wave8.size();
    ds.wave16 += rows16.size();
    ds.lanes16 += nlanes16;
    ds.host += host.size();
    auto queue = [&]() -> int {
        HIP_TRY(ctx, hipMemcpyAsync(d_off, offsets, n * 8, hipMemcpyHostToDevice, s));
        HIP_TRY(ctx, hipMemcpyAsync(d_len, lens, n * 8, hipMemcpyHostToDevice, s));
        HIP_TRY(ctx, hipMemcpyAsync(d_status, dev_status.data(), n * 4, hipMemcpyHostToDevice, s));
        if (!rows.empty()) HIP_TRY(ctx, hipMemcpyAsync(d_rows, rows.data(), rows.size() * sizeof(DecodeRow), hipMemcpyHostToDevice, s));
        if (!waves.empty()) HIP_TRY(ctx, hipMemcpyAsync(d_waves, waves.data(), waves.size() * sizeof(LaneWave), hipMemcpyHostToDevice, s));
        if (!slots.empty()) HIP_TRY(ctx, hipMemcpyAsync(d_slots, slots.data(), slots.size() * sizeof(LaneSlot), hipMemcpyHostToDevice, s));
        if (!rviews.empty()) HIP_TRY(ctx, hipMemcpyAsync(d_rviews, rviews.data(), rviews.size() * sizeof(ViewRow), hipMemcpyHostToDevice, s));
        if (!sviews.empty()) HIP_TRY(ctx, hipMemcpyAsync(d_sviews, sviews.data(), sviews.size() * sizeof(ViewRow), hipMemcpyHostToDevice, s));
        // the launches that do not depend on each other go to distinct streams of the context, behind the uploads
        std::vector<hipStream_t> work;
        for (int li = 0; li < ctx->nlanes; li++) {
            Lane &l = ctx->lanes[li];
            for (hipStream_t w : {l.front, l.kstream, li ? l.stream : l.tail})
                if (w && std::find(work.begin(), work.end(), w) == work.end()) work.push_back(w);
        }
        HIP_TRY(ctx, hipEventRecord(l0.slice_done[0], s));
        for (hipStream_t w : work) HIP_TRY(ctx, hipStreamWaitEvent(w, l0.slice_done[0], 0));
        size_t next = 0;
        auto stream_for = [&]() { return work[next++ % work.size()]; };
        const uint8_t *st = (const uint8_t *)d_streams;
        if (!rows16.empty()) {
            hipStream_t w = stream_for();
            for (size_t p = 0; p < rows16.size(); p += per16) {
                const size_t cnt = std::min(per16, rows16.size() - p);
                uint32_t lds = 0, epoch0 = 0;
                uint64_t mx = 0;
                bool rgb = false;
                DecodeViews dv{d_rviews + rows16_first + p, false, false};
                for (size_t k = p; k < p + cnt; k++) {
                    const size_t i = rows16[k];
                    lds = std::max(lds, decode16_lds_bytes(rec[i].W));
                    mx = std::max(mx, npix[i]);
                    rgb = rgb || rec[i].color;
                    dv.pitched = dv.pitched || pitched(i);
                    dv.strided = dv.strided || strided(i);
                }
                int r = dec16_epoch(ctx, w, epoch0);
                if (r) return r;
                if (vp)
                    HIP_TRY(ctx, launch_decode16_rows_views(w, st, d_off, d_len, d_rows + rows16_first + p, (uint32_t)cnt, lds, mx, rgb,
                                                            (int32_t *)ctx->dec_planes16.p, (uint32_t *)ctx->dec_table.p, epoch0, d_status, dv));
                else
                    HIP_TRY(ctx, launch_decode16_rows(w, st, d_off, d_len, d_rows + rows16_first + p, (uint32_t)cnt, lds, mx, rgb, (uint16_t *)d_pixels,
                                                      (int32_t *)ctx->dec_planes16.p, (uint32_t *)ctx->dec_table.p, epoch0, d_status));
            }
        }
        if (nslots8) {
            hipStream_t w = stream_for();
            HIP_TRY(ctx, hipMemsetAsync(ctx->dec_lane_table.p, 0, lt_bytes, w));
            for (int col = 0; col < 2; col++)
                if (vp)
                    HIP_TRY(ctx, launch_decode8_lanes_waves_views(w, st, d_off, d_len, d_waves + lanes[col].first, (uint32_t)lanes[col].cnt,
                                                                  d_slots + slot0[col], col, d_rows + conv.first, (uint32_t)conv.cnt, lanes[1].max_npix,
                                                                  (int16_t *)ctx->dec_planes.p,
                                                                  (uint32_t *)((uint8_t *)ctx->dec_lane_table.p + (col ? lt_gray : 0)), d_status,
                                                                  DecodeViews{d_sviews + slot0[col], lanes[col].pitched, false},
                                                                  DecodeViews{d_rviews + conv.first, false, conv.strided}));
                else
                    HIP_TRY(ctx, launch_decode8_lanes_waves(w, st, d_off, d_len, d_waves + lanes[col].first, (uint32_t)lanes[col].cnt, d_slots + slot0[col],
                                                            col, d_rows + conv.first, (uint32_t)conv.cnt, lanes[1].max_npix, d_pixels,
                                                            (int16_t *)ctx->dec_planes.p, (uint32_t *)((uint8_t *)ctx->dec_lane_table.p + (col ? lt_gray : 0)),
                                                            d_status));
        }
        if (!passes16.empty()) {
            hipStream_t w = stream_for();
            for (const LanePass16 &P : passes16) {
                uint32_t epoch0 = 0;
                int r = dec16_lanes_epoch(ctx, w, epoch0);
                if (r) return r;
                if (vp)
                    HIP_TRY(ctx, launch_decode16_lanes_waves_views(w, st, d_off, d_len, d_waves + P.wave_first, (uint32_t)P.wave_cnt, d_slots + P.slot_first,
                                                                   P.col, d_rows + P.conv_first, (uint32_t)P.conv_cnt, P.max_npix,
                                                                   (int32_t *)ctx->dec_planes16.p, (uint32_t *)ctx->dec_lane16_table.p, epoch0, d_status,
                                                                   DecodeViews{d_sviews + P.slot_first, P.pitched, false},
                                                                   DecodeViews{d_rviews + P.conv_first, false, P.strided}));
                else
                    HIP_TRY(ctx, launch_decode16_lanes_waves(w, st, d_off, d_len, d_waves + P.wave_first, (uint32_t)P.wave_cnt, d_slots + P.slot_first, P.col,
                                                             d_rows + P.conv_first, (uint32_t)P.conv_cnt, P.max_npix, (uint16_t *)d_pixels,
                                                             (int32_t *)ctx->dec_planes16.p, (uint32_t *)ctx->dec_lane16_table.p, epoch0, d_status));
            }
        }
        for (const Launch &L : classes)
            if (vp)
                HIP_TRY(ctx, launch_decode8_rows_views(stream_for(), st, d_off, d_len, d_rows + L.first, (uint32_t)L.cnt, L.lds, L.max_npix, L.rgb,
                                                       (int16_t *)ctx->dec_planes.p, d_status, DecodeViews{d_rviews + L.first, L.pitched, L.strided}));
            else
                HIP_TRY(ctx, launch_decode8_rows(stream_for(), st, d_off, d_len, d_rows + L.first, (uint32_t)L.cnt, L.lds, L.max_npix, L.rgb, d_pixels,
                                                 (int16_t *)ctx->dec_planes.p, d_status));
        // the host decoder meanwhile (into frames no kernel writes)
        std::vector<uint8_t> sbuf, pbuf;
        if (vp && ctx->view_ready && !host.empty()) HIP_TRY(ctx, hipStreamWaitEvent(nullptr, ctx->view_ready, 0));  // (its copies run on the null stream)
        for (size_t i : host) {
            const felics_header want{rec[i].color, rec[i].depth, rec[i].W, rec[i].H};
            const int r = host_decode(ctx, st + offsets[i], lens[i], felics_max_compressed_size(rec[i].W, rec[i].H, rec[i].color, rec[i].depth), want,
                                      d_pixels + pix_offsets[i], sbuf, pbuf);
            if (r == FELICS_E_HIP) return r;
            status[i] = r == HOST_DECODE_NO_MEMORY ? FELICS_E_IO : r;
        }
        const size_t used = std::min(next, work.size());
        for (size_t k = 0; k < used; k++) {
            HIP_TRY(ctx, hipEventRecord(l0.spine_done[k], work[k]));
            HIP_TRY(ctx, hipStreamWaitEvent(s, l0.spine_done[k], 0));
        }
        if (nscat) {
            // the staged frames through their views: the kernels' (they look at the stream's status on the device) and the host
            // decoder's (those it decoded)
            uint32_t row_samples[2] = {0, 0}, max_h[2] = {0, 0};
            for (size_t i = 0; i < n; i++) {
                if (status[i] != FELICS_OK || vp->cls[i] != VIEW_SCATTERED || !npix[i]) continue;
                const felics_view &w = vp->views[i];
                const uint32_t C = w.color ? 3 : 1, d = w.depth ? 1 : 0;
                scat[d].push_back(ScatterRow{(uint32_t)i, w.width, w.height, C, (const void *)(uintptr_t)pix_offsets[i],
                                             ViewRow{w.data, w.row_stride, w.pixel_stride, w.color ? w.channel_stride : 0}});
                row_samples[d] = (uint32_t)std::min<uint64_t>(std::max<uint64_t>(row_samples[d], (uint64_t)w.width * C), 0xFFFFFFFFu);
                max_h[d] = std::max(max_h[d], w.height);
            }
            ScatterRow *d_scat16 = d_scat + scat[0].size();
            if (!scat[0].empty()) {
                HIP_TRY(ctx, hipMemcpyAsync(d_scat, scat[0].data(), scat[0].size() * sizeof(ScatterRow), hipMemcpyHostToDevice, s));
                HIP_TRY(ctx, launch_scatter_views<uint8_t>(s, d_scat, (uint32_t)scat[0].size(), row_samples[0], max_h[0], d_status));
            }
            if (!scat[1].empty()) {
                HIP_TRY(ctx, hipMemcpyAsync(d_scat16, scat[1].data(), scat[1].size() * sizeof(ScatterRow), hipMemcpyHostToDevice, s));
                HIP_TRY(ctx, launch_scatter_views<uint16_t>(s, d_scat16, (uint32_t)scat[1].size(), row_samples[1], max_h[1], d_status));
            }
        }
        HIP_TRY(ctx, hipMemcpyAsync(dev_status.data(), d_status, n * 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(ctx, hipStreamSynchronize(s));
        return FELICS_OK;
    };
    if ((rc = queue()) != 0) {
        for (size_t i = 0; i < n; i++) status[i] = FELICS_E_HIP;
        return rc;
    }
    std::vector<char> on_host(n, 0);
    for (size_t i : host) on_host[i] = 1;
    int first = FELICS_OK;
    for (size_t i = 0; i < n; i++) {
        if (!on_host[i]) status[i] = dev_status[i];
        if (status[i] && !first) first = status[i];
    }
    return first;
}

// What a pass of `most` same-shape 16-bit streams needs beside its tables: offsets | lens | status in dec_meta and, RGB, the int32
// planes in dec_planes.
int dec16_buffers(felics_ctx *ctx, size_t most, const felics_header &hdr) {
    int rc = reserve(ctx, ctx->dec_meta, most * 8 * 2 + most * 4);
    if (!rc && hdr.color_type == FELICS_COLOR_RGB) rc = reserve(ctx, ctx->dec_planes, (size_t)((uint64_t)hdr.width * hdr.height * 3 * 4 * most) + 64);
    return rc;
}

// The passes of the same-shape 16-bit decoders (a wave per stream: launch_decode16 on dec_table; 64 streams per wave:
// launch_decode16_lanes on dec_lane16_table): n streams of shape `hdr`, `per` to a pass, every pass with fresh epochs on its table.
int decode16_passes(felics_ctx *ctx, size_t n, size_t per, const void *d_streams, const uint64_t *offsets, const uint64_t *lens, const felics_header &hdr,
                    void *d_pixels, decltype(&launch_decode16) launch, const DevBuf &table, int (*next_epoch)(felics_ctx *, hipStream_t, uint32_t &),
                    int *status) {
    const bool rgb = hdr.color_type == FELICS_COLOR_RGB;
    const uint64_t frame_samples = (uint64_t)hdr.width * hdr.height * (rgb ? 3 : 1);
    int32_t *d_planes32 = rgb ? (int32_t *)ctx->dec_planes.p : nullptr;
    int rc;
    hipStream_t s = ctx->lanes[0].stream;
    for (size_t i = 0; i < n; i++) status[i] = FELICS_E_HIP;  // until the kernel's own word arrives
    int first_rc = FELICS_OK;
    for (size_t first = 0; first < n; first += per) {
        const size_t cnt = std::min(per, n - first);
        uint32_t epoch0 = 0;
        if ((rc = next_epoch(ctx, s, epoch0)) != 0) return rc;
        uint64_t *d_off = (uint64_t *)ctx->dec_meta.p, *d_len = d_off + cnt;
        int *d_status = (int *)(d_len + cnt);
        HIP_TRY(ctx, hipMemcpyAsync(d_off, offsets + first, cnt * 8, hipMemcpyHostToDevice, s));
        HIP_TRY(ctx, hipMemcpyAsync(d_len, lens + first, cnt * 8, hipMemcpyHostToDevice, s));
        HIP_TRY(ctx, hipMemsetAsync(d_status, 0xFF, cnt * 4, s));
        HIP_TRY(ctx, launch(s, (const uint8_t *)d_streams, d_off, d_len, (uint32_t)cnt, hdr.width, hdr.height, hdr.color_type,
                            (uint16_t *)d_pixels + first * frame_samples, d_planes32, (uint32_t *)table.p, epoch0, d_status));
        HIP_TRY(ctx, hipMemcpyAsync(status + first, d_status, cnt * 4, hipMemcpyDeviceToHost, s));
        HIP_TRY(ctx, hipStreamSynchronize(s));
        for (size_t i = first; i < first + cnt && !first_rc; i++)
            if (status[i]) first_rc = status[i];
    }
    return first_rc;
}

// ---- the indexed calls: dense (felics_decompress_batch_device_indexed, _indexed16), regions (felics_decompress_regions_device_indexed,
// _indexed16) and views (felics_decompress_views_device_indexed, _indexed16).  One driver per call kind (dense_indexed, regions_indexed,
// decompress_views_indexed); what the depths differ in is a form: Depth8 / Depth16 for every kind, IndexSame8 / IndexSame16 on top
// of them for the two same-shape kinds, IndexViews8 / IndexViews16 for the views.  Regions into views
// (felics_decompress_region_views_device_indexed, _indexed16) are a fourth kind: region_views_indexed, RegionViews8 / RegionViews16.

int first_error(const int *status, size_t n) {
    for (size_t i = 0; i < n; i++)
        if (status[i]) return status[i];
    return FELICS_OK;
}

// FELICS_TEST_INDEX16_PASS=k: at most k waves in a pass of the 16-bit calls (tests)
uint64_t index16_pass_cap(uint64_t items) {
    if (const char *e = getenv("FELICS_TEST_INDEX16_PASS"))
        if (atoll(e) > 0) return std::min<uint64_t>(items, (uint64_t)atoll(e));
    return items;
}

// FELICS_TEST_INDEX_VIEWS_PASS=<bytes>: at most that many bytes of RGB planes in a pass of felics_decompress_views_device_indexed (tests)
uint64_t index_views_pass_cap() {
    const char *e = getenv("FELICS_TEST_INDEX_VIEWS_PASS");
    return e && atoll(e) > 0 ? (uint64_t)atoll(e) : UINT64_MAX;
}

// 8-bit streams, version-1 indexes.  A launch holds any number of items and needs nothing beside the call's tables.
struct Depth8 {
    using Layout = IndexLayout;
    using Pixel = uint8_t;
    using Plane = int16_t;  // an RGB plane's sample
    static constexpr int DEPTH = FELICS_DEPTH_8;
    static constexpr uintptr_t INDEX_ALIGN = 16;  // of every index address: the kernel loads a checkpoint as aligned words
    static constexpr size_t EXTRA = 0;            // bytes the form keeps on the device beside the status words
    static constexpr bool OWN_BEFORE_LDS = true;  // the opening's order: the call's own output checks, then the LDS bound
    static uint32_t lds_bytes(uint32_t W, uint32_t color) { return decode8_lds_bytes(W, color); }
    static bool lds_ok(uint32_t W, uint32_t color) { return index_lds_bytes(W, color) <= DECODE_LDS_LIMIT; }
    // an index header against its stream's header and length; the index fits the idx_len bytes it was given
    static bool index_ok(const uint8_t *ih, uint32_t color, uint32_t W, uint32_t H, uint64_t len, uint64_t idx_len, Layout &L) {
        return index_header_check(ih, color, W, H, len, L) == FELICS_OK && L.total <= idx_len;
    }
    int tables(felics_ctx *, size_t) { return FELICS_OK; }
    size_t launches_of(size_t) const { return 1; }
    int begin(felics_ctx *, hipStream_t, void *) { return FELICS_OK; }
    int end(felics_ctx *, hipStream_t) { return FELICS_OK; }
};

// 16-bit streams, version-2 indexes.  Every wave of a launch owns a dense estimator table in dec_table, so a launch holds at most
// `per` items (dec16_tables' bound, FELICS_TEST_INDEX16_PASS) and takes a fresh epoch: the items of a call or of an LDS class are cut
// into such passes wherever the cut falls -- inside a stream, a region or a plane: an item needs its own table and nothing of its
// neighbours'.  Behind the status words lies the rows-loaded counter.
struct Depth16 {
    using Layout = Index16Layout;
    using Pixel = uint16_t;
    using Plane = int32_t;
    static constexpr int DEPTH = FELICS_DEPTH_16;
    static constexpr uintptr_t INDEX_ALIGN = 64;  // the kernel loads a state row as one aligned 64-byte line
    static constexpr size_t EXTRA = 8;
    static constexpr bool OWN_BEFORE_LDS = false;  // the LDS bound first
    size_t per = 1;
    unsigned long long *d_loaded = nullptr, loaded = 0;
    static uint32_t lds_bytes(uint32_t W, uint32_t) { return decode16_lds_bytes(W); }
    static bool lds_ok(uint32_t W, uint32_t) { return decode16_lds_bytes(W) <= DECODE_LDS_LIMIT; }
    static bool index_ok(const uint8_t *ih, uint32_t color, uint32_t W, uint32_t H, uint64_t len, uint64_t idx_len, Layout &L) {
        return index16_header_check(ih, color, W, H, len, idx_len, L) == FELICS_OK;  // (total_bytes = idx_len is one of its checks)
    }
    int tables(felics_ctx *ctx, size_t most_items) { return dec16_tables(ctx, (size_t)index16_pass_cap(most_items), per); }  // most_items >= 1
    size_t table_bytes() const { return decode16_table_bytes((uint32_t)per); }
    size_t launches_of(size_t cnt) const { return (cnt + per - 1) / per; }
    int begin(felics_ctx *ctx, hipStream_t s, void *extra) {
        d_loaded = (unsigned long long *)extra;
        HIP_TRY(ctx, hipMemsetAsync(d_loaded, 0, 8, s));
        return FELICS_OK;
    }
    // launch(first item, items, tables, epoch) for every pass of n items, behind one another on the one stream: the passes share the tables
    template <typename Launch>
    int passes(felics_ctx *ctx, hipStream_t s, size_t n, Launch launch) {
        for (size_t o = 0; o < n; o += per) {
            uint32_t epoch = 0;
            const int rc = dec16_epoch(ctx, s, epoch);
            if (rc) return rc;
            HIP_TRY(ctx, launch(o, std::min(per, n - o), (uint32_t *)ctx->dec_table.p, epoch));
        }
        return FELICS_OK;
    }
    int end(felics_ctx *ctx, hipStream_t s) {
        HIP_TRY(ctx, hipMemcpyAsync(&loaded, d_loaded, 8, hipMemcpyDeviceToHost, s));
        return FELICS_OK;
    }
};

// What a same-shape call hands its launches: the streams of shape `hdr`, their indexes cut in segments of `seg` pixels, K to a plane.
struct SameShape {
    const uint8_t *streams;
    const uint64_t *d_off, *d_len;
    felics_header hdr;
    uint32_t seg, K;
    void *pixels, *planes;
    int *item_status, *status;  // a word per item; per stream or region
};

// The same-shape kinds at 8 bits: index i lies at index + i * stride.  The dense call's lane form is this form's own business:
// felics.h "Restart index: 64 segments per wave".
struct IndexSame8 : Depth8 {
    const uint8_t *index;
    uint64_t stride;
    static constexpr size_t ARRAYS = 2;  // u64 arrays of the call on the device: offsets | lens
    size_t n64 = 0;                      // dense: the first n64 streams take the lane form, in passes of pass_waves of their `waves` waves
    uint64_t waves = 0, pass_waves = 0;
    bool given() const { return index != nullptr; }
    bool aligned(size_t) const { return (((uintptr_t)index | stride) & (INDEX_ALIGN - 1u)) == 0; }
    const uint8_t *index0() const { return index; }
    uint64_t len0() const { return stride; }
    int upload(felics_ctx *, hipStream_t, uint64_t *, size_t) { return FELICS_OK; }
    static felics_region_stats &region_stats(felics_ctx *ctx) { return ctx->rstats; }

    // Which form (felics.h): the first n64 streams 64 segments to a wave, the others a wave per segment beside them; the lane form's
    // passes: whole waves, within the table memory index_lanes_tables grants
    int plan_dense(felics_ctx *ctx, size_t n, const felics_header &hdr, uint32_t K) {
        const uint32_t planes = hdr.color_type == FELICS_COLOR_RGB ? 3 : 1;
        if (hdr.width >= 8 && K >= 1 && n >= 64) {
            const uint64_t items = (uint64_t)(n / 64 * 64) * planes * K;
            const uint32_t least = felics_index_lanes_min_items(hdr.color_type);
            bool by_lane = least != INDEX8_LANES_NEVER && items >= least;
            if (const char *e = getenv("FELICS_TEST_INDEX_LANES")) by_lane = atoi(e) != 0;
            if (by_lane) n64 = n / 64 * 64;
        }
        waves = (uint64_t)(n64 / 64) * planes * K;
        if (waves) {
            const size_t wave_bytes = index8_lanes_table_bytes(64, hdr.color_type);
            size_t tbytes = 0;
            const int rc = index_lanes_tables(ctx, (size_t)std::min<uint64_t>(waves, index_lanes_pass_cap() / 64) * wave_bytes, wave_bytes, tbytes);
            if (rc) return rc;
            pass_waves = std::min<uint64_t>(waves, tbytes / wave_bytes);
        }
        ctx->istats.streams += n;
        ctx->istats.lane_segments8 += waves * 64;
        ctx->istats.segments8 += (n - n64) * planes * K;
        return FELICS_OK;
    }
    int dense(felics_ctx *ctx, hipStream_t s, const SameShape &d, size_t n) {
        const uint32_t W = d.hdr.width, H = d.hdr.height, color = d.hdr.color_type;
        const uint64_t npix = (uint64_t)W * H, per = (color ? 3u : 1u) * std::max(d.K, 1u), frame = npix * (color ? 3u : 1u);
        Pixel *pixels = (Pixel *)d.pixels;
        Plane *planes = (Plane *)d.planes;
        Lane &l = ctx->lanes[0];
        const bool beside = n64 && n64 < n;  // the wave form's streams run on the lane's front stream, between two events
        hipStream_t s2 = beside ? l.front : s;
        if (beside) {
            HIP_TRY(ctx, hipEventRecord(l.slice_done[0], s));
            HIP_TRY(ctx, hipStreamWaitEvent(s2, l.slice_done[0], 0));
        }
        // (the kernel is handed the pointers of stream n64 on and knows nothing of the streams in front)
        HIP_TRY(ctx, launch_decode8_seg(s2, d.streams, d.d_off + n64, d.d_len + n64, index + n64 * stride, stride, (uint32_t)(n - n64), W, H, color, d.seg,
                                        d.K, pixels + n64 * frame, planes ? planes + n64 * 3 * npix : nullptr, d.item_status + n64 * per, d.status + n64));
        for (uint64_t w0 = 0; w0 < waves; w0 += pass_waves) {  // behind one another: they share the tables
            HIP_TRY(ctx, launch_decode8_seg_lanes(s, d.streams, d.d_off, d.d_len, index, stride, W, H, color, d.seg, d.K, (uint32_t)w0,
                                                  (uint32_t)std::min(pass_waves, waves - w0), pixels, planes, (uint32_t *)ctx->dec_lane_table.p,
                                                  d.item_status));
            ctx->istats.lane_passes++;
        }
        HIP_TRY(ctx, launch_seg_finish(s, (uint32_t)n64, W, H, color, d.K, pixels, planes, d.item_status, d.status));
        if (beside) {
            HIP_TRY(ctx, hipEventRecord(l.spine_done[0], s2));
            HIP_TRY(ctx, hipStreamWaitEvent(s, l.spine_done[0], 0));
        }
        return FELICS_OK;
    }
    void done_dense(felics_ctx *) {}
    int regions(felics_ctx *ctx, hipStream_t s, const SameShape &d, const RegionRow *d_rows, const RegionItem *d_items, size_t n_items) {
        HIP_TRY(ctx, launch_decode8_regions(s, d.streams, d.d_off, d.d_len, index, stride, d.hdr.width, d.hdr.height, d.hdr.color_type, d.seg, d.K, d_rows,
                                            d_items, (uint32_t)n_items, (Pixel *)d.pixels, (Plane *)d.planes, d.item_status));
        return FELICS_OK;
    }
    void done_regions(felics_ctx *) {}
};

// The same-shape kinds at 16 bits: index i lies at index + offs[i] and is lens[i] bytes long; both arrays go to the device behind the
// streams'.
struct IndexSame16 : Depth16 {
    const uint8_t *index;
    const uint64_t *offs, *lens;
    static constexpr size_t ARRAYS = 4;  // offsets | lens | index offsets | index lens
    const uint64_t *d_ioff = nullptr, *d_ilen = nullptr;
    bool given() const { return index && offs && lens; }
    bool aligned(size_t n) const {  // every index address
        if ((uintptr_t)index & (INDEX_ALIGN - 1u)) return false;
        for (size_t i = 0; i < n; i++)
            if (offs[i] & (INDEX_ALIGN - 1u)) return false;
        return true;
    }
    const uint8_t *index0() const { return index + offs[0]; }
    uint64_t len0() const { return lens[0]; }
    int upload(felics_ctx *ctx, hipStream_t s, uint64_t *d_ix, size_t n) {
        HIP_TRY(ctx, hipMemcpyAsync(d_ix, offs, n * 8, hipMemcpyHostToDevice, s));
        HIP_TRY(ctx, hipMemcpyAsync(d_ix + n, lens, n * 8, hipMemcpyHostToDevice, s));
        d_ioff = d_ix, d_ilen = d_ix + n;
        return FELICS_OK;
    }
    static felics_region16_stats &region_stats(felics_ctx *ctx) { return ctx->r16stats; }

    int plan_dense(felics_ctx *ctx, size_t n, const felics_header &hdr, uint32_t K) {
        ctx->i16stats.streams += n;
        ctx->i16stats.segments16 += n * (hdr.color_type == FELICS_COLOR_RGB ? 3 : 1) * std::max(K, 1u);
        ctx->i16stats.table_bytes = table_bytes();
        return FELICS_OK;
    }
    int dense(felics_ctx *ctx, hipStream_t s, const SameShape &d, size_t n) {
        const uint32_t W = d.hdr.width, H = d.hdr.height, color = d.hdr.color_type;
        const int rc = passes(ctx, s, n * (color ? 3u : 1u) * std::max(d.K, 1u), [&](size_t o, size_t cnt, uint32_t *table, uint32_t epoch) {
            ctx->i16stats.passes++;
            return launch_decode16_seg(s, d.streams, d.d_off, d.d_len, index, d_ioff, d_ilen, W, H, color, d.seg, d.K, (uint32_t)o, (uint32_t)cnt,
                                       (Pixel *)d.pixels, (Plane *)d.planes, table, epoch, d.item_status, d_loaded);
        });
        if (rc) return rc;
        HIP_TRY(ctx, launch_seg_finish(s, (uint32_t)n, W, H, color, d.K, (Pixel *)d.pixels, (Plane *)d.planes, d.item_status, d.status));
        return FELICS_OK;
    }
    void done_dense(felics_ctx *ctx) { ctx->i16stats.rows_loaded += loaded; }
    int regions(felics_ctx *ctx, hipStream_t s, const SameShape &d, const RegionRow *d_rows, const RegionItem *d_items, size_t n_items) {
        return passes(ctx, s, n_items, [&](size_t o, size_t cnt, uint32_t *table, uint32_t epoch) {  // (a pass boundary may fall inside a region)
            ctx->r16stats.passes++;
            return launch_decode16_regions(s, d.streams, d.d_off, d.d_len, index, d_ioff, d_ilen, d.hdr.width, d.hdr.height, d.hdr.color_type, d.seg, d.K,
                                           d_rows, d_items, (uint32_t)o, (uint32_t)cnt, (uint8_t *)d.pixels, (Plane *)d.planes, table, epoch,
                                           d.item_status, d_loaded);
        });
    }
    void done_regions(felics_ctx *ctx) { ctx->r16stats.rows_loaded += loaded; }
};

// What every same-shape indexed call opens with: the shape every stream must have (header of stream 0: the form's depth, w * h < 2^32,
// a row the kernels' LDS holds -- there is no host fallback here), own(hdr) -- the checks of the call's own output --, then how every
// index is cut (header of index 0: L, seg), which must fit stream 0 and the bytes it was given.  (One index header; the streams' own
// headers are the kernels' to check.)  FELICS_OK, or the code the caller puts into every status and returns; FELICS_E_HIP leaves
// status alone.  The order of the codes is felics.h's, per depth: Form::OWN_BEFORE_LDS.
template <typename Form, typename Own>
int indexed_open(felics_ctx *ctx, const void *d_streams, const uint64_t *offsets, const uint64_t *lens, const Form &form, felics_header &hdr,
                 felics_header *hdr_out, typename Form::Layout &L, uint32_t &seg, Own own) {
    uint8_t h0[FELICS_HEADER_BYTES] = {0};
    const size_t hl = (size_t)std::min<uint64_t>(lens[0], FELICS_HEADER_BYTES);
    if (hl) HIP_TRY(ctx, hipMemcpy(h0, (const uint8_t *)d_streams + offsets[0], hl, hipMemcpyDeviceToHost));
    int rc = felics_read_header(h0, hl, &hdr);
    if (rc) return rc;  // stream 0 names the shape: without it nothing is decoded
    if (hdr_out) *hdr_out = hdr;
    if (hdr.pixel_depth != Form::DEPTH) return FELICS_E_UNSUPPORTED;  // the other depth has a format and calls of its own
    if ((uint64_t)hdr.width * hdr.height > 0xFFFFFFFFull) return FELICS_E_INVALID_DIMENSIONS;
    const int lds = Form::lds_ok(hdr.width, hdr.color_type) ? FELICS_OK : FELICS_E_UNSUPPORTED;
    if (!Form::OWN_BEFORE_LDS && lds) return lds;
    if ((rc = own(hdr)) != 0) return rc;
    if (lds) return lds;
    if (form.len0() < INDEX_HEADER_BYTES) return FELICS_E_INVALID_INDEX;
    uint8_t ih[INDEX_HEADER_BYTES];
    HIP_TRY(ctx, hipMemcpy(ih, form.index0(), INDEX_HEADER_BYTES, hipMemcpyDeviceToHost));
    if (!Form::index_ok(ih, hdr.color_type, hdr.width, hdr.height, lens[0], form.len0(), L)) return FELICS_E_INVALID_INDEX;
    seg = idx_rd32(ih + IDX_SEGPIX);
    return FELICS_OK;
}

// felics_decompress_batch_device_indexed and _indexed16 (felics.h "Restart index", "Restart index: 16-bit streams"): n streams of one
// shape, every (stream, plane, segment) an item with a status word of its own.  The alignment rule and a pending batch return without
// touching status.
template <typename Form>
int dense_indexed(felics_ctx *ctx, size_t n, const void *d_streams, const uint64_t *offsets, const uint64_t *lens, void *d_pixels, size_t d_pixels_cap,
                  felics_header *hdr_out, int *status, Form form) {
    using Pixel = typename Form::Pixel;
    using Plane = typename Form::Plane;
    if (!ctx || (n && (!d_streams || !offsets || !lens || !form.given() || !status))) return FELICS_E_INVALID_ARGUMENT;
    if (ctx->failed) return FELICS_E_HIP;
    if (n == 0) return FELICS_OK;
    if (any_pending(ctx)) return FELICS_E_INVALID_ARGUMENT;  // felics_wait_batch first
    if (!form.aligned(n)) return FELICS_E_INVALID_ARGUMENT;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    auto fail_all = [&](int code) { return fail_call(n, status, nullptr, nullptr, code); };
    // the opening checks; this call's own: the frames must fit
    felics_header hdr;
    typename Form::Layout L;
    uint32_t seg = 0;
    int rc = indexed_open(ctx, d_streams, offsets, lens, form, hdr, hdr_out, L, seg, [&](const felics_header &h) {
        const uint64_t bytes = (uint64_t)h.width * h.height * (h.color_type == FELICS_COLOR_RGB ? 3 : 1) * sizeof(Pixel);
        if (bytes * n > d_pixels_cap) return (int)FELICS_E_BUFFER_TOO_SMALL;
        return bytes && !d_pixels ? (int)FELICS_E_INVALID_ARGUMENT : (int)FELICS_OK;
    });
    if (rc) return rc == FELICS_E_HIP ? rc : fail_all(rc);
    const uint32_t planes = hdr.color_type == FELICS_COLOR_RGB ? 3 : 1;
    const uint64_t npix = (uint64_t)hdr.width * hdr.height;
    const uint64_t per = (uint64_t)planes * std::max(L.K, 1u);
    if (n > 0x7FFFFFFFull / per) return fail_all(FELICS_E_UNSUPPORTED);  // one block and one status word per segment, 32-bit item numbers
    const size_t items = (size_t)(n * per);
    if ((rc = form.tables(ctx, items)) != 0) return fail_all(rc);
    // the form's arrays | what it keeps | status on the device; a word per segment beside them
    if ((rc = reserve(ctx, ctx->dec_meta, n * 8 * Form::ARRAYS + Form::EXTRA + n * 4)) != 0) return fail_all(rc);
    if ((rc = reserve(ctx, ctx->dec_seg_status, items * 4)) != 0) return fail_all(rc);
    if (planes == 3 && (rc = reserve(ctx, ctx->dec_planes, (size_t)(npix * 3 * sizeof(Plane) * n) + 64)) != 0) return fail_all(rc);
    if ((rc = form.plan_dense(ctx, n, hdr, L.K)) != 0) return fail_all(rc);
    uint64_t *d_off = (uint64_t *)ctx->dec_meta.p, *d_len = d_off + n;
    uint8_t *extra = (uint8_t *)(d_off + n * Form::ARRAYS);
    int *d_status = (int *)(extra + Form::EXTRA);
    const SameShape d{(const uint8_t *)d_streams, d_off, d_len, hdr, seg, L.K, d_pixels, planes == 3 ? ctx->dec_planes.p : nullptr,
                      (int *)ctx->dec_seg_status.p, d_status};
    hipStream_t s = ctx->lanes[0].stream;
    for (size_t i = 0; i < n; i++) status[i] = FELICS_E_HIP;  // until the kernel's own word arrives
    HIP_TRY(ctx, hipMemcpyAsync(d_off, offsets, n * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(ctx, hipMemcpyAsync(d_len, lens, n * 8, hipMemcpyHostToDevice, s));
    if ((rc = form.upload(ctx, s, d_len + n, n)) != 0) return rc;
    if ((rc = form.begin(ctx, s, extra)) != 0) return rc;
    HIP_TRY(ctx, hipMemsetAsync(d_status, 0xFF, n * 4, s));
    HIP_TRY(ctx, hipMemsetAsync(d.item_status, 0xFF, items * 4, s));
    if ((rc = form.dense(ctx, s, d, n)) != 0) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(status, d_status, n * 4, hipMemcpyDeviceToHost, s));
    if ((rc = form.end(ctx, s)) != 0) return rc;
    HIP_TRY(ctx, hipStreamSynchronize(s));
    form.done_dense(ctx);
    return first_error(status, n);
}

// felics_decompress_regions_device_indexed and _indexed16 (felics.h "Restart index: regions", "... of 16-bit streams"): the plan
// (felics_index.h: region_plan) names the items, a wave each; crops are dense and back to back.
template <typename Form>
int regions_indexed(felics_ctx *ctx, size_t n_streams, const void *d_streams, const uint64_t *offsets, const uint64_t *lens, size_t n_regions,
                    const felics_region *regions, void *d_pixels, size_t d_pixels_cap, uint64_t *out_offsets, felics_header *hdr_out, int *status,
                    Form form) {
    using Pixel = typename Form::Pixel;
    using Plane = typename Form::Plane;
    if (!ctx || (n_streams && (!d_streams || !offsets || !lens || !form.given())) || (n_regions && (!regions || !status)))
        return FELICS_E_INVALID_ARGUMENT;
    if (ctx->failed) return FELICS_E_HIP;
    if (n_regions == 0) return FELICS_OK;
    auto fail_all = [&](int code) { return fail_call(n_regions, status, nullptr, nullptr, code); };
    if (any_pending(ctx)) return fail_all(FELICS_E_INVALID_ARGUMENT);  // felics_wait_batch first
    if (n_streams == 0 || n_streams > 0xFFFFFFFFull || n_regions > 0x7FFFFFFFull) return fail_all(FELICS_E_INVALID_ARGUMENT);
    if (!form.aligned(n_streams) || ((uintptr_t)d_pixels & (sizeof(Pixel) - 1u))) return fail_all(FELICS_E_INVALID_ARGUMENT);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    // the opening checks; this call's own: the requests inside the image, of a stream of the call; the crops, back to back, must fit
    felics_header hdr;
    typename Form::Layout L;
    uint32_t seg = 0;
    int rc = indexed_open(ctx, d_streams, offsets, lens, form, hdr, hdr_out, L, seg, [&](const felics_header &h) {
        for (size_t r = 0; r < n_regions; r++)
            if (regions[r].stream >= n_streams || !region_inside(h.width, h.height, regions[r])) return (int)FELICS_E_INVALID_ARGUMENT;
        const uint64_t pixel_bytes = (h.color_type == FELICS_COLOR_RGB ? 3 : 1) * sizeof(Pixel);
        uint64_t total = 0;
        for (size_t r = 0; r < n_regions; r++) {
            total += (uint64_t)regions[r].w * regions[r].h * pixel_bytes;  // (a crop has < 6 * 2^32 bytes: the sum is looked at before it can wrap)
            if (total > d_pixels_cap) return (int)FELICS_E_BUFFER_TOO_SMALL;
        }
        return total && !d_pixels ? (int)FELICS_E_INVALID_ARGUMENT : (int)FELICS_OK;
    });
    if (rc) return rc == FELICS_E_HIP ? rc : fail_all(rc);
    const uint32_t planes = hdr.color_type == FELICS_COLOR_RGB ? 3 : 1;
    RegionPlan P;
    if ((rc = region_plan(hdr.width, hdr.height, seg, planes, sizeof(Pixel), regions, n_regions, out_offsets, P)) != 0) return fail_all(rc);
    const size_t n_items = P.items.size();
    if ((rc = form.tables(ctx, n_items)) != 0) return fail_all(rc);
    // the form's arrays | what it keeps | status on the device; the region table and the work list; a word per item
    if ((rc = reserve(ctx, ctx->dec_meta, n_streams * 8 * Form::ARRAYS + Form::EXTRA + n_regions * 4)) != 0) return fail_all(rc);
    if ((rc = reserve(ctx, ctx->dec_region_work, n_regions * sizeof(RegionRow) + n_items * sizeof(RegionItem))) != 0) return fail_all(rc);
    if ((rc = reserve(ctx, ctx->dec_seg_status, n_items * 4)) != 0) return fail_all(rc);
    if (planes == 3 && (rc = reserve(ctx, ctx->dec_planes, (size_t)(P.plane_samples * sizeof(Plane)) + 64)) != 0) return fail_all(rc);  // crop-sized
    uint64_t *d_off = (uint64_t *)ctx->dec_meta.p, *d_len = d_off + n_streams;
    uint8_t *extra = (uint8_t *)(d_off + n_streams * Form::ARRAYS);
    int *d_status = (int *)(extra + Form::EXTRA);
    RegionRow *d_rows = (RegionRow *)ctx->dec_region_work.p;
    RegionItem *d_items = (RegionItem *)(d_rows + n_regions);
    const SameShape d{(const uint8_t *)d_streams, d_off, d_len, hdr, seg, L.K, d_pixels, planes == 3 ? ctx->dec_planes.p : nullptr,
                      (int *)ctx->dec_seg_status.p, d_status};
    auto &rs = Form::region_stats(ctx);
    rs.regions += n_regions;
    rs.segments_walked += P.walked;
    rs.segments_skipped += P.skipped;
    rs.pixels_walked += P.pixels_walked;
    hipStream_t s = ctx->lanes[0].stream;
    for (size_t i = 0; i < n_regions; i++) status[i] = FELICS_E_HIP;  // until the kernel's own word arrives
    HIP_TRY(ctx, hipMemcpyAsync(d_off, offsets, n_streams * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(ctx, hipMemcpyAsync(d_len, lens, n_streams * 8, hipMemcpyHostToDevice, s));
    if ((rc = form.upload(ctx, s, d_len + n_streams, n_streams)) != 0) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(d_rows, P.rows.data(), n_regions * sizeof(RegionRow), hipMemcpyHostToDevice, s));
    HIP_TRY(ctx, hipMemcpyAsync(d_items, P.items.data(), n_items * sizeof(RegionItem), hipMemcpyHostToDevice, s));
    if ((rc = form.begin(ctx, s, extra)) != 0) return rc;
    HIP_TRY(ctx, hipMemsetAsync(d_status, 0xFF, n_regions * 4, s));
    HIP_TRY(ctx, hipMemsetAsync(d.item_status, 0xFF, n_items * 4, s));
    if ((rc = form.regions(ctx, s, d, d_rows, d_items, n_items)) != 0) return rc;
    HIP_TRY(ctx, launch_regions_finish(s, d_rows, (uint32_t)n_regions, P.max_crop, (Pixel *)d_pixels, (Plane *)d.planes, d.item_status, d_status));
    HIP_TRY(ctx, hipMemcpyAsync(status, d_status, n_regions * 4, hipMemcpyDeviceToHost, s));
    if ((rc = form.end(ctx, s)) != 0) return rc;
    HIP_TRY(ctx, hipStreamSynchronize(s));  // (the plan lives until here)
    form.done_regions(ctx);
    return first_error(status, n_regions);
}

// The views kind: the streams have shapes of their own, so every index is addressed by its offset and length, at both depths.
// felics_decompress_views_device_indexed: k_decode8_seg_views; an index is exactly as long as its layout says.
struct IndexViews8 : Depth8 {
    using Stats = felics_index_view_stats;
    static Stats &stats(felics_ctx *ctx) { return ctx->ivstats; }
    static bool index_ok(const uint8_t *ih, uint32_t color, uint32_t W, uint32_t H, uint64_t len, uint64_t idx_len, Layout &L) {
        return Depth8::index_ok(ih, color, W, H, len, idx_len, L) && L.total == idx_len;
    }
    int launch(felics_ctx *ctx, hipStream_t s, const uint8_t *st, const uint64_t *d_off, const uint64_t *d_len, const uint8_t *ix, const uint64_t *,
               const IndexViewRow *d_rows, const IndexViewItem *d_items, size_t cnt, uint32_t lds, Plane *d_planes, int *d_item_status) {
        HIP_TRY(ctx, launch_decode8_seg_views(s, st, d_off, d_len, ix, d_rows, d_items, (uint32_t)cnt, lds, d_planes, d_item_status));
        return FELICS_OK;
    }
    void done(felics_ctx *) {}
};

// felics_decompress_views_device_indexed16: k_decode16_seg_views; a class's items in passes of the tables (Depth16).
struct IndexViews16 : Depth16 {
    using Stats = felics_index16_view_stats;
    static Stats &stats(felics_ctx *ctx) { return ctx->iv16stats; }
    int tables(felics_ctx *ctx, size_t most_items) {  // the largest class of a pass
        const int rc = Depth16::tables(ctx, most_items);
        if (!rc) stats(ctx).table_bytes = table_bytes();
        return rc;
    }
    int launch(felics_ctx *ctx, hipStream_t s, const uint8_t *st, const uint64_t *d_off, const uint64_t *d_len, const uint8_t *ix,
               const uint64_t *d_ilen, const IndexViewRow *d_rows, const IndexViewItem *d_items, size_t cnt, uint32_t lds, Plane *d_planes,
               int *d_item_status) {
        return passes(ctx, s, cnt, [&](size_t o, size_t c, uint32_t *table, uint32_t epoch) {
            return launch_decode16_seg_views(s, st, d_off, d_len, ix, d_ilen, d_rows, d_items + o, (uint32_t)c, lds, d_planes, table, epoch,
                                             d_item_status + o, d_loaded);
        });
    }
    void done(felics_ctx *ctx) { stats(ctx).rows_loaded += loaded; }
};

// felics_decompress_views_device_indexed and felics_decompress_views_device_indexed16 after the checks that need no device (felics.h
// "Restart index: views and mixed shapes", "Restart index: 16-bit streams into views and mixed shapes"), `form` being what they
// differ in:
//   1. the ready event in front of the lane's stream, on which everything below runs;
//   2. k_read_headers and k_read_index_headers, both records copied back, ONE synchronise;
//   3. every stream classified on the host, in the order felics.h lists the codes (the form's index header check with the stream's own
//      header and length; the index's exact size);
//   4. the streams in passes of consecutive streams whose RGB planes fit the scratch; within a pass the rows in LDS classes as
//      decompress_images cuts them for k_decode8, a class per launch (the 16-bit form: per launches of as many items as it has
//      tables), so a narrow stream does not pay a 4K row's LDS.  A row's items are contiguous in (plane, segment) order; rows, items
//      and the finish tables go up on the lane's stream;
//   5. per pass: the launches, k_seg_status over the pass's rows (a RegionRow per row names its items), the strided conversion of
//      its clean RGB rows -- behind one another on the one stream, since the passes share the planes (and the launches the tables);
//   6. one copy back of the rows' statuses (and of what the form counted).
template <typename Form>
int decompress_views_indexed(felics_ctx *ctx, size_t n, const void *d_streams, const uint64_t *offsets, const uint64_t *lens, const void *d_index,
                             const uint64_t *idx_offsets, const uint64_t *idx_lens, const felics_view *views, felics_header *hdrs, int *status,
                             Form form) {
    using Plane = typename Form::Plane;
    hipStream_t s = ctx->lanes[0].stream;
    typename Form::Stats &vs = Form::stats(ctx);
    vs.streams += n;
    vs.plane_bytes = 0;
    auto fail_all = [&](int code) {
        for (size_t i = 0; i < n; i++) status[i] = code;
        vs.undecoded += n;
        return code;
    };
    auto al = [](size_t b) { return (b + 15) & ~(size_t)15; };
    // offsets | lens | index offsets | index lens | stream headers | index headers in dec_meta
    const size_t o_rec = n * 32, o_ih = o_rec + al(n * sizeof(DecodeHeader)), o_meta_end = o_ih + n * INDEX_HEADER_BYTES;
    int rc = reserve(ctx, ctx->dec_meta, o_meta_end);
    if (rc) return fail_all(rc);
    // (one copy up -- the four arrays back to back -- and one copy back: the two kinds of headers as they lie in dec_meta)
    std::vector<uint64_t> up;
    std::vector<uint8_t> back;
    try {
        up.resize(4 * n);
        back.resize(o_meta_end - o_rec);
    } catch (const std::bad_alloc &) {
        return fail_all(FELICS_E_IO);
    }
    std::copy(offsets, offsets + n, up.begin());
    std::copy(lens, lens + n, up.begin() + n);
    std::copy(idx_offsets, idx_offsets + n, up.begin() + 2 * n);
    std::copy(idx_lens, idx_lens + n, up.begin() + 3 * n);
    const DecodeHeader *rec = reinterpret_cast<const DecodeHeader *>(back.data());
    const uint8_t *ih = back.data() + (o_ih - o_rec);
    uint8_t *meta = (uint8_t *)ctx->dec_meta.p;
    uint64_t *d_off = (uint64_t *)meta, *d_len = d_off + n, *d_ioff = d_len + n, *d_ilen = d_ioff + n;
    DecodeHeader *d_rec = (DecodeHeader *)(meta + o_rec);
    uint8_t *d_ih = meta + o_ih;
    const uint8_t *st = (const uint8_t *)d_streams, *ix = (const uint8_t *)d_index;
    auto headers = [&]() -> int {
        int r = wait_ready(ctx, s);  // (the header kernels read stream and index bytes)
        if (r) return r;
        HIP_TRY(ctx, hipMemcpyAsync(d_off, up.data(), n * 32, hipMemcpyHostToDevice, s));
        HIP_TRY(ctx, launch_read_headers(s, st, d_off, d_len, (uint32_t)n, d_rec));
        HIP_TRY(ctx, launch_read_index_headers(s, ix, d_ioff, d_ilen, (uint32_t)n, d_ih));
        HIP_TRY(ctx, hipMemcpyAsync(back.data(), d_rec, back.size(), hipMemcpyDeviceToHost, s));
        HIP_TRY(ctx, hipStreamSynchronize(s));
        return FELICS_OK;
    };
    if ((rc = headers()) != 0) return fail_all(rc);
    // the streams one by one: the first code of felics.h's list
    std::vector<typename Form::Layout> lay;
    std::vector<uint32_t> segpix;
    try {
        lay.resize(n);
        segpix.assign(n, 0);
    } catch (const std::bad_alloc &) {
        return fail_all(FELICS_E_IO);
    }
    uint64_t total_items = 0;
    size_t nrows = 0;
    for (size_t i = 0; i < n; i++) {
        const DecodeHeader &h = rec[i];
        const felics_view &w = views[i];
        if (hdrs) hdrs[i] = h.status == FELICS_OK ? felics_header{h.color, h.depth, h.W, h.H} : felics_header{};
        int code = h.dstatus;
        if (!code && h.depth != Form::DEPTH) code = FELICS_E_UNSUPPORTED;  // the other depth has a format and a call of its own
        if (!code && !Form::lds_ok(h.W, h.color)) code = FELICS_E_UNSUPPORTED;  // no host fallback here
        if (!code && ((int)h.color != w.color || (int)h.depth != w.depth || h.W != w.width || h.H != w.height)) code = FELICS_E_INVALID_DIMENSIONS;
        if (!code && (idx_lens[i] < INDEX_HEADER_BYTES || !Form::index_ok(ih + i * INDEX_HEADER_BYTES, h.color, h.W, h.H, lens[i], idx_lens[i], lay[i])))
            code = FELICS_E_INVALID_INDEX;
        status[i] = code;
        if (code) continue;
        segpix[i] = idx_rd32(ih + i * INDEX_HEADER_BYTES + IDX_SEGPIX);
        total_items += (uint64_t)lay[i].planes * std::max(lay[i].K, 1u);
        nrows++;
    }
    if (total_items > 0x7FFFFFFFull) return fail_all(FELICS_E_UNSUPPORTED);  // one block per item, a word per item
    // passes: consecutive streams whose planes (three Plane samples per RGB pixel) fit the budget; a single larger stream is a pass of its own
    auto plane_bytes_of = [&](size_t i) { return status[i] == FELICS_OK && rec[i].color ? 3ull * sizeof(Plane) * rec[i].W * rec[i].H : 0ull; };
    uint64_t plane_total = 0;
    for (size_t i = 0; i < n; i++) plane_total += plane_bytes_of(i);
    uint64_t budget = UINT64_MAX;
    size_t free_b = 0, total_b = 0;
    if (plane_total && plane_total + 64 > ctx->dec_planes.cap && hipMemGetInfo(&free_b, &total_b) == hipSuccess)
        budget = ((uint64_t)free_b + ctx->dec_planes.cap) / 4;
    budget = std::min(budget, index_views_pass_cap());
    std::vector<size_t> pass_end;
    std::vector<uint64_t> plane_off;
    uint64_t most = 0;
    // the tables: rows in (pass, LDS class, stream) order, a row's items contiguous
    constexpr uint32_t LDS_CLASS[] = {16u << 10, 32u << 10, 64u << 10, DECODE_LDS_LIMIT};
    struct Launch {
        size_t item0, cnt;
        uint32_t lds;
    };
    struct Pass {
        size_t row0, rows, launch0, launches;
        uint64_t max_npix;  // of its RGB rows
    };
    // rows | items | the finish tables (a RegionRow, a DecodeRow and a ViewRow per row), built where they are copied from in one piece
    const size_t n_items = (size_t)total_items;
    const size_t o_items = al(nrows * sizeof(IndexViewRow)), o_regions = o_items + al(n_items * sizeof(IndexViewItem)),
                 o_conv = o_regions + al(nrows * sizeof(RegionRow)), o_cviews = o_conv + al(nrows * sizeof(DecodeRow)),
                 o_end = o_cviews + nrows * sizeof(ViewRow);
    std::vector<uint8_t> tables;
    std::vector<int> row_status;
    std::vector<Launch> launches;
    std::vector<Pass> passes;
    IndexViewRow *rows = nullptr;
    size_t nr = 0, ni = 0;  // rows and items so far
    try {
        tables.assign(o_end, 0);
        row_status.assign(nrows, FELICS_E_HIP);  // until the kernels' own word arrives
        rows = reinterpret_cast<IndexViewRow *>(tables.data());
        IndexViewItem *items = reinterpret_cast<IndexViewItem *>(tables.data() + o_items);
        RegionRow *regions = reinterpret_cast<RegionRow *>(tables.data() + o_regions);
        DecodeRow *conv = reinterpret_cast<DecodeRow *>(tables.data() + o_conv);
        ViewRow *cviews = reinterpret_cast<ViewRow *>(tables.data() + o_cviews);
        plane_off.assign(n, 0);
        uint64_t acc = 0;
        for (size_t i = 0; i < n; i++) {
            const uint64_t b = plane_bytes_of(i);
            if (acc && acc + b > budget) {
                pass_end.push_back(i);
                acc = 0;
            }
            plane_off[i] = acc / sizeof(Plane);  // elements
            acc += b;
            most = std::max(most, acc);
        }
        pass_end.push_back(n);
        size_t i0 = 0;
        for (const size_t i1 : pass_end) {
            Pass P{nr, 0, launches.size(), 0, 0};
            for (int c = 0; c < 4; c++) {
                Launch L{ni, 0, 0};
                for (size_t i = i0; i < i1; i++) {
                    if (status[i] != FELICS_OK) continue;
                    const DecodeHeader &h = rec[i];
                    const uint32_t lds = Form::lds_bytes(h.W, h.color);
                    if (lds > LDS_CLASS[c] || (c > 0 && lds <= LDS_CLASS[c - 1])) continue;
                    const felics_view &w = views[i];
                    const uint32_t K = lay[i].K, keff = std::max(K, 1u), cnt = lay[i].planes * keff;
                    const uint32_t r = (uint32_t)nr++;
                    const ViewRow vr{w.data, w.row_stride, w.pixel_stride, h.color ? w.channel_stride : 0};
                    rows[r] = IndexViewRow{(uint32_t)i, h.W, h.H, h.color, segpix[i], K, (uint32_t)ni, cnt, idx_offsets[i], plane_off[i], vr};
                    regions[r] = RegionRow{(uint32_t)i, 0, 0, h.W, h.H, (uint32_t)ni, cnt, 0, 0, plane_off[i]};
                    conv[r] = DecodeRow{r - (uint32_t)P.row0, h.W, h.H, h.color, 0, plane_off[i]};  // (stream: the row within its pass, as status is)
                    cviews[r] = vr;
                    for (uint32_t p = 0; p < lay[i].planes; p++)
                        for (uint32_t j = 0; j < keff; j++) items[ni++] = IndexViewItem{r, p, j};
                    L.cnt += cnt;
                    L.lds = std::max(L.lds, lds);
                    if (h.color) P.max_npix = std::max(P.max_npix, (uint64_t)h.W * h.H);
                }
                if (L.cnt) launches.push_back(L);
            }
            P.rows = nr - P.row0;
            P.launches = launches.size() - P.launch0;
            passes.push_back(P);
            i0 = i1;
        }
    } catch (const std::bad_alloc &) {
        return fail_all(FELICS_E_IO);
    }
    // device side: the tables in dec_region_work; a word per item and one per row in dec_seg_status, what the form keeps behind them;
    // the form's own tables for the largest class of a pass
    const size_t o_extra = al(n_items * 4) + al(nrows * 4);
    size_t most_items = 0, n_launches = 0;
    for (const Launch &L : launches) most_items = std::max(most_items, L.cnt);
    if (nrows && (rc = reserve(ctx, ctx->dec_region_work, o_end)) != 0) return fail_all(rc);
    if (nrows && (rc = reserve(ctx, ctx->dec_seg_status, o_extra + Form::EXTRA)) != 0) return fail_all(rc);
    if (most && (rc = reserve(ctx, ctx->dec_planes, (size_t)most + 64)) != 0) return fail_all(rc);
    if (nrows && (rc = form.tables(ctx, most_items)) != 0) return fail_all(rc);
    for (const Launch &L : launches) n_launches += form.launches_of(L.cnt);
    for (size_t i = 0; i < n; i++) vs.undecoded += status[i] != FELICS_OK;
    vs.items += n_items;
    vs.launches += n_launches;
    vs.passes += passes.size();
    vs.plane_bytes = most;
    if (nrows) {
        uint8_t *work = (uint8_t *)ctx->dec_region_work.p;
        IndexViewRow *d_rows = (IndexViewRow *)work;
        IndexViewItem *d_items = (IndexViewItem *)(work + o_items);
        RegionRow *d_regions = (RegionRow *)(work + o_regions);
        DecodeRow *d_conv = (DecodeRow *)(work + o_conv);
        ViewRow *d_cviews = (ViewRow *)(work + o_cviews);
        int *d_item_status = (int *)ctx->dec_seg_status.p, *d_row_status = (int *)((uint8_t *)ctx->dec_seg_status.p + al(n_items * 4));
        Plane *d_planes = (Plane *)ctx->dec_planes.p;
        auto queue = [&]() -> int {
            int r;
            HIP_TRY(ctx, hipMemcpyAsync(work, tables.data(), o_end, hipMemcpyHostToDevice, s));  // (the five tables in one copy)
            HIP_TRY(ctx, hipMemsetAsync(d_item_status, 0xFF, al(n_items * 4) + nrows * 4, s));
            if ((r = form.begin(ctx, s, (uint8_t *)ctx->dec_seg_status.p + o_extra)) != 0) return r;
            for (const Pass &P : passes) {
                for (size_t k = P.launch0; k < P.launch0 + P.launches; k++) {
                    const Launch &L = launches[k];
                    if ((r = form.launch(ctx, s, st, d_off, d_len, ix, d_ilen, d_rows, d_items + L.item0, L.cnt, L.lds, d_planes,
                                         d_item_status + L.item0)) != 0)
                        return r;
                }
                HIP_TRY(ctx, (launch_seg_views_finish<Plane, typename Form::Pixel>(s, (uint32_t)P.rows, d_regions + P.row0, d_item_status, d_conv + P.row0,
                                                                                   d_cviews + P.row0, P.max_npix, d_planes, d_row_status + P.row0)));
            }
            HIP_TRY(ctx, hipMemcpyAsync(row_status.data(), d_row_status, nrows * 4, hipMemcpyDeviceToHost, s));
            if ((r = form.end(ctx, s)) != 0) return r;
            HIP_TRY(ctx, hipStreamSynchronize(s));  // (the host tables live until here)
            form.done(ctx);
            return FELICS_OK;
        };
        if ((rc = queue()) != 0) {
            for (size_t r = 0; r < nrows; r++) status[rows[r].stream] = FELICS_E_HIP;
            return rc;
        }
        for (size_t r = 0; r < nrows; r++) status[rows[r].stream] = row_status[r];
    }
    return first_error(status, n);
}

// The two calls' entry: the checks that need no device, made before anything is launched, then decompress_views_indexed between the
// setting and the clearing of the ready event.
template <typename Form>
int views_indexed_call(felics_ctx *ctx, size_t n, const void *d_streams, const uint64_t *offsets, const uint64_t *lens, const void *d_index,
                       const uint64_t *idx_offsets, const uint64_t *idx_lens, const felics_view *views, void *ready_event, felics_header *hdrs,
                       int *status, Form form) {
    if (!ctx || (n && !status)) return FELICS_E_INVALID_ARGUMENT;
    auto fail_all = [&](int code) { return fail_call(n, status, hdrs, nullptr, code); };
    if (n && (!d_streams || !offsets || !lens || !d_index || !idx_offsets || !idx_lens || !views)) return fail_all(FELICS_E_INVALID_ARGUMENT);
    for (size_t i = 0; i < n; i++) {  // every view and every index address before anything is launched: the first error in view order
        const int rc = felics_view_writable(&views[i]);
        if (rc) return fail_all(rc);
        if (((uintptr_t)d_index + idx_offsets[i]) & (Form::INDEX_ALIGN - 1u)) return fail_all(FELICS_E_INVALID_ARGUMENT);
    }
    if (ctx->failed) return fail_all(FELICS_E_HIP);
    if (n == 0) return FELICS_OK;
    if (any_pending(ctx)) return fail_all(FELICS_E_INVALID_ARGUMENT);  // felics_wait_batch first
    if (n > 0xFFFFFFFFull) return fail_all(FELICS_E_INVALID_ARGUMENT);
    if (hipSetDevice(ctx->device) != hipSuccess) return fail_all(hip_fail(ctx, hipGetLastError(), "hipSetDevice"));
    ctx->view_ready = (hipEvent_t)ready_event;
    const int rc = decompress_views_indexed(ctx, n, d_streams, offsets, lens, d_index, idx_offsets, idx_lens, views, hdrs, status, form);
    ctx->view_ready = nullptr;
    return rc;
}

// The region views kind (felics.h "Restart index: regions into views and mixed shapes"): the views kind's streams and indexes, a plan
// per region from its own stream's geometry.  felics_decompress_region_views_device_indexed: k_decode8_region_views.
struct RegionViews8 : Depth8 {
    using Stats = felics_region_view_stats;
    static Stats &stats(felics_ctx *ctx) { return ctx->rvstats; }
    static bool index_ok(const uint8_t *ih, uint32_t color, uint32_t W, uint32_t H, uint64_t len, uint64_t idx_len, Layout &L) {
        return IndexViews8::index_ok(ih, color, W, H, len, idx_len, L);
    }
    int launch(felics_ctx *ctx, hipStream_t s, const uint8_t *st, const uint64_t *d_off, const uint64_t *d_len, const uint8_t *ix, const uint64_t *,
               const RegionViewStream *d_srows, const RegionRow *d_regions, const ViewRow *d_views, const RegionItem *d_items, size_t cnt,
               uint32_t lds, Plane *d_planes, int *d_item_status) {
        HIP_TRY(ctx, launch_decode8_region_views(s, st, d_off, d_len, ix, d_srows, d_regions, d_views, d_items, (uint32_t)cnt, lds, d_planes,
                                                 d_item_status));
        return FELICS_OK;
    }
    void done(felics_ctx *) {}
};

// felics_decompress_region_views_device_indexed16: k_decode16_region_views; a class's items in passes of the tables (Depth16).
struct RegionViews16 : Depth16 {
    using Stats = felics_region16_view_stats;
    static Stats &stats(felics_ctx *ctx) { return ctx->rv16stats; }
    int tables(felics_ctx *ctx, size_t most_items) {  // the largest class of a pass
        const int rc = Depth16::tables(ctx, most_items);
        if (!rc) stats(ctx).table_bytes = table_bytes();
        return rc;
    }
    int launch(felics_ctx *ctx, hipStream_t s, const uint8_t *st, const uint64_t *d_off, const uint64_t *d_len, const uint8_t *ix,
               const uint64_t *d_ilen, const RegionViewStream *d_srows, const RegionRow *d_regions, const ViewRow *d_views,
               const RegionItem *d_items, size_t cnt, uint32_t lds, Plane *d_planes, int *d_item_status) {
        return passes(ctx, s, cnt, [&](size_t o, size_t c, uint32_t *table, uint32_t epoch) {  // (a table cut may fall inside a region or a plane)
            return launch_decode16_region_views(s, st, d_off, d_len, ix, d_ilen, d_srows, d_regions, d_views, d_items + o, (uint32_t)c, lds, d_planes,
                                                table, epoch, d_item_status + o, d_loaded);
        });
    }
    void done(felics_ctx *ctx) { stats(ctx).rows_loaded += loaded; }
};

// felics_decompress_region_views_device_indexed and its 16-bit form after the checks that need no device, `form` being what they
// differ in.  Steps 1 - 3 are decompress_views_indexed's (the event, the two header kernels and ONE synchronise, every stream
// classified on the host -- without the comparison with a view, which is per region here); then
//   4. every region classified: its stream's code, the window inside the stream's image, the view's colour and depth;
//   5. the plan: the clean, non-empty regions in passes of consecutive regions whose crop-sized RGB planes fit the scratch, within a
//      pass in the LDS classes of their streams' rows, a row per region with the items region_plan_add names for the stream's own W,
//      H, segment_pixels and planes (an empty region has no row: its code is final here);
//   6. per pass: a launch per class (the 16-bit form: cut by its tables), k_seg_status over the pass's rows, the strided conversion
//      of its clean RGB rows (a DecodeRow of W = w, H = h per row), behind one another on the one stream;
//   7. one copy back of the rows' statuses (and of what the form counted).
template <typename Form>
int region_views_indexed(felics_ctx *ctx, size_t n, const void *d_streams, const uint64_t *offsets, const uint64_t *lens, const void *d_index,
                         const uint64_t *idx_offsets, const uint64_t *idx_lens, size_t n_regions, const felics_region *regions,
                         const felics_view *views, felics_header *hdrs, int *status, Form form) {
    using Plane = typename Form::Plane;
    using Pixel = typename Form::Pixel;
    hipStream_t s = ctx->lanes[0].stream;
    typename Form::Stats &vs = Form::stats(ctx);
    vs.regions += n_regions;
    vs.plane_bytes = 0;
    bool headers_read = false;
    auto fail_all = [&](int code) {
        for (size_t r = 0; r < n_regions; r++) status[r] = code;
        for (size_t i = 0; hdrs && !headers_read && i < n; i++) hdrs[i] = felics_header{};  // (no stale header beside a failure code)
        vs.undecoded += n_regions;
        return code;
    };
    auto al = [](size_t b) { return (b + 15) & ~(size_t)15; };
    // offsets | lens | index offsets | index lens | stream headers | index headers in dec_meta
    const size_t o_rec = n * 32, o_ih = o_rec + al(n * sizeof(DecodeHeader)), o_meta_end = o_ih + n * INDEX_HEADER_BYTES;
    int rc = reserve(ctx, ctx->dec_meta, o_meta_end);
    if (rc) return fail_all(rc);
    std::vector<uint64_t> up;
    std::vector<uint8_t> back;
    std::vector<typename Form::Layout> lay;
    std::vector<RegionViewStream> srows;
    std::vector<int> scode;
    try {
        up.resize(4 * n);
        back.resize(o_meta_end - o_rec);
        lay.resize(n);
        srows.assign(n, RegionViewStream{});
        scode.assign(n, FELICS_OK);
    } catch (const std::bad_alloc &) {
        return fail_all(FELICS_E_IO);
    }
    std::copy(offsets, offsets + n, up.begin());
    std::copy(lens, lens + n, up.begin() + n);
    std::copy(idx_offsets, idx_offsets + n, up.begin() + 2 * n);
    std::copy(idx_lens, idx_lens + n, up.begin() + 3 * n);
    const DecodeHeader *rec = reinterpret_cast<const DecodeHeader *>(back.data());
    const uint8_t *ih = back.data() + (o_ih - o_rec);
    uint8_t *meta = (uint8_t *)ctx->dec_meta.p;
    uint64_t *d_off = (uint64_t *)meta, *d_len = d_off + n, *d_ioff = d_len + n, *d_ilen = d_ioff + n;
    DecodeHeader *d_rec = (DecodeHeader *)(meta + o_rec);
    uint8_t *d_ih = meta + o_ih;
    const uint8_t *st = (const uint8_t *)d_streams, *ix = (const uint8_t *)d_index;
    auto headers = [&]() -> int {
        int r = wait_ready(ctx, s);  // (the header kernels read stream and index bytes)
        if (r) return r;
        HIP_TRY(ctx, hipMemcpyAsync(d_off, up.data(), n * 32, hipMemcpyHostToDevice, s));
        HIP_TRY(ctx, launch_read_headers(s, st, d_off, d_len, (uint32_t)n, d_rec));
        HIP_TRY(ctx, launch_read_index_headers(s, ix, d_ioff, d_ilen, (uint32_t)n, d_ih));
        HIP_TRY(ctx, hipMemcpyAsync(back.data(), d_rec, back.size(), hipMemcpyDeviceToHost, s));
        HIP_TRY(ctx, hipStreamSynchronize(s));
        return FELICS_OK;
    };
    if ((rc = headers()) != 0) return fail_all(rc);
    headers_read = true;  // (hdrs[] is filled below, whatever happens after it)
    // the streams one by one: the first code of the views call's list, the comparison with a view left out
    for (size_t i = 0; i < n; i++) {
        const DecodeHeader &h = rec[i];
        if (hdrs) hdrs[i] = h.status == FELICS_OK ? felics_header{h.color, h.depth, h.W, h.H} : felics_header{};
        int code = h.dstatus;
        if (!code && h.depth != Form::DEPTH) code = FELICS_E_UNSUPPORTED;  // the other depth has a format and a call of its own
        if (!code && !Form::lds_ok(h.W, h.color)) code = FELICS_E_UNSUPPORTED;  // no host fallback here
        if (!code && (idx_lens[i] < INDEX_HEADER_BYTES || !Form::index_ok(ih + i * INDEX_HEADER_BYTES, h.color, h.W, h.H, lens[i], idx_lens[i], lay[i])))
            code = FELICS_E_INVALID_INDEX;
        scode[i] = code;
        if (!code) srows[i] = RegionViewStream{h.W, h.H, h.color, idx_rd32(ih + i * INDEX_HEADER_BYTES + IDX_SEGPIX), lay[i].K, 0, idx_offsets[i]};
    }
    // the regions one by one; `walks`: a clean region with pixels to decode
    auto walks = [&](size_t r) { return status[r] == FELICS_OK && !region_empty(regions[r]); };
    for (size_t r = 0; r < n_regions; r++) {
        const felics_region &g = regions[r];
        const DecodeHeader &h = rec[g.stream];
        int code = scode[g.stream];
        if (!code && !region_inside(h.W, h.H, g)) code = FELICS_E_INVALID_ARGUMENT;
        if (!code && ((int)h.color != views[r].color || (int)h.depth != views[r].depth)) code = FELICS_E_INVALID_DIMENSIONS;
        status[r] = code;
    }
    // passes: consecutive regions whose crop-sized planes (three Plane samples per RGB crop pixel) fit the budget; a single larger
    // region is a pass of its own
    auto plane_bytes_of = [&](size_t r) {
        return walks(r) && rec[regions[r].stream].color ? 3ull * sizeof(Plane) * regions[r].w * regions[r].h : 0ull;
    };
    uint64_t plane_total = 0;
    for (size_t r = 0; r < n_regions; r++) plane_total += plane_bytes_of(r);
    uint64_t budget = UINT64_MAX;
    size_t free_b = 0, total_b = 0;
    if (plane_total && plane_total + 64 > ctx->dec_planes.cap && hipMemGetInfo(&free_b, &total_b) == hipSuccess)
        budget = ((uint64_t)free_b + ctx->dec_planes.cap) / 4;
    budget = std::min(budget, index_views_pass_cap());
    constexpr uint32_t LDS_CLASS[] = {16u << 10, 32u << 10, 64u << 10, DECODE_LDS_LIMIT};
    struct Launch {
        size_t item0, cnt;
        uint32_t lds;
    };
    struct Pass {
        size_t row0, rows, launch0, launches;
        uint64_t max_npix;  // of its RGB rows' crops
    };
    RegionPlan P;  // rows in (pass, LDS class, region) order, a row's items contiguous; plane_off within the pass
    std::vector<uint32_t> row_region, segs;
    std::vector<ViewRow> cviews;
    std::vector<DecodeRow> conv;
    std::vector<Launch> launches;
    std::vector<Pass> passes;
    std::vector<int> row_status;
    std::vector<uint8_t> tables;
    uint64_t most = 0, skipped = 0;
    size_t o_regions = 0, o_views = 0, o_items = 0, o_conv = 0, o_end = 0;
    try {
        size_t r0 = 0;
        while (r0 < n_regions) {
            size_t r1 = r0;
            uint64_t acc = 0;
            for (; r1 < n_regions; r1++) {
                const uint64_t b = plane_bytes_of(r1);
                if (acc && acc + b > budget) break;
                acc += b;
            }
            most = std::max(most, acc);
            Pass pass{P.rows.size(), 0, launches.size(), 0, 0};
            P.plane_samples = 0;
            P.max_crop = 0;
            for (int c = 0; c < 4; c++) {
                Launch L{P.items.size(), 0, 0};
                for (size_t r = r0; r < r1; r++) {
                    if (!walks(r)) continue;
                    const felics_region &g = regions[r];
                    const RegionViewStream &sr = srows[g.stream];
                    const uint32_t lds = Form::lds_bytes(sr.W, sr.color);
                    if (lds > LDS_CLASS[c] || (c > 0 && lds <= LDS_CLASS[c - 1])) continue;
                    const felics_view &w = views[r];
                    const uint32_t planes = sr.color ? 3u : 1u, row = (uint32_t)P.rows.size();
                    const uint64_t walked0 = P.walked;
                    uint64_t out_at = 0;
                    if ((rc = region_plan_add(sr.W, sr.H, sr.segment_pixels, planes, sizeof(Pixel), g, row, false, out_at, segs, P)) != 0)
                        return fail_all(rc);  // 2^31 work items or more
                    skipped += (uint64_t)planes * sr.K - (P.walked - walked0);
                    row_region.push_back((uint32_t)r);
                    cviews.push_back(ViewRow{w.data, w.row_stride, w.pixel_stride, sr.color ? w.channel_stride : 0});
                    conv.push_back(DecodeRow{row - (uint32_t)pass.row0, g.w, g.h, sr.color, 0, P.rows[row].plane_off});  // (stream: the row within its pass)
                    L.cnt += P.rows[row].nitems;
                    L.lds = std::max(L.lds, lds);
                }
                if (L.cnt) launches.push_back(L);
            }
            pass.rows = P.rows.size() - pass.row0;
            pass.launches = launches.size() - pass.launch0;
            pass.max_npix = P.max_crop;
            if (pass.rows) passes.push_back(pass);
            r0 = r1;
        }
        // stream rows | region rows | their views | items | the conversion rows, copied up in one piece
        const size_t nrows = P.rows.size(), n_items = P.items.size();
        o_regions = al(n * sizeof(RegionViewStream));
        o_views = o_regions + al(nrows * sizeof(RegionRow));
        o_items = o_views + al(nrows * sizeof(ViewRow));
        o_conv = o_items + al(n_items * sizeof(RegionItem));
        o_end = o_conv + nrows * sizeof(DecodeRow);
        if (nrows) {
            tables.assign(o_end, 0);
            memcpy(tables.data(), srows.data(), n * sizeof(RegionViewStream));
            memcpy(tables.data() + o_regions, P.rows.data(), nrows * sizeof(RegionRow));
            memcpy(tables.data() + o_views, cviews.data(), nrows * sizeof(ViewRow));
            memcpy(tables.data() + o_items, P.items.data(), n_items * sizeof(RegionItem));
            memcpy(tables.data() + o_conv, conv.data(), nrows * sizeof(DecodeRow));
            row_status.assign(nrows, FELICS_E_HIP);  // until the kernels' own word arrives
        }
    } catch (const std::bad_alloc &) {
        return fail_all(FELICS_E_IO);
    }
    const size_t nrows = P.rows.size(), n_items = P.items.size();
    // device side: the tables in dec_region_work; a word per item and one per row in dec_seg_status, what the form keeps behind them;
    // the form's own tables for the largest class of a pass
    const size_t o_extra = al(n_items * 4) + al(nrows * 4);
    size_t most_items = 0, n_launches = 0;
    for (const Launch &L : launches) most_items = std::max(most_items, L.cnt);
    if (nrows && (rc = reserve(ctx, ctx->dec_region_work, o_end)) != 0) return fail_all(rc);
    if (nrows && (rc = reserve(ctx, ctx->dec_seg_status, o_extra + Form::EXTRA)) != 0) return fail_all(rc);
    if (most && (rc = reserve(ctx, ctx->dec_planes, (size_t)most + 64)) != 0) return fail_all(rc);
    if (nrows && (rc = form.tables(ctx, most_items)) != 0) return fail_all(rc);
    for (const Launch &L : launches) n_launches += form.launches_of(L.cnt);
    for (size_t r = 0; r < n_regions; r++) vs.undecoded += status[r] != FELICS_OK;
    for (size_t r = 0; r < n_regions; r++)  // (an empty region skips every segment of its stream)
        if (status[r] == FELICS_OK && region_empty(regions[r])) skipped += (uint64_t)(srows[regions[r].stream].color ? 3u : 1u) * srows[regions[r].stream].K;
    vs.segments_walked += P.walked;
    vs.segments_skipped += skipped;
    vs.pixels_walked += P.pixels_walked;
    vs.launches += n_launches;
    vs.passes += passes.size();
    vs.plane_bytes = most;
    if (nrows) {
        uint8_t *work = (uint8_t *)ctx->dec_region_work.p;
        const RegionViewStream *d_srows = (const RegionViewStream *)work;
        const RegionRow *d_regions = (const RegionRow *)(work + o_regions);
        const ViewRow *d_cviews = (const ViewRow *)(work + o_views);
        const RegionItem *d_items = (const RegionItem *)(work + o_items);
        const DecodeRow *d_conv = (const DecodeRow *)(work + o_conv);
        int *d_item_status = (int *)ctx->dec_seg_status.p, *d_row_status = (int *)((uint8_t *)ctx->dec_seg_status.p + al(n_items * 4));
        Plane *d_planes = (Plane *)ctx->dec_planes.p;
        auto queue = [&]() -> int {
            int r;
            HIP_TRY(ctx, hipMemcpyAsync(work, tables.data(), o_end, hipMemcpyHostToDevice, s));  // (the five tables in one copy)
            HIP_TRY(ctx, hipMemsetAsync(d_item_status, 0xFF, al(n_items * 4) + nrows * 4, s));
            if ((r = form.begin(ctx, s, (uint8_t *)ctx->dec_seg_status.p + o_extra)) != 0) return r;
            for (const Pass &pass : passes) {
                for (size_t k = pass.launch0; k < pass.launch0 + pass.launches; k++) {
                    const Launch &L = launches[k];
                    if ((r = form.launch(ctx, s, st, d_off, d_len, ix, d_ilen, d_srows, d_regions, d_cviews, d_items + L.item0, L.cnt, L.lds, d_planes,
                                         d_item_status + L.item0)) != 0)
                        return r;
                }
                HIP_TRY(ctx, (launch_seg_views_finish<Plane, Pixel>(s, (uint32_t)pass.rows, d_regions + pass.row0, d_item_status, d_conv + pass.row0,
                                                                    d_cviews + pass.row0, pass.max_npix, d_planes, d_row_status + pass.row0)));
            }
            HIP_TRY(ctx, hipMemcpyAsync(row_status.data(), d_row_status, nrows * 4, hipMemcpyDeviceToHost, s));
            if ((r = form.end(ctx, s)) != 0) return r;
            HIP_TRY(ctx, hipStreamSynchronize(s));  // (the host tables live until here)
            form.done(ctx);
            return FELICS_OK;
        };
        if ((rc = queue()) != 0) {
            for (size_t r = 0; r < nrows; r++) status[row_region[r]] = FELICS_E_HIP;
            return rc;
        }
        for (size_t r = 0; r < nrows; r++) status[row_region[r]] = row_status[r];
    }
    return first_error(status, n_regions);
}

// The two calls' entry: the checks that need no device, made before anything is launched, then region_views_indexed between the
// setting and the clearing of the ready event.
template <typename Form>
int region_views_call(felics_ctx *ctx, size_t n_streams, const void *d_streams, const uint64_t *offsets, const uint64_t *lens, const void *d_index,
                      const uint64_t *idx_offsets, const uint64_t *idx_lens, size_t n_regions, const felics_region *regions, const felics_view *views,
                      void *ready_event, felics_header *hdrs, int *status, Form form) {
    if (!ctx || (n_regions && !status)) return FELICS_E_INVALID_ARGUMENT;
    auto fail_all = [&](int code) {
        for (size_t i = 0; hdrs && i < n_streams; i++) hdrs[i] = felics_header{};
        return fail_call(n_regions, status, nullptr, nullptr, code);
    };
    if ((n_streams && (!d_streams || !offsets || !lens || !d_index || !idx_offsets || !idx_lens)) || (n_regions && (!regions || !views)))
        return fail_all(FELICS_E_INVALID_ARGUMENT);
    if (n_regions > 0x7FFFFFFFull || n_streams > 0xFFFFFFFFull || (n_regions && n_streams == 0)) return fail_all(FELICS_E_INVALID_ARGUMENT);
    for (size_t r = 0; r < n_regions; r++) {  // every region and its view before anything is launched: the first error in region order
        if (regions[r].stream >= n_streams) return fail_all(FELICS_E_INVALID_ARGUMENT);
        const int rc = felics_view_writable(&views[r]);
        if (rc) return fail_all(rc);
        if (views[r].width != regions[r].w || views[r].height != regions[r].h) return fail_all(FELICS_E_INVALID_ARGUMENT);
    }
    for (size_t i = 0; i < n_streams; i++)  // every index address
        if (((uintptr_t)d_index + idx_offsets[i]) & (Form::INDEX_ALIGN - 1u)) return fail_all(FELICS_E_INVALID_ARGUMENT);
    if (ctx->failed) return fail_all(FELICS_E_HIP);
    if (n_regions == 0) return FELICS_OK;
    if (any_pending(ctx)) return fail_all(FELICS_E_INVALID_ARGUMENT);  // felics_wait_batch first
    if (hipSetDevice(ctx->device) != hipSuccess) return fail_all(hip_fail(ctx, hipGetLastError(), "hipSetDevice"));
    ctx->view_ready = (hipEvent_t)ready_event;
    const int rc = region_views_indexed(ctx, n_streams, d_streams, offsets, lens, d_index, idx_offsets, idx_lens, n_regions, regions, views, hdrs,
                                        status, form);
    ctx->view_ready = nullptr;
    return rc;
}

}  // namespace

}  // namespace felics

extern "C" {

int felics_get_decode_stats(const felics_ctx *ctx, felics_decode_stats *out, size_t out_size) {
    return copy_stats(ctx, &felics_ctx::dstats, out, out_size);
}

int felics_get_decode_view_stats(const felics_ctx *ctx, felics_decode_view_stats *out, size_t out_size) {
    return copy_stats(ctx, &felics_ctx::dvstats, out, out_size);
}

int felics_view_writable(const felics_view *v) {
    return v ? view_writable_code(*v) : FELICS_E_INVALID_ARGUMENT;  // (felics_viewcheck.h: check_view's checks and the nested rule)
}

uint32_t felics_decode_lanes_min_streams(int depth, int color) {
    if (depth) return color ? DECODE16_LANES_MIN_STREAMS_RGB : DECODE16_LANES_MIN_STREAMS;
    return color ? DECODE8_LANES_MIN_STREAMS_RGB : DECODE8_LANES_MIN_STREAMS;
}

int felics_decompress_batch_device(felics_ctx *ctx, size_t n, const void *d_streams, const uint64_t *offsets,
                                   const uint64_t *lens, void *d_pixels, size_t d_pixels_cap, felics_header *hdr_out,
                                   int *status) {
    if (!ctx || (n && (!d_streams || !offsets || !lens || !status))) return FELICS_E_INVALID_ARGUMENT;
    if (ctx->failed) return FELICS_E_HIP;
    if (n == 0) return FELICS_OK;
    if (any_pending(ctx)) return FELICS_E_INVALID_ARGUMENT;  // felics_wait_batch first
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    Lane &l = ctx->lanes[0];
    // the shape every stream must have: header of stream 0
    uint8_t h0[FELICS_HEADER_BYTES] = {0};
    const size_t hl = (size_t)std::min<uint64_t>(lens[0], FELICS_HEADER_BYTES);
    if (hl) HIP_TRY(ctx, hipMemcpy(h0, (const uint8_t *)d_streams + offsets[0], hl, hipMemcpyDeviceToHost));
    felics_decode_stats &ds = ctx->dstats;
    ds.streams += n;
    ds.lanes16_table_bytes = 0;
    auto fail_all = [&](int code) { return fail_decode(ctx, n, status, code); };
    felics_header hdr;
    int rc = felics_read_header(h0, hl, &hdr);
    if (rc) return fail_all(rc);  // stream 0 names the shape: without it nothing is decoded
    if (hdr_out) *hdr_out = hdr;
    const uint32_t planes = hdr.color_type == FELICS_COLOR_RGB ? 3 : 1;
    const size_t bps = hdr.pixel_depth == FELICS_DEPTH_16 ? 2 : 1;
    const uint64_t npix = (uint64_t)hdr.width * hdr.height;
    if (npix > 0xFFFFFFFFull) return fail_all(FELICS_E_INVALID_DIMENSIONS);
    const uint64_t frame_bytes = npix * planes * bps;
    if (frame_bytes * n > d_pixels_cap) return fail_all(FELICS_E_BUFFER_TOO_SMALL);
    if (frame_bytes && !d_pixels) return fail_all(FELICS_E_INVALID_ARGUMENT);
    // a stream of this shape is never longer than this: a caller's length beyond it is not a stream (and not a size to allocate)
    const uint64_t max_len = felics_max_compressed_size(hdr.width, hdr.height, hdr.color_type, hdr.pixel_depth);
    const int forced16 = dec16_lanes_forced();
    if (bps == 2 && hdr.width >= 8 && decode16_lds_bytes(hdr.width) <= DECODE_LDS_LIMIT &&
        (forced16 == 1 || (forced16 < 0 && n >= (planes == 3 ? DECODE16_LANES_MIN_STREAMS_RGB : DECODE16_LANES_MIN_STREAMS)))) {
        // 16-bit streams 64 to a wave (k_decode16_lanes): passes of whole waves, bounded by the hashed tables' memory
        const size_t tb1 = decode16_lanes_table_bytes(1, hdr.width, hdr.height, hdr.color_type);
        const size_t n64 = (n + 63) / 64 * 64;
        size_t tbytes = 0;
        if ((rc = dec16_lanes_tables(ctx, std::min(n64, dec16_lanes_pass_cap()) * tb1, 64 * tb1, tbytes)) != 0) return fail_all(rc);
        const size_t per = std::min(n64, tbytes / tb1 / 64 * 64);
        const size_t most = std::min(per, n);
        if ((rc = dec16_buffers(ctx, most, hdr)) != 0) return fail_all(rc);
        ds.lanes16 += n;
        ds.lanes16_table_bytes = most * tb1;
        return decode16_passes(ctx, n, per, d_streams, offsets, lens, hdr, d_pixels, launch_decode16_lanes, ctx->dec_lane16_table, dec16_lanes_epoch, status);
    }
    if (bps == 2 && decode16_lds_bytes(hdr.width) <= DECODE_LDS_LIMIT) {
        // 16-bit streams a wave each: passes of at most DEC16_PASS streams (a stream's estimator table is 8.4 MB of HBM)
        // (and of at most a quarter of the free HBM; an allocation that fails all the same halves the pass)
        size_t per = 0;
        if ((rc = dec16_tables(ctx, n, per)) != 0) return fail_all(rc);
        if ((rc = dec16_buffers(ctx, per, hdr)) != 0) return fail_all(rc);
        ds.wave16 += n;
        return decode16_passes(ctx, n, per, d_streams, offsets, lens, hdr, d_pixels, launch_decode16, ctx->dec_table, dec16_epoch, status);
    }
    if (bps == 2 || decode8_lds_bytes(hdr.width, hdr.color_type) > DECODE_LDS_LIMIT) {
        // host decoder, stream by stream
        std::vector<uint8_t> sbuf, pbuf;
        try {
            pbuf.resize((size_t)frame_bytes);
            sbuf.reserve((size_t)std::min<uint64_t>(max_len, 1ull << 32));
        } catch (const std::bad_alloc &) {
            return fail_all(FELICS_E_IO);
        }
        ds.host += n;
        int first_rc = FELICS_OK;
        for (size_t i = 0; i < n; i++) {
            const int r = host_decode(ctx, (const uint8_t *)d_streams + offsets[i], lens[i], max_len, hdr, (uint8_t *)d_pixels + i * frame_bytes,
                                      sbuf, pbuf);
            if (r == FELICS_E_HIP) {
                for (size_t k = i; k < n; k++) status[k] = FELICS_E_HIP;
                return r;
            }
            if (r == HOST_DECODE_NO_MEMORY) {
                for (size_t k = i; k < n; k++) status[k] = FELICS_E_IO;
                return first_rc ? first_rc : FELICS_E_IO;
            }
            status[i] = r;
            if (r && !first_rc) first_rc = r;
        }
        return first_rc;
    }
    // offsets | lens | status on the device
    const size_t meta = n * 8 * 2 + n * 4;
    if ((rc = reserve(ctx, ctx->dec_meta, meta)) != 0) return fail_all(rc);
    uint64_t *d_off = (uint64_t *)ctx->dec_meta.p, *d_len = d_off + n;
    int *d_status = (int *)(d_len + n);
    int16_t *d_planes = nullptr;
    if (planes == 3) {
        if ((rc = reserve(ctx, ctx->dec_planes, (size_t)(npix * 3 * 2 * n) + 64)) != 0) return fail_all(rc);
        d_planes = (int16_t *)ctx->dec_planes.p;
    }
    hipStream_t s = l.stream;
    for (size_t i = 0; i < n; i++) status[i] = FELICS_E_HIP;  // until the kernel's own word arrives
    HIP_TRY(ctx, hipMemcpyAsync(d_off, offsets, n * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(ctx, hipMemcpyAsync(d_len, lens, n * 8, hipMemcpyHostToDevice, s));
    HIP_TRY(ctx, hipMemsetAsync(d_status, 0xFF, n * 4, s));
    // hundreds of streams and more: 64 streams per wave (lane = stream); fewer: one wave per stream
    // (FELICS_TEST_DECODE_LANES=1 / =0 force one form whatever the batch: tests)
    bool by_lane = hdr.width >= 8 && n >= (planes == 3 ? DECODE8_LANES_MIN_STREAMS_RGB : DECODE8_LANES_MIN_STREAMS);
    if (const char *e = getenv("FELICS_TEST_DECODE_LANES")) by_lane = hdr.width >= 8 && atoi(e) != 0;
    if (by_lane) {
        const size_t tb = decode8_lanes_table_bytes((uint32_t)n, hdr.color_type);
        if ((rc = reserve(ctx, ctx->dec_lane_table, tb)) != 0) return fail_all(rc);
        ds.lanes8 += n;
        HIP_TRY(ctx, hipMemsetAsync(ctx->dec_lane_table.p, 0, tb, s));
        HIP_TRY(ctx, launch_decode8_lanes(s, (const uint8_t *)d_streams, d_off, d_len, (uint32_t)n, hdr.width, hdr.height, hdr.color_type,
                                          (uint8_t *)d_pixels, d_planes, (uint32_t *)ctx->dec_lane_table.p, d_status));
    } else {
        ds.wave8 += n;
        HIP_TRY(ctx, launch_decode8(s, (const uint8_t *)d_streams, d_off, d_len, (uint32_t)n, hdr.width, hdr.height, hdr.color_type,
                                    (uint8_t *)d_pixels, d_planes, d_status));
    }
    HIP_TRY(ctx, hipMemcpyAsync(status, d_status, n * 4, hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipStreamSynchronize(s));
    return first_error(status, n);
}

uint32_t felics_index_lanes_min_items(int color) { return color ? INDEX8_LANES_MIN_ITEMS_RGB : INDEX8_LANES_MIN_ITEMS; }

int felics_get_index_stats(const felics_ctx *ctx, felics_index_stats *out, size_t out_size) {
    return copy_stats(ctx, &felics_ctx::istats, out, out_size);
}

int felics_decompress_batch_device_indexed(felics_ctx *ctx, size_t n, const void *d_streams, const uint64_t *offsets, const uint64_t *lens,
                                           const void *d_index, size_t index_stride, void *d_pixels, size_t d_pixels_cap, felics_header *hdr_out,
                                           int *status) {
    return dense_indexed(ctx, n, d_streams, offsets, lens, d_pixels, d_pixels_cap, hdr_out, status, IndexSame8{{}, (const uint8_t *)d_index, index_stride});
}

int felics_get_index_wide_stats(const felics_ctx *ctx, felics_index16_stats *out, size_t out_size) {
    return copy_stats(ctx, &felics_ctx::i16stats, out, out_size);
}

int felics_decompress_batch_device_indexed_wide(felics_ctx *ctx, size_t n, const void *d_streams, const uint64_t *offsets, const uint64_t *lens,
                                             const void *d_index, const uint64_t *idx_offsets, const uint64_t *idx_lens, void *d_pixels,
                                             size_t d_pixels_cap, felics_header *hdr_out, int *status) {
    return dense_indexed(ctx, n, d_streams, offsets, lens, d_pixels, d_pixels_cap, hdr_out, status,
                         IndexSame16{{}, (const uint8_t *)d_index, idx_offsets, idx_lens});
}

int felics_get_region_stats(const felics_ctx *ctx, felics_region_stats *out, size_t out_size) {
    return copy_stats(ctx, &felics_ctx::rstats, out, out_size);
}

int felics_decompress_regions_device_indexed(felics_ctx *ctx, size_t n_streams, const void *d_streams, const uint64_t *offsets,
                                             const uint64_t *lens, const void *d_index, size_t index_stride, size_t n_regions,
                                             const felics_region *regions, void *d_pixels, size_t d_pixels_cap, uint64_t *out_offsets,
                                             felics_header *hdr_out, int *status) {
    return regions_indexed(ctx, n_streams, d_streams, offsets, lens, n_regions, regions, d_pixels, d_pixels_cap, out_offsets, hdr_out, status,
                           IndexSame8{{}, (const uint8_t *)d_index, index_stride});
}

int felics_get_region_wide_stats(const felics_ctx *ctx, felics_region16_stats *out, size_t out_size) {
    return copy_stats(ctx, &felics_ctx::r16stats, out, out_size);
}

int felics_decompress_regions_device_indexed_wide(felics_ctx *ctx, size_t n_streams, const void *d_streams, const uint64_t *offsets,
                                                  const uint64_t *lens, const void *d_index, const uint64_t *idx_offsets,
                                                  const uint64_t *idx_lens, size_t n_regions, const felics_region *regions, void *d_pixels,
                                                  size_t d_pixels_cap, uint64_t *out_offsets, felics_header *hdr_out, int *status) {
    return regions_indexed(ctx, n_streams, d_streams, offsets, lens, n_regions, regions, d_pixels, d_pixels_cap, out_offsets, hdr_out, status,
                           IndexSame16{{}, (const uint8_t *)d_index, idx_offsets, idx_lens});
}

int felics_read_headers_device(felics_ctx *ctx, size_t n, const void *d_streams, const uint64_t *offsets, const uint64_t *lens,
                               felics_header *hdrs, int *status) {
    if (!ctx || (n && (!d_streams || !offsets || !lens || !hdrs || !status))) return FELICS_E_INVALID_ARGUMENT;
    auto fail_all = [&](int code) { return fail_call(n, status, hdrs, nullptr, code); };
    if (ctx->failed) return fail_all(FELICS_E_HIP);
    if (n == 0) return FELICS_OK;
    if (any_pending(ctx)) return fail_all(FELICS_E_INVALID_ARGUMENT);  // felics_wait_batch first
    if (n > 0xFFFFFFFFull) return fail_all(FELICS_E_INVALID_ARGUMENT);
    if (hipSetDevice(ctx->device) != hipSuccess) return fail_all(hip_fail(ctx, hipGetLastError(), "hipSetDevice"));
    // one launch, one copy back
    std::vector<DecodeHeader> rec;
    const int rc = read_headers(ctx, n, d_streams, offsets, lens, rec, ctx->lanes[0].stream);
    if (rc) return fail_all(rc);
    int first = FELICS_OK;
    for (size_t i = 0; i < n; i++) {
        status[i] = rec[i].status;
        hdrs[i] = rec[i].status == FELICS_OK ? felics_header{rec[i].color, rec[i].depth, rec[i].W, rec[i].H} : felics_header{};
        if (rec[i].status && !first) first = rec[i].status;
    }
    return first;
}

int felics_decompress_images_device(felics_ctx *ctx, size_t n, const void *d_streams, const uint64_t *offsets, const uint64_t *lens,
                                    void *d_pixels, size_t d_pixels_cap, uint64_t *pix_offsets, felics_header *hdrs, int *status) {
    if (!ctx || (n && (!d_streams || !offsets || !lens || !pix_offsets || !status))) return FELICS_E_INVALID_ARGUMENT;
    auto fail_all = [&](int code) { return fail_call(n, status, hdrs, pix_offsets, code); };
    if (ctx->failed) return fail_all(FELICS_E_HIP);
    if (n == 0) return FELICS_OK;
    if (any_pending(ctx)) return fail_all(FELICS_E_INVALID_ARGUMENT);  // felics_wait_batch first
    if (n > 0xFFFFFFFFull) return fail_all(FELICS_E_INVALID_ARGUMENT);
    if (hipSetDevice(ctx->device) != hipSuccess) return fail_all(hip_fail(ctx, hipGetLastError(), "hipSetDevice"));
    return decompress_images(ctx, n, d_streams, offsets, lens, (uint8_t *)d_pixels, d_pixels_cap, pix_offsets, hdrs, status);
}

int felics_decompress_views_device(felics_ctx *ctx, size_t n, const void *d_streams, const uint64_t *offsets, const uint64_t *lens,
                                   const felics_view *views, void *ready_event, felics_header *hdrs, int *status) {
    if (!ctx || (n && (!d_streams || !offsets || !lens || !views || !status))) return FELICS_E_INVALID_ARGUMENT;
    auto fail_all = [&](int code) { return fail_call(n, status, hdrs, nullptr, code); };
    for (size_t i = 0; i < n; i++) {  // every view checked before anything is launched: the first error in view order
        const int rc = felics_view_writable(&views[i]);
        if (rc) return fail_all(rc);
    }
    if (ctx->failed) return fail_all(FELICS_E_HIP);
    if (n == 0) return FELICS_OK;
    if (any_pending(ctx)) return fail_all(FELICS_E_INVALID_ARGUMENT);  // felics_wait_batch first
    if (n > 0xFFFFFFFFull) return fail_all(FELICS_E_INVALID_ARGUMENT);
    if (hipSetDevice(ctx->device) != hipSuccess) return fail_all(hip_fail(ctx, hipGetLastError(), "hipSetDevice"));
    // the class of every view, and the staged frames of the scattered ones (256-byte steps)
    std::vector<uint8_t> cls(n, VIEW_DENSE);
    std::vector<uint64_t> stage(n, 0), frame(n, 0);
    felics_decode_view_stats add = {};
    uint64_t stage_total = 0, stage_largest = 0;
    for (size_t i = 0; i < n; i++) {
        const felics_view &v = views[i];
        const int64_t size = v.depth == FELICS_DEPTH_16 ? 2 : 1;
        const bool rgb = v.color == FELICS_COLOR_RGB;
        const uint64_t npix = (uint64_t)v.width * v.height;
        add.views++;
        const bool dense = v.pixel_stride == size * (rgb ? 3 : 1) && v.row_stride == (int64_t)v.width * v.pixel_stride && (!rgb || v.channel_stride == size);
        if (!npix) {
            add.dense++;
        } else if (rows_for_host(v.width, rgb, v.depth)) {
            cls[i] = VIEW_SCATTERED;
        } else if (dense) {
            add.dense++;
        } else if (rgb || (v.pixel_stride == size && v.row_stride >= (int64_t)v.width * size)) {
            cls[i] = VIEW_IN_PLACE;
            add.in_place++;
        } else {
            cls[i] = VIEW_SCATTERED;
        }
        if (cls[i] == VIEW_SCATTERED) {
            add.scattered++;
            frame[i] = (npix * (rgb ? 3 : 1) * size + 255) & ~255ull;
            stage_total += frame[i];
            stage_largest = std::max(stage_largest, frame[i]);
        }
    }
    // The staging is bounded as the 16-bit lane tables are: passes of consecutive streams whose staged frames fit a quarter of the free
    // device memory (the buffer the context already holds counted as free); a single larger frame is a pass of its own.
    // FELICS_TEST_VIEW_STAGE_BYTES=k: at most k bytes a pass (tests).
    uint64_t budget = UINT64_MAX;
    size_t free_b = 0, total_b = 0;
    if (stage_total > ctx->view_stage.cap && hipMemGetInfo(&free_b, &total_b) == hipSuccess) budget = ((uint64_t)free_b + ctx->view_stage.cap) / 4;
    if (const char *e = getenv("FELICS_TEST_VIEW_STAGE_BYTES"))
        if (atoll(e) > 0) budget = (uint64_t)atoll(e);
    std::vector<size_t> pass_end;
    uint64_t acc = 0, most = 0;
    for (size_t i = 0; i < n; i++) {
        if (acc && acc + frame[i] > budget) {
            pass_end.push_back(i);
            acc = 0;
        }
        stage[i] = acc;
        acc += frame[i];
        most = std::max(most, acc);
    }
    pass_end.push_back(n);
    int rc;
    if (most && (rc = reserve(ctx, ctx->view_stage, (size_t)most + 64)) != 0) return fail_all(rc);
    ctx->dvstats.views += add.views;
    ctx->dvstats.dense += add.dense;
    ctx->dvstats.in_place += add.in_place;
    ctx->dvstats.scattered += add.scattered;
    ctx->view_ready = (hipEvent_t)ready_event;
    std::vector<uint64_t> addr(n, 0);
    int first = FELICS_OK;
    uint64_t table_bytes = 0;
    size_t i0 = 0;
    for (size_t i1 : pass_end) {
        const ViewPlan vp{views + i0, cls.data() + i0, stage.data() + i0};
        rc = decompress_images(ctx, i1 - i0, d_streams, offsets + i0, lens + i0, nullptr, SIZE_MAX, addr.data() + i0, hdrs ? hdrs + i0 : nullptr,
                               status + i0, &vp);
        table_bytes = std::max(table_bytes, ctx->dstats.lanes16_table_bytes);
        if (rc && !first) first = rc;
        if (rc == FELICS_E_HIP && ctx->err.size() && i1 < n) {  // (not a stream's status: the call ends here)
            fail_call(n - i1, status + i1, hdrs ? hdrs + i1 : nullptr, nullptr, rc);
            break;
        }
        i0 = i1;
    }
    ctx->dstats.lanes16_table_bytes = table_bytes;
    ctx->view_ready = nullptr;
    return first;
}

int felics_get_index_view_stats(const felics_ctx *ctx, felics_index_view_stats *out, size_t out_size) {
    return copy_stats(ctx, &felics_ctx::ivstats, out, out_size);
}

int felics_decompress_views_device_indexed(felics_ctx *ctx, size_t n, const void *d_streams, const uint64_t *offsets, const uint64_t *lens,
                                           const void *d_index, const uint64_t *idx_offsets, const uint64_t *idx_lens, const felics_view *views,
                                           void *ready_event, felics_header *hdrs, int *status) {
    return felics::views_indexed_call(ctx, n, d_streams, offsets, lens, d_index, idx_offsets, idx_lens, views, ready_event, hdrs, status,
                                      felics::IndexViews8{});
}

int felics_get_index_view_wide_stats(const felics_ctx *ctx, felics_index16_view_stats *out, size_t out_size) {
    return copy_stats(ctx, &felics_ctx::iv16stats, out, out_size);
}

int felics_decompress_views_device_indexed_wide(felics_ctx *ctx, size_t n, const void *d_streams, const uint64_t *offsets, const uint64_t *lens,
                                                const void *d_index, const uint64_t *idx_offsets, const uint64_t *idx_lens,
                                                const felics_view *views, void *ready_event, felics_header *hdrs, int *status) {
    return felics::views_indexed_call(ctx, n, d_streams, offsets, lens, d_index, idx_offsets, idx_lens, views, ready_event, hdrs, status,
                                      felics::IndexViews16{});
}

int felics_get_region_view_stats(const felics_ctx *ctx, felics_region_view_stats *out, size_t out_size) {
    return copy_stats(ctx, &felics_ctx::rvstats, out, out_size);
}

int felics_decompress_region_views_device_indexed(felics_ctx *ctx, size_t n_streams, const void *d_streams, const uint64_t *offsets,
                                                  const uint64_t *lens, const void *d_index, const uint64_t *idx_offsets,
                                                  const uint64_t *idx_lens, size_t n_regions, const felics_region *regions,
                                                  const felics_view *views, void *ready_event, felics_header *hdrs, int *status) {
    return felics::region_views_call(ctx, n_streams, d_streams, offsets, lens, d_index, idx_offsets, idx_lens, n_regions, regions, views,
                                     ready_event, hdrs, status, felics::RegionViews8{});
}

int felics_get_region_view_wide_stats(const felics_ctx *ctx, felics_region16_view_stats *out, size_t out_size) {
    return copy_stats(ctx, &felics_ctx::rv16stats, out, out_size);
}

int felics_decompress_region_views_device_indexed_wide(felics_ctx *ctx, size_t n_streams, const void *d_streams, const uint64_t *offsets,
                                                       const uint64_t *lens, const void *d_index, const uint64_t *idx_offsets,
                                                       const uint64_t *idx_lens, size_t n_regions, const felics_region *regions,
                                                       const felics_view *views, void *ready_event, felics_header *hdrs, int *status) {
    return felics::region_views_call(ctx, n_streams, d_streams, offsets, lens, d_index, idx_offsets, idx_lens, n_regions, regions, views,
                                     ready_event, hdrs, status, felics::RegionViews16{});
}

}  // extern "C"
