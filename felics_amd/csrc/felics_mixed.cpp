// felics_mixed.cpp -- images of different shapes in one call (felics_compress_images*) and strided views of device surfaces
// (felics_compress_views_device): buckets, the mixed sub-batches' plane tables, landing and remedies; the restart indexes of
// such a call (felics_compress_views_device_indexed, felics_index_plan; 16-bit: felics_compress_views_device_indexed16, placed by the
// library where a sub-batch lands -- emit_index16_views).
#include "felics_host.h"
#include "felics_index.h"
#include "felics_viewcheck.h"

namespace felics {

namespace {

// ---- mixed shapes (felics_compress_images*) ------------------------------------------------------------------------------
// 8-bit images go in BUCKETS of similar size: sorted by sort tiles T = ceil(w h / SORT_TILE), a bucket holds T_min .. ceil(1.25 T_min)
// (at most 25 % of a bucket's tiles are padding), and a bucket is one sub-batch whose tile count is uniform at its T_max; what
// differs per plane (samples, W, H, npix, the image's slot) comes from a table (Geometry::mixed).  16-bit images are bucketed by the
// same rule; a bucket (or a pass of one) of ONE shape takes the uniform path (frames gathered in mix_in, streams copied out of
// mix_stage), every other one is a mixed 16-bit sub-batch: run_wide with the table, frames read in place, streams straight into
// their slots.  The sub-batches are queued over the lanes like felics_compress_batch's chunks.

constexpr size_t MIX_MAX_IMAGES = 8192;  // images of one mixed sub-batch (k_concat_planes / k_rgb8_to_planes_mixed: one grid row per image)

// Image m as a dense frame at dst: a copy, or the gather of its view (counted: felics_view_stats::bytes_staged, or -- a surfaces call
// at work -- felics_surface_stats::bytes_staged).
int stage_frame(felics_ctx *ctx, hipStream_t s, void *dst, const MixImage &m) {
    if (!m.frame_bytes) return FELICS_OK;
    if (!m.view) {
        HIP_TRY(ctx, hipMemcpyAsync(dst, m.px, m.frame_bytes, hipMemcpyDeviceToDevice, s));
        return FELICS_OK;
    }
    if (m.depth == FELICS_DEPTH_16)
        launch_gather_view<uint16_t>(s, m.vr, m.w, m.h, m.planes, (uint16_t *)dst);
    else
        launch_gather_view<uint8_t>(s, m.vr, m.w, m.h, m.planes, (uint8_t *)dst);
    HIP_TRY(ctx, hipGetLastError());
    *(ctx->staged_bytes ? ctx->staged_bytes : &ctx->vstats.bytes_staged) += m.frame_bytes;
    return FELICS_OK;
}

MixImage mix_image(const felics_image &im) {
    MixImage m;
    m.px = (const uint8_t *)im.pixels;
    m.w = im.width;
    m.h = im.height;
    m.color = im.color;
    m.depth = im.depth;
    m.npix = (uint64_t)im.width * im.height;
    m.planes = im.color == FELICS_COLOR_RGB ? 3 : 1;
    m.frame_bytes = (size_t)(m.npix * m.planes * (im.depth == FELICS_DEPTH_16 ? 2 : 1));
    return m;
}

// every image checked before anything is launched: the first error in image order
int check_images(size_t n, const felics_image *images) {
    for (size_t i = 0; i < n; i++) {
        const felics_image &im = images[i];
        int rc = check_args(im.width, im.height, im.color, im.depth);
        if (rc) return rc;
        const MixImage m = mix_image(im);
        if (!im.pixels && m.npix) return FELICS_E_INVALID_ARGUMENT;
        if (m.npix * m.planes >= 0xE0000000ull) return FELICS_E_UNSUPPORTED;
        if (m.depth == FELICS_DEPTH_16 && m.npix > WIDE_MAX_PLANE_PIXELS) return FELICS_E_UNSUPPORTED;
    }
    return FELICS_OK;
}

uint32_t sort_tiles_of(uint64_t npix) { return (uint32_t)((npix + SORT_TILE - 1) / SORT_TILE); }

struct MixJob {
    bool wide = false;          // a 16-bit group of one shape (uniform path), else a mixed sub-batch ...
    bool wide_mixed = false;    // ... of 16-bit images (launch_mixed_wide), else of 8-bit ones (launch_mixed)
    std::vector<size_t> idx;    // its images
    int lane = -1;
    size_t in_off = 0, stage_off = 0;  // 16-bit: where its frames are gathered (mix_in; mixed: its views only) and, one shape, its streams land (mix_stage)
    uint64_t slot = 0;                 // 16-bit group of one shape: its slot in mix_stage
};

// Where a call's streams go: image i at base + off[i], at most slot[i] bytes.  lens[i] = the size of stream i whether it fit or
// not; overflow = one did not (the caller places the streams exactly and runs again).
struct MixOut {
    uint8_t *base;
    const uint64_t *off, *slot;
    uint64_t *lens;
    bool overflow;
    bool want_index = true;  // the images' restart indexes as well (MixImage::index / index16); false: a run for the sizes alone
    Index16Place *ix = nullptr;  // felics_compress_views_device_indexed16: where the version-2 indexes go
};

// image m's index is to be written by this run
bool wants_index(const MixImage &m, const MixOut &o) { return o.want_index && m.index != nullptr; }
// ... its version-2 index (placed by the library: Index16Place)
bool wants_index16(const MixImage &m, const MixOut &o) { return o.want_index && o.ix && m.index16; }
// the segment that groups the images of a remedy: the uniform writers take one per call
uint32_t index_segment(const MixImage &m, const MixOut &o) { return wants_index(m, o) || wants_index16(m, o) ? m.segment_pixels : 0u; }

// The per-checkpoint workspace of the version-2 writers (bitmap and prefix: a bit and a share of a word per context; n_rows, rows_off)
uint64_t index16_cp_bytes(int color) { return index16_words_per_checkpoint((uint32_t)color) * 8ull + 12u; }
// the checkpoints image m adds to a sub-batch that writes its index
uint64_t index16_cps(const MixImage &m) { return (uint64_t)m.planes * index16_layout(m.w, m.h, (uint32_t)m.color, m.segment_pixels).K; }

// an index has been written by a kernel (felics_index_emit_stats)
void count_index(felics_ctx *ctx, const MixImage &m, bool mixed) {
    ctx->iestats.indexes++;
    ctx->iestats.checkpoints += (uint64_t)m.planes * index_layout(m.w, m.h, (uint32_t)m.color, m.segment_pixels).K;
    (mixed ? ctx->iestats.in_mixed : ctx->iestats.redone)++;
}

// a view's dense copy in a mixed 16-bit job's part of mix_in: 256-byte steps
size_t gather_step(const MixImage &m) { return m.view && !m.wide_in_place ? (m.frame_bytes + 255) & ~(size_t)255 : 0; }

// The head of a mixed sub-batch of either depth on lane l, whose first kernel runs on stream s: the padded geometry (every plane
// T_max tiles of SORT_TILE samples: the stride of the RGB planes buffer and of k_map), the planes buffer, the pinned table (with
// one extra row per plane for what views add) and its device copy of tbytes, and -- behind the caller's ready event -- the
// profiling span.  max_npix = the largest image's pixels.  The caller fills the rows (plane_rows) and uploads them (upload_table).
int begin_mixed(felics_ctx *ctx, Lane &l, const std::vector<MixImage> &im, const std::vector<size_t> &idx, int depth, int nslices, hipStream_t s,
                size_t tbytes, uint64_t &max_npix) {
    const MixImage &f = im[idx[0]];
    uint32_t tmax = 0;
    max_npix = 0;
    for (size_t i : idx) {
        tmax = std::max(tmax, sort_tiles_of(im[i].npix));
        max_npix = std::max(max_npix, im[i].npix);
    }
    const Geometry &g = begin_sub_batch(ctx, l, 0, idx.size(), SORT_TILE, tmax, f.color, depth, nslices, true);
    int rc;
    if (f.planes == 3 && (rc = reserve(ctx, l.planes, (size_t)g.nplanes * g.npix * (depth == FELICS_DEPTH_16 ? 4 : 2) + STAGE_PAD)) != 0) return rc;
    static_assert(sizeof(PitchedGeom) >= sizeof(ViewRow) && sizeof(PlaneGeom) % 8 == 0, "one extra row per plane holds either");
    // (... and one IndexGeom per plane for the indexes of felics_compress_views_device_indexed)
    if ((rc = reserve_pinned(ctx, (void **)&l.h_table, l.h_table_cap, g.nplanes,
                             (size_t)g.nplanes * (sizeof(PlaneGeom) + sizeof(PitchedGeom) + sizeof(IndexGeom)))) != 0)
        return rc;
    if ((rc = reserve(ctx, l.mtable, tbytes)) != 0) return rc;
    if ((rc = wait_ready(ctx, s)) != 0) return rc;
    if (ctx->profiling) HIP_TRY(ctx, hipEventRecord(l.span_begin, s));
    return FELICS_OK;
}

// The table rows of image j of the sub-batch (image i of the call, dense at `frame`): gray samples are read where the frame lies, the
// planes of an RGB image from the lane's planes buffer (int16 / int32 samples: sample_bytes), where the plane transform puts them.
void plane_rows(Lane &l, size_t j, const MixImage &m, const void *frame, size_t sample_bytes, const MixOut &o, size_t i) {
    for (uint32_t c = 0; c < m.planes; c++) {
        PlaneGeom &pg = l.h_table[j * m.planes + c];
        pg.samples = m.planes == 3 ? (const void *)((const uint8_t *)l.planes.p + (j * m.planes + c) * l.g.npix * sample_bytes) : frame;
        pg.image = frame;
        pg.W = m.w;
        pg.H = m.h;
        pg.npix = (uint32_t)m.npix;
        pg.ntiles = (uint32_t)((m.npix + PACK_TILE - 1) / PACK_TILE);
        pg.out_off = o.off[i];
        pg.out_slot = o.slot[i];
    }
}

// The filled table to the device; from here on the sub-batch is a mixed one (every plane's samples come from the table).
int upload_table(felics_ctx *ctx, Lane &l, size_t tbytes, hipStream_t s) {
    HIP_TRY(ctx, hipMemcpyAsync(l.mtable.p, l.h_table, tbytes, hipMemcpyHostToDevice, s));
    l.g.mixed = (const PlaneGeom *)l.mtable.p;
    l.d_planes = l.g.planes_per_image == 3 ? l.planes.p : nullptr;
    return FELICS_OK;
}

// Queues a mixed 8-bit sub-batch on lane l (see launch_sub_batch).  Views are read where they lie: behind the table, the pitched
// policy's rows of a gray sub-batch (Geometry::pitched), the views of an RGB one (the dense images as views of their own).
int launch_mixed(felics_ctx *ctx, Lane &l, const std::vector<MixImage> &im, const std::vector<size_t> &idx, const MixOut &o, int nslices) {
    const uint32_t planes = im[idx[0]].planes;
    const size_t cnt = idx.size();
    bool any_view = false;
    for (size_t i : idx) any_view = any_view || im[i].view;
    const size_t extra_off = cnt * planes * sizeof(PlaneGeom);
    bool any_index = false;
    for (size_t i : idx) any_index = any_index || wants_index(im[i], o);
    static_assert(sizeof(PitchedGeom) % 8 == 0 && sizeof(ViewRow) % 8 == 0, "the IndexGeom rows behind them hold pointers");
    const size_t index_off = extra_off + (any_view ? (planes == 1 ? cnt * sizeof(PitchedGeom) : cnt * sizeof(ViewRow)) : 0);
    const size_t tbytes = index_off + (any_index ? cnt * planes * sizeof(IndexGeom) : 0);
    hipStream_t fs = ctx->serial ? l.stream : l.front;
    uint64_t max_npix;
    int rc = begin_mixed(ctx, l, im, idx, FELICS_DEPTH_8, nslices, fs, tbytes, max_npix);
    if (rc) return rc;
    PitchedGeom *h_pitched = (PitchedGeom *)((uint8_t *)l.h_table + extra_off);  // gray
    ViewRow *h_views = (ViewRow *)((uint8_t *)l.h_table + extra_off);            // RGB
    for (size_t j = 0; j < cnt; j++) {
        const MixImage &m = im[idx[j]];
        plane_rows(l, j, m, m.px, 2, o, idx[j]);
        if (any_view && planes == 1) h_pitched[j] = PitchedGeom{l.h_table[j], m.pitch ? m.pitch : (uint64_t)m.w};  // (a dense plane: pitch = W)
        if (any_view && planes == 3) h_views[j] = m.view ? m.vr : ViewRow{m.px, 3ll * m.w, 3, 1};
        if (!any_index) continue;
        // the image's index, one row per plane (uploaded with the table: on the front stream, behind the ready event); its range is
        // zeroed and the rows are read on the tail stream, behind the sub-batch's last pack kernel (run_lane)
        IndexGeom ig{};
        if (wants_index(m, o)) {
            const IndexLayout L = index_layout(m.w, m.h, (uint32_t)m.color, m.segment_pixels);
            ig = IndexGeom{m.index, L.K, m.segment_pixels / SORT_TILE, L.cp_bytes, L.win_off};
            l.idx_max_K = std::max(l.idx_max_K, L.K);
            l.idx_zero.emplace_back(m.index, (size_t)L.total);
        }
        for (uint32_t c = 0; c < planes; c++) ((IndexGeom *)((uint8_t *)l.h_table + index_off))[j * planes + c] = ig;
    }
    if ((rc = upload_table(ctx, l, tbytes, fs)) != 0) return rc;
    if (any_index) l.idx_rows = (const IndexGeom *)((const uint8_t *)l.mtable.p + index_off);
    Geometry &g = l.g;
    if (any_view && planes == 1) g.pitched = (const PitchedGeom *)((const uint8_t *)l.mtable.p + extra_off);
    if (planes == 3) {
        StageTimer t(ctx, l, ST_PLANES, fs, true);
        if (any_view)
            launch_rgb8_view_to_planes(fs, g.mixed, (const ViewRow *)((const uint8_t *)l.mtable.p + extra_off), g.npix, (uint32_t)max_npix, (uint32_t)cnt);
        else
            launch_rgb8_to_planes_mixed(fs, g.mixed, g.npix, (uint32_t)max_npix, (uint32_t)cnt);
    }
    return run_sub_batch(ctx, l, o.base, 0);
}

// Queues a mixed 16-bit sub-batch on lane l: run_wide with the plane table.  gray16 frames are read where the caller has them, RGB16
// frames by the plane transform; a view is gathered to `gathered` first (stage_frame: counted in bytes_staged) and its rows point
// there -- unless it is marked wide_in_place (felics_submit_surfaces_device): then, behind the table, the 16-bit pitched rows of a gray
// sub-batch (Geometry::pitched16) or the views of an RGB one (the other images as views of their own), and nothing is gathered.
// Everything on the lane's one stream.
int launch_mixed_wide(felics_ctx *ctx, Lane &l, const std::vector<MixImage> &im, const std::vector<size_t> &idx, const MixOut &o, uint8_t *gathered,
                      int nslices) {
    const size_t cnt = idx.size();
    const uint32_t planes = im[idx[0]].planes;
    bool in_place = false;
    for (size_t i : idx) in_place = in_place || im[i].wide_in_place;
    static_assert(sizeof(PitchedGeom16) == sizeof(PitchedGeom), "the extra row begin_mixed reserves per plane holds either");
    const size_t extra_off = cnt * planes * sizeof(PlaneGeom);
    const size_t tbytes = extra_off + (in_place ? (planes == 1 ? cnt * sizeof(PitchedGeom16) : cnt * sizeof(ViewRow)) : 0);
    hipStream_t s = l.stream;
    uint64_t max_npix;
    int rc = begin_mixed(ctx, l, im, idx, FELICS_DEPTH_16, nslices, s, tbytes, max_npix);
    if (rc) return rc;
    PitchedGeom16 *h_pitched = (PitchedGeom16 *)((uint8_t *)l.h_table + extra_off);  // gray
    ViewRow *h_views = (ViewRow *)((uint8_t *)l.h_table + extra_off);                // RGB
    size_t at = 0;
    for (size_t j = 0; j < cnt; j++) {
        const MixImage &m = im[idx[j]];
        const uint8_t *frame = m.px;
        if (m.view && !m.wide_in_place) {
            frame = gathered + at;
            if ((rc = stage_frame(ctx, s, gathered + at, m)) != 0) return rc;
            at += gather_step(m);
        }
        plane_rows(l, j, m, frame, 4, o, idx[j]);
        if (in_place && planes == 1) h_pitched[j] = PitchedGeom16{l.h_table[j], m.wide_in_place ? m.pitch / 2 : (uint64_t)m.w};  // (in samples)
        if (in_place && planes == 3) h_views[j] = m.wide_in_place ? m.vr : ViewRow{frame, 6ll * m.w, 6, 2};
    }
    if ((rc = upload_table(ctx, l, tbytes, s)) != 0) return rc;
    const uint8_t *extra = (const uint8_t *)l.mtable.p + extra_off;
    if (in_place && planes == 1) l.g.pitched16 = (const PitchedGeom16 *)extra;
    if (planes == 3) {
        StageTimer t(ctx, l, ST_PLANES, s, true);
        if (in_place)
            launch_rgb16_view_to_planes(s, l.g.mixed, (const ViewRow *)extra, (uint32_t)max_npix, (uint32_t)cnt);
        else
            launch_rgb16_to_planes_mixed(s, l.g.mixed, (uint32_t)max_npix, (uint32_t)cnt);
    }
    return run_sub_batch(ctx, l, o.base, 0);
}

// Streams k of a group (lens[k] bytes at from + offs[k]) into the slots of the call's images idx[k], on the lane's main stream, and
// waits for them; a stream that outgrew its slot is not copied (o.overflow: the caller places the streams exactly and runs again).
int copy_to_slots(felics_ctx *ctx, Lane &l, const std::vector<size_t> &idx, const uint8_t *from, const uint64_t *offs, const uint64_t *lens, MixOut &o) {
    for (size_t k = 0; k < idx.size(); k++) {
        const size_t i = idx[k];
        o.lens[i] = lens[k];
        if (lens[k] > o.slot[i]) {
            o.overflow = true;
            continue;
        }
        HIP_TRY(ctx, hipMemcpyAsync(o.base + o.off[i], from + offs[k], (size_t)lens[k], hipMemcpyDeviceToDevice, l.stream));
    }
    HIP_TRY(ctx, hipStreamSynchronize(l.stream));
    return FELICS_OK;
}

// The remedy: the images of `idx` once more through encode_device (its whole ladder), one group per shape, frames gathered
// into one buffer, streams copied into their slots.
int redo_by_shape(felics_ctx *ctx, Lane &l, const std::vector<MixImage> &im, const std::vector<size_t> &idx, MixOut &o) {
    std::vector<size_t> rest = idx;
    int rc;
    while (!rest.empty()) {
        const MixImage &f = im[rest[0]];
        std::vector<size_t> grp, other;
        for (size_t i : rest) {
            const MixImage &m = im[i];
            const bool same = m.w == f.w && m.h == f.h && m.color == f.color && m.depth == f.depth;
            // (the uniform writer takes one segment per call: images that want indexes are grouped by their segment as well)
            (same && index_segment(m, o) == index_segment(f, o) ? grp : other).push_back(i);
        }
        rest.swap(other);
        const size_t cnt = grp.size();
        if ((rc = reserve(ctx, ctx->mix_redo, f.frame_bytes * cnt + 64)) != 0) return rc;
        if ((rc = wait_ready(ctx, l.stream)) != 0) return rc;
        for (size_t j = 0; j < cnt && f.frame_bytes; j++)  // (a view: gathered, the path wants dense frames)
            if ((rc = stage_frame(ctx, l.stream, (uint8_t *)ctx->mix_redo.p + j * f.frame_bytes, im[grp[j]])) != 0) return rc;
        HIP_TRY(ctx, hipStreamSynchronize(l.stream));
        std::vector<uint64_t> offs(cnt), lens(cnt);
        uint8_t *used = nullptr;
        // the group's indexes back to back in a buffer of the context, then each to where the caller wants it
        IndexRequest req{nullptr, 0, 0};
        if (wants_index(f, o)) {
            req.bytes = index_layout(f.w, f.h, (uint32_t)f.color, f.segment_pixels).total;
            req.segment_pixels = f.segment_pixels;
            if ((rc = reserve(ctx, ctx->mix_index, (size_t)(req.bytes * cnt))) != 0) return rc;
            req.d_index = (uint8_t *)ctx->mix_index.p;
        }
        // a 16-bit group: the uniform version-2 writer, into the caller's buffer behind what has been placed so far
        std::vector<uint64_t> ioffs(cnt), ilens(cnt);
        Index16Request rq16{nullptr, 0, f.segment_pixels, SIZE_MAX, ioffs.data(), ilens.data()};
        const bool ask16 = wants_index16(f, o);
        if (ask16) {
            Index16Place &ix = *o.ix;
            rq16.d_index = ix.d_index + ix.total;  // (every size is a multiple of 64: so is this)
            rq16.cap = ix.cap > ix.total ? ix.cap - ix.total : 0;
            rq16.pass_images = (size_t)std::max<uint64_t>(1, ix.budget / (index16_cps(f) * index16_cp_bytes(f.color) + 24u));
        }
        if ((rc = encode_device(ctx, l, cnt, ctx->mix_redo.p, f.w, f.h, f.color, f.depth, nullptr, 0, offs.data(), lens.data(), &used, false,
                                req.d_index ? &req : nullptr, ask16 ? &rq16 : nullptr)) != 0)
            return rc;
        if (ask16) {  // (encode_device has waited for its writer)
            Index16Place &ix = *o.ix;
            for (size_t j = 0; j < cnt; j++) {
                ix.idx_offsets[grp[j]] = ix.total + ioffs[j];
                ix.idx_lens[grp[j]] = ilens[j];
            }
            ix.total += rq16.total;
            ix.too_small = ix.too_small || rq16.too_small;
            ix.indexes += rq16.written;
            ix.redone += rq16.written;
            ix.rows += rq16.rows;
            ix.bytes += rq16.bytes;
        }
        for (size_t j = 0; j < cnt && req.d_index; j++) {  // (encode_device has waited for its writer; copy_to_slots waits for these)
            HIP_TRY(ctx, hipMemcpyAsync(im[grp[j]].index, req.d_index + j * req.bytes, (size_t)req.bytes, hipMemcpyDeviceToDevice, l.stream));
            count_index(ctx, im[grp[j]], false);
        }
        if ((rc = copy_to_slots(ctx, l, grp, used, offs.data(), lens.data(), o)) != 0) return rc;  // (waits: ctx->own is reused by the next group)
    }
    return FELICS_OK;
}

// The version-2 indexes of a 16-bit job that has landed usable (felics_compress_views_device_indexed16), by the table-driven writer
// (launch_index16_scan_table / _write_table) from what run_wide left in the lane's workspace -- emit_index16's shape: scan, read the
// totals back, place behind what has been placed so far, upload index_off, write.  One emitter for both kinds of job: a mixed
// sub-batch's rows take its PlaneGeom rows' samples, a same-shape group's rows all name one shape and point into the lane's planes
// (the gathered frames, or the Y / Co / Cg planes).  On the lane's stream, and complete on return: the next job reuses the workspace.
int emit_index16_views(felics_ctx *ctx, Lane &l, const MixJob &j, const std::vector<MixImage> &im, MixOut &o) {
    Index16Place &ix = *o.ix;
    const Geometry &g = l.g;
    const size_t cnt = j.idx.size();
    const uint32_t C = g.planes_per_image;
    const size_t sample_bytes = C == 3 ? 4 : 2;
    std::vector<Index16Geom> rows(cnt * C);
    std::vector<std::pair<uint32_t, uint32_t>> shapes;
    uint64_t cps = 0, max_rows_base = 0, max_npix = 0;
    for (size_t k = 0; k < cnt; k++) {
        const MixImage &m = im[j.idx[k]];
        const bool want = wants_index16(m, o);
        Index16Layout L{};
        if (want) L = index16_layout(m.w, m.h, (uint32_t)m.color, m.segment_pixels);
        for (uint32_t c = 0; c < C; c++) {
            Index16Geom &r = rows[k * C + c];
            r.samples = j.wide ? (const void *)((const uint8_t *)l.d_planes + (k * C + c) * (size_t)g.npix * sample_bytes) : l.h_table[k * C + c].samples;
            r.image = (uint32_t)k;
            r.c = c;
            r.W = m.w;
            r.H = m.h;
            r.npix = (uint32_t)m.npix;
            r.segment_pixels = want ? m.segment_pixels : 0;
            r.K = want ? L.K : 0;
            r.cp0 = (uint32_t)cps;
            r.win_base = L.win_base;
            r.win_bytes = L.win_bytes;
            r.rows_base = L.rows_base;
            cps += r.K;
        }
        if (!want) continue;
        max_rows_base = std::max(max_rows_base, L.rows_base);
        max_npix = std::max(max_npix, m.npix);
        if (std::find(shapes.begin(), shapes.end(), std::make_pair(m.w, m.h)) == shapes.end()) shapes.emplace_back(m.w, m.h);
    }
    if (cps == 0) return FELICS_OK;  // no image of the job asks for an index
    if (cps > 0xFFFFFFFFull) return FELICS_E_UNSUPPORTED;  // (never: the budget cuts a sub-batch far below)
    const uint32_t wpc = index16_words_per_checkpoint(g.color);
    int rc;
    if ((rc = reserve(ctx, l.i16_bitmap, (size_t)cps * wpc * 4)) != 0) return rc;
    if ((rc = reserve(ctx, l.i16_prefix, (size_t)cps * wpc * 4)) != 0) return rc;
    if ((rc = reserve(ctx, l.i16_nrows, (size_t)cps * 4)) != 0) return rc;
    if ((rc = reserve(ctx, l.i16_rows_off, (size_t)cps * 8)) != 0) return rc;
    if ((rc = reserve(ctx, l.i16_totals, cnt * 16)) != 0) return rc;
    if ((rc = reserve(ctx, l.i16_index_off, cnt * 8)) != 0) return rc;
    if ((rc = reserve(ctx, l.i16_table, rows.size() * sizeof(Index16Geom))) != 0) return rc;
    hipStream_t s = l.stream;
    if (ctx->poison) {
        DevBuf *bufs[] = {&l.i16_bitmap, &l.i16_prefix, &l.i16_nrows, &l.i16_rows_off, &l.i16_totals, &l.i16_index_off, &l.i16_table};
        for (DevBuf *b : bufs) HIP_TRY(ctx, hipMemsetAsync(b->p, 0xA5, b->cap, s));
    }
    HIP_TRY(ctx, hipMemcpyAsync(l.i16_table.p, rows.data(), rows.size() * sizeof(Index16Geom), hipMemcpyHostToDevice, s));
    const Index16TableEmit t{ix.d_index, (const uint64_t *)l.i16_index_off.p, (uint32_t *)l.i16_bitmap.p, (uint32_t *)l.i16_prefix.p,
                             (uint32_t *)l.i16_nrows.p, (uint64_t *)l.i16_rows_off.p, (uint64_t *)l.i16_totals.p, (const Index16Geom *)l.i16_table.p,
                             g.color, C, (uint32_t)(cnt * C), (uint32_t)cnt, (uint32_t)cps, wpc};
    const uint64_t *recs = (const uint64_t *)l.wrecs[0].p;
    const uint32_t *meta = (const uint32_t *)l.wmeta.p;
    launch_index16_scan_table(s, recs, meta, t, (uint32_t)max_npix);
    HIP_TRY(ctx, hipGetLastError());
    std::vector<uint64_t> totals(cnt * 2), where(cnt);
    HIP_TRY(ctx, hipMemcpyAsync(totals.data(), l.i16_totals.p, totals.size() * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipStreamSynchronize(s));
    uint64_t fit = 0, fit_rows = 0, fit_bytes = 0;
    for (size_t k = 0; k < cnt; k++) {
        const size_t i = j.idx[k];
        where[k] = ~0ull;
        if (!wants_index16(im[i], o)) continue;
        const uint64_t bytes = totals[2 * k];
        ix.idx_offsets[i] = ix.total;
        ix.idx_lens[i] = bytes;
        if (bytes <= ix.cap && ix.total <= ix.cap - bytes) {
            where[k] = ix.total;
            fit++, fit_rows += totals[2 * k + 1], fit_bytes += bytes;
        } else {
            ix.too_small = true;
        }
        ix.total += bytes;  // (rows_base and a row are multiples of 64: so is every offset)
    }
    if (fit == 0) return FELICS_OK;
    HIP_TRY(ctx, hipMemcpyAsync(l.i16_index_off.p, where.data(), where.size() * 8, hipMemcpyHostToDevice, s));
    launch_index16_write_table(s, recs, meta, (const uint64_t *)l.heads.p, (const uint32_t *)l.scalars.p, (const uint64_t *)l.tile_bitoff.p,
                               l.plane_base, l.plane_base - g.nplanes, g.pack_tiles, t, max_rows_base);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipStreamSynchronize(s));  // (`where` is pageable and leaves scope; the workspace is free again)
    ix.indexes += fit;
    ix.rows += fit_rows;
    ix.bytes += fit_bytes;
    ix.sub_batches++;
    ix.shapes_max = std::max<uint64_t>(ix.shapes_max, shapes.size());
    return FELICS_OK;
}

// A job's sub-batch is complete: sizes, its own checks, and the remedy where one is needed.
int land_job(felics_ctx *ctx, MixJob &j, const std::vector<MixImage> &im, MixOut &o) {
    Lane &l = ctx->lanes[j.lane];
    int rc = wait_event(ctx, l.sized, "stream sizes");
    if (rc) return rc;
    const size_t cnt = j.idx.size();
    if (j.wide) {
        std::vector<uint64_t> offs(cnt), lens(cnt);
        const SlotOutcome so = read_sizes(ctx, l, true, j.slot, offs.data(), lens.data());
        uint8_t *from = (uint8_t *)ctx->mix_stage.p + j.stage_off;
        if ((rc = sync_lane(ctx, l)) != 0) return rc;
        bool any16 = false;
        for (size_t i : j.idx) any16 = any16 || wants_index16(im[i], o);
        if (so.overflow && any16) {
            // ... and its images want version-2 indexes: the uniform writer takes one segment per call, so the group goes through the
            // remedy that groups by segment (frames gathered once more, streams copied into their slots)
            (void)apply_remedy(ctx, l, so);
            if ((rc = redo_by_shape(ctx, l, im, j.idx, o)) != 0) return rc;
            collect_timing(ctx, l);
            return FELICS_OK;
        }
        if (so.overflow) {  // a stream outgrew its slot: the group again with exact placement (encode_device)
            (void)apply_remedy(ctx, l, so);
            const MixImage &f = im[j.idx[0]];
            if ((rc = encode_device(ctx, l, cnt, (uint8_t *)ctx->mix_in.p + j.in_off, f.w, f.h, f.color, f.depth, nullptr, 0, offs.data(),
                                    lens.data(), &from, true)) != 0)
                return rc;
        }
        if ((rc = copy_to_slots(ctx, l, j.idx, from, offs.data(), lens.data(), o)) != 0) return rc;
        collect_timing(ctx, l);
        // (the pass was usable as it came out: its records, heads and bit offsets are still in the lane's workspace)
        if (any16 && (rc = emit_index16_views(ctx, l, j, im, o)) != 0) return rc;
        return FELICS_OK;
    }
    // a mixed sub-batch: its table lists the images in the order of j.idx (run_wide copies the sizes and nothing else: no status word)
    SlotOutcome so = j.wide_mixed ? SlotOutcome{} : decode_status(ctx, l, l.h_sizes[cnt]);
    for (size_t k = 0; k < cnt; k++) {
        const size_t i = j.idx[k];
        o.lens[i] = l.h_sizes[k];
        if (l.h_sizes[k] > o.slot[i]) so.overflow = true;
    }
    if (!so.redo() && !so.overflow && !so.spine_error) {
        if (j.wide_mixed && ctx->profiling && (rc = sync_lane(ctx, l)) != 0) return rc;  // (run_wide records span_end behind `sized`)
        collect_timing(ctx, l);
        for (size_t i : j.idx)  // (the mixed writers ran in front of `sized`: the indexes are complete)
            if (!j.wide_mixed && wants_index(im[i], o)) count_index(ctx, im[i], true);
        // a mixed 16-bit sub-batch: its version-2 indexes here, behind `sized` and before the lane's workspace is reused
        if (j.wide_mixed && o.want_index && o.ix) return emit_index16_views(ctx, l, j, im, o);
        return FELICS_OK;
    }
    if ((rc = sync_lane(ctx, l)) != 0) return rc;
    if ((rc = apply_remedy(ctx, l, so)) != 0) return rc;
    return redo_by_shape(ctx, l, im, j.idx, o);
}

// The jobs of the call's images of one depth and colour, appended to `jobs`.  Sorted by sort tiles T, a BUCKET holds T_min ..
// ceil(1.25 T_min); it is cut into passes by the pass bound of its padded planes (T_max * SORT_TILE samples: for 16-bit images that
// keeps planes * npix of a mixed sub-batch <= 2^30 samples, so the chain kernels' 32-bit kbase = plane * npix -- k_map is strided by
// the padded npix -- stays valid).  Every pass of 8-bit images is a mixed sub-batch.  A 16-bit bucket of ONE shape is cut by that
// shape's own npix (the passes that shape always had) and takes the uniform path, as does any other 16-bit pass that holds one shape.
// A run that writes version-2 indexes (o.ix) also cuts a 16-bit pass where its images' checkpoints would outgrow the workspace budget
// (or FELICS_TEST_INDEX16_EMIT_CPS), at least one image per pass; every other run is cut exactly as before.
void bucket_images(const std::vector<MixImage> &im, int depth, int color, const MixOut &o, std::vector<MixJob> &jobs) {
    const bool wide = depth == FELICS_DEPTH_16;
    const uint32_t planes = color == FELICS_COLOR_RGB ? 3 : 1;
    std::vector<size_t> v;
    for (size_t i = 0; i < im.size(); i++)
        if (im[i].npix && im[i].depth == depth && im[i].color == color) v.push_back(i);
    std::stable_sort(v.begin(), v.end(), [&](size_t a, size_t b) { return sort_tiles_of(im[a].npix) < sort_tiles_of(im[b].npix); });
    auto one_shape = [&](size_t first, size_t last) {
        for (size_t k = first; k < last; k++)
            if (im[v[k]].w != im[v[first]].w || im[v[k]].h != im[v[first]].h) return false;
        return true;
    };
    for (size_t a = 0; a < v.size();) {
        const uint64_t tmin = sort_tiles_of(im[v[a]].npix), lim = (5 * tmin + 3) / 4;  // ceil(1.25 T_min)
        size_t b = a;
        while (b < v.size() && sort_tiles_of(im[v[b]].npix) <= lim) b++;
        const bool uniform = wide && one_shape(a, b);
        const size_t per = uniform ? max_images_per_pass(im[v[a]].npix, planes, depth)
                                   : std::min(MIX_MAX_IMAGES, max_images_per_pass((uint64_t)sort_tiles_of(im[v[b - 1]].npix) * SORT_TILE, planes, depth));
        const bool cut_cps = wide && o.want_index && o.ix;
        const uint64_t cps_max = !cut_cps ? 0 : std::max<uint64_t>(1, std::min(o.ix->budget / index16_cp_bytes(color), o.ix->test_cps ? o.ix->test_cps : UINT64_MAX));
        for (size_t c = a, e; c < b; c = e) {
            e = std::min(b, c + per);
            if (cut_cps) {
                uint64_t cps = 0;
                for (size_t k = c; k < e; k++) {
                    cps += wants_index16(im[v[k]], o) ? index16_cps(im[v[k]]) : 0;
                    if (cps > cps_max && k > c) e = k;
                }
            }
            MixJob j;
            j.wide = wide && (uniform || one_shape(c, e));
            j.wide_mixed = wide && !j.wide;
            j.idx.assign(v.begin() + c, v.begin() + e);
            jobs.push_back(std::move(j));
        }
        a = b;
    }
}

// Every image of the call into the slots of `o`: zero-sized images on the host path, the jobs queued over the lanes.
int run_images(felics_ctx *ctx, const std::vector<MixImage> &im, MixOut &o) {
    const size_t n = im.size();
    int rc;
    o.overflow = false;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    std::vector<MixJob> jobs;
    for (int depth : {FELICS_DEPTH_8, FELICS_DEPTH_16})
        for (int color : {FELICS_COLOR_GRAY, FELICS_COLOR_RGB}) bucket_images(im, depth, color, o, jobs);
    size_t in_total = 0, stage_total = 0;  // 16-bit jobs: their parts of mix_in and mix_stage
    for (MixJob &j : jobs) {
        j.in_off = in_total;
        if (j.wide) {  // frames gathered back to back, streams into slots of one size
            const size_t fb = im[j.idx[0]].frame_bytes;
            j.slot = default_slot(fb);
            j.stage_off = stage_total;
            in_total += ((fb * j.idx.size()) + 255) & ~(size_t)255;
            stage_total += (size_t)(j.slot * j.idx.size());
        } else if (j.wide_mixed) {  // its views only
            for (size_t i : j.idx) in_total += gather_step(im[i]);
        }
    }
    if (in_total && (rc = reserve(ctx, ctx->mix_in, in_total + 64)) != 0) return rc;
    if (stage_total && (rc = reserve(ctx, ctx->mix_stage, stage_total + 64)) != 0) return rc;
    for (size_t i = 0; i < n; i++) {  // zero-sized images: header + two zero words per plane, encode_device's host path
        if (im[i].npix) continue;
        if (ctx->view_ready) HIP_TRY(ctx, hipStreamWaitEvent(nullptr, ctx->view_ready, 0));  // (the copy below runs on the null stream)
        uint64_t off = 0, len = 0;
        if ((rc = encode_device(ctx, ctx->lanes[0], 1, nullptr, im[i].w, im[i].h, im[i].color, im[i].depth, o.base + o.off[i], (size_t)o.slot[i], &off,
                                &len, nullptr)) != 0)
            return rc;
        o.lens[i] = len;
        if (wants_index(im[i], o)) {  // (K = 0: the header alone, built on the host as felics_compress_batch_device_indexed builds it)
            uint8_t ih[INDEX_HEADER_BYTES];
            empty_index(ih, im[i].w, im[i].h, (uint32_t)im[i].color, im[i].segment_pixels);
            HIP_TRY(ctx, hipMemcpy(im[i].index, ih, INDEX_HEADER_BYTES, hipMemcpyHostToDevice));
        }
        if (wants_index16(im[i], o)) {  // (the version-2 header alone, as felics_compress_batch_device_indexed16 builds it; placed like the others)
            Index16Place &ix = *o.ix;
            uint8_t ih[INDEX_HEADER_BYTES];
            empty_index(ih, im[i].w, im[i].h, (uint32_t)im[i].color, im[i].segment_pixels);
            ih[IDX_VERSION] = (uint8_t)INDEX16_VERSION;
            ih[IDX_DEPTH] = FELICS_DEPTH_16;
            ih[IDX16_TOTAL] = (uint8_t)INDEX_HEADER_BYTES;
            ix.idx_offsets[i] = ix.total;
            ix.idx_lens[i] = INDEX_HEADER_BYTES;
            if (ix.total + INDEX_HEADER_BYTES <= ix.cap) {
                HIP_TRY(ctx, hipMemcpy(ix.d_index + ix.total, ih, INDEX_HEADER_BYTES, hipMemcpyHostToDevice));
                ix.bytes += INDEX_HEADER_BYTES;
            } else {
                ix.too_small = true;
            }
            ix.total += INDEX_HEADER_BYTES;
        }
    }
    const int nslices = jobs.size() > 1 || ctx->only_lane >= 0 ? ctx->slices_queued : ctx->slices_blocking;
    std::vector<size_t> flying;  // jobs in flight, oldest first (lanes handed out in turn: the oldest holds the next lane)
    auto drain = [&](int r) {
        for (size_t f : flying) {
            (void)wait_event(ctx, ctx->lanes[jobs[f].lane].sized, "stream sizes");
            (void)sync_lane(ctx, ctx->lanes[jobs[f].lane]);
        }
        return r;
    };
    // (a surfaces submission done at once while other lanes hold tickets: its own lane only, and the turn of the lanes stays)
    const int nlanes = ctx->only_lane >= 0 ? 1 : ctx->nlanes;
    for (size_t q = 0; q < jobs.size(); q++) {
        const int use_lane = ctx->only_lane >= 0 ? ctx->only_lane : ctx->next_lane;
        if ((int)flying.size() == nlanes) {
            rc = land_job(ctx, jobs[flying.front()], im, o);
            flying.erase(flying.begin());
            if (rc) return drain(rc);
        }
        MixJob &j = jobs[q];
        if (!j.wide && !j.wide_mixed && ctx->two_pass) {  // (the mixed kernels are single-pass: a context on the two-pass kernels takes the uniform path,
                                         // blocking, once every lane is idle)
            while (!flying.empty()) {
                rc = land_job(ctx, jobs[flying.front()], im, o);
                flying.erase(flying.begin());
                if (rc) return drain(rc);
            }
            if ((rc = redo_by_shape(ctx, ctx->lanes[use_lane], im, j.idx, o)) != 0) return rc;
            continue;
        }
        j.lane = use_lane;
        Lane &l = ctx->lanes[j.lane];
        if (ctx->only_lane < 0) ctx->next_lane = (ctx->next_lane + 1) % ctx->nlanes;
        if (j.wide) {
            const MixImage &f = im[j.idx[0]];
            uint8_t *in = (uint8_t *)ctx->mix_in.p + j.in_off;
            if ((rc = wait_ready(ctx, l.stream)) != 0) return drain(rc);
            for (size_t k = 0; k < j.idx.size(); k++)  // (a view is gathered by a kernel instead of copied)
                if ((rc = stage_frame(ctx, l.stream, in + k * f.frame_bytes, im[j.idx[k]])) != 0) return drain(rc);
            rc = launch_sub_batch(ctx, l, 0, j.idx.size(), in, f.w, f.h, f.color, f.depth, (uint8_t *)ctx->mix_stage.p + j.stage_off, j.slot, nslices, true);
        } else if (j.wide_mixed) {
            rc = launch_mixed_wide(ctx, l, im, j.idx, o, (uint8_t *)ctx->mix_in.p + j.in_off, nslices);
        } else {
            rc = launch_mixed(ctx, l, im, j.idx, o, nslices);
        }
        if (rc) {
            (void)sync_lane(ctx, l);
            return drain(rc);
        }
        flying.push_back(q);
    }
    while (!flying.empty()) {
        rc = land_job(ctx, jobs[flying.front()], im, o);
        flying.erase(flying.begin());
        if (rc) return drain(rc);
    }
    return FELICS_OK;
}

// felics_compress_images_device without the argument checks: slots as encode_device sizes them if d_out holds them, else (or if
// a stream outgrew its slot) a second run with every stream placed exactly, back to back.
int images_device(felics_ctx *ctx, const std::vector<MixImage> &im, uint8_t *d_out, size_t d_out_cap, uint64_t *offsets, uint64_t *lens,
                  Index16Place *ix = nullptr) {
    const size_t n = im.size();
    std::vector<uint64_t> off(n), slot(n);
    uint64_t total = 0;
    for (size_t i = 0; i < n; i++) {
        slot[i] = default_slot(im[i].frame_bytes);
        off[i] = total;
        total += slot[i];
    }
    MixOut o{d_out, off.data(), slot.data(), lens, false};
    o.ix = ix;
    int rc;
    if (total > d_out_cap) {  // the sizes first, into a buffer of the library's own
        if ((rc = reserve(ctx, ctx->mix_out, (size_t)total + 64)) != 0) return rc;
        o.base = (uint8_t *)ctx->mix_out.p;
        o.want_index = false;  // (the run below places the streams and writes the indexes that remain)
    }
    if ((rc = run_images(ctx, im, o)) != 0) return rc;
    if (o.base == d_out && !o.overflow) {
        for (size_t i = 0; i < n; i++) offsets[i] = off[i];
        return FELICS_OK;
    }
    uint64_t need = 0;
    for (size_t i = 0; i < n; i++) {
        off[i] = need;
        slot[i] = (lens[i] + 15) & ~15ull;
        need += slot[i];
    }
    if (need > d_out_cap) {
        if (n) lens[0] = need;
        return FELICS_E_BUFFER_TOO_SMALL;
    }
    o = MixOut{d_out, off.data(), slot.data(), lens, false};
    o.ix = ix;
    if (ix) {  // (what the run above placed is written again: the placement starts from 0, the outputs as the entry point left them)
        ix->begin_run();
        for (size_t i = 0; i < n; i++) ix->idx_offsets[i] = ix->idx_lens[i] = 0;
    }
    if ((rc = run_images(ctx, im, o)) != 0) return rc;
    if (o.overflow) {
        ctx->err = "internal error: a stream outgrew the exact size it had before";
        return FELICS_E_HIP;
    }
    for (size_t i = 0; i < n; i++) offsets[i] = off[i];
    return FELICS_OK;
}

}  // namespace

// The caller's ready event in front of a stream's first access to a view or to the output (felics_compress_views_device).
int wait_ready(felics_ctx *ctx, hipStream_t s) {
    if (ctx->view_ready) HIP_TRY(ctx, hipStreamWaitEvent(s, ctx->view_ready, 0));
    return FELICS_OK;
}

// A view's checks (felics_view_extent and felics_compress_views_device alike) and the hull of its samples' bytes relative to data.
int check_view(const felics_view &v, int64_t &lo, int64_t &hi, bool encode_limits) {
    lo = hi = 0;
    const int rc = view_args_check(v);  // (felics_viewcheck.h: the host model of the indexed views call makes the same checks)
    if (rc) return rc;
    const uint64_t npix = (uint64_t)v.width * v.height;
    const uint32_t planes = v.color == FELICS_COLOR_RGB ? 3 : 1;
    if (encode_limits && npix * planes >= 0xE0000000ull) return FELICS_E_UNSUPPORTED;
    if (encode_limits && v.depth == FELICS_DEPTH_16 && npix > WIDE_MAX_PLANE_PIXELS) return FELICS_E_UNSUPPORTED;
    return view_hull(v, lo, hi);
}

// (ask: felics_compress_views_device_indexed -- view i's index at d_index + offsets[i], segment_pixels[i] pixels per segment, 0: none)
struct IndexAsk {
    uint8_t *d_index;
    const uint64_t *offsets;
    const uint32_t *segment_pixels;
    // felics_compress_views_device_indexed16: the segments name version-2 indexes of the 16-bit views instead, placed by the library
    Index16Place *wide = nullptr;
};
int views_device(felics_ctx *ctx, size_t n, const felics_view *views, void *ready_event, void *d_out, size_t d_out_cap, uint64_t *offsets,
                 uint64_t *lens, felics_view_stats &counted, const IndexAsk *ask = nullptr);

// felics_surfaces_extent: the view's checks on frame 0, the frame axis, and the hull of all frames' sample bytes relative to frame0.data.
int check_surfaces(const felics_surfaces &s, int64_t &lo, int64_t &hi) {
    int rc = check_view(s.frame0, lo, hi);
    if (rc) return rc;
    if (s.frame0.depth == FELICS_DEPTH_16 && (s.frame_stride & 1)) return FELICS_E_INVALID_ARGUMENT;
    if (!s.count || !s.frame0.width || !s.frame0.height) {
        lo = hi = 0;
        return FELICS_OK;
    }
    const __int128 span = (__int128)(s.count - 1) * s.frame_stride;
    const __int128 l = (__int128)lo + (span < 0 ? span : 0), h = (__int128)hi + (span > 0 ? span : 0);
    lo = hi = 0;
    if (l < INT64_MIN || h > INT64_MAX) return FELICS_E_INVALID_ARGUMENT;
    lo = (int64_t)l;
    hi = (int64_t)h;
    return FELICS_OK;
}

// A queued surfaces ticket has come back (felics_wait_batch; the lane's sizes are on the host): land_job's body for its one mixed
// sub-batch, judged by the mode it was launched with.  A sub-batch that is not to be used is redone from gathered frames
// (redo_by_shape on this lane alone: other lanes may hold tickets); after a slot overflow the streams are placed exactly in d_out.
int land_surfaces(felics_ctx *ctx, Lane &l, uint64_t *offsets, uint64_t *lens) {
    const size_t n = l.p_n;
    const std::vector<MixImage> &im = l.s_im;
    const bool wide = im[0].depth == FELICS_DEPTH_16;
    std::vector<size_t> idx(n);
    for (size_t i = 0; i < n; i++) idx[i] = i;
    MixOut o{l.p_out, l.s_off.data(), l.s_slot.data(), lens, false};
    SlotOutcome so = wide ? SlotOutcome{} : decode_status(ctx, l, l.h_sizes[n]);  // (run_wide copies the sizes and nothing else)
    for (size_t k = 0; k < n; k++) {
        lens[k] = l.h_sizes[k];
        if (lens[k] > l.s_slot[k]) so.overflow = true;
    }
    int rc;
    if (!so.redo() && !so.overflow && !so.spine_error) {
        if (wide && ctx->profiling && (rc = sync_lane(ctx, l)) != 0) return rc;
        collect_timing(ctx, l);
        for (size_t k = 0; k < n; k++) offsets[k] = l.s_off[k];
        return FELICS_OK;
    }
    if ((rc = sync_lane(ctx, l)) != 0) return rc;
    if ((rc = apply_remedy(ctx, l, so)) != 0) return rc;
    ctx->staged_bytes = &ctx->sstats.bytes_staged;
    auto leave = [&](int r) {
        ctx->staged_bytes = nullptr;
        return r;
    };
    if (so.redo()) {  // nothing of the sub-batch is to be used, its sizes included: into the slots once more
        if ((rc = redo_by_shape(ctx, l, im, idx, o)) != 0) return leave(rc);
        if (!o.overflow) {
            for (size_t k = 0; k < n; k++) offsets[k] = l.s_off[k];
            return leave(FELICS_OK);
        }
    }
    // a stream outgrew its slot (lens holds every stream's size): exact placement, back to back
    std::vector<uint64_t> off(n), slot(n);
    uint64_t need = 0;
    for (size_t k = 0; k < n; k++) {
        off[k] = need;
        slot[k] = (lens[k] + 15) & ~15ull;
        need += slot[k];
    }
    if (need > l.p_cap) {
        lens[0] = need;
        return leave(FELICS_E_BUFFER_TOO_SMALL);
    }
    MixOut exact{l.p_out, off.data(), slot.data(), lens, false};
    if ((rc = redo_by_shape(ctx, l, im, idx, exact)) != 0) return leave(rc);
    if (exact.overflow) {
        ctx->err = "internal error: a stream outgrew the exact size it had before";
        return leave(FELICS_E_HIP);
    }
    for (size_t k = 0; k < n; k++) offsets[k] = off[k];
    return leave(FELICS_OK);
}

// felics_submit_surfaces_device behind its checks (the next lane is free).
static int submit_surfaces(felics_ctx *ctx, const felics_surfaces &s, void *ready_event, void *d_out, size_t d_out_cap, int *ticket) {
    const felics_view &v = s.frame0;
    const size_t n = (size_t)s.count;
    const int L = ctx->next_lane;
    Lane &l = ctx->lanes[L];
    const MixImage m0 = mix_image(felics_image{v.data, v.width, v.height, v.color, v.depth});
    const bool wide = v.depth == FELICS_DEPTH_16, rgb = v.color == FELICS_COLOR_RGB;
    const int64_t bytes = wide ? 2 : 1;
    const bool dense_frame = v.pixel_stride == bytes * (rgb ? 3 : 1) && v.row_stride == (int64_t)v.width * v.pixel_stride && (!rgb || v.channel_stride == bytes);
    int rc;
    if (m0.npix && dense_frame && (n == 1 || s.frame_stride == (int64_t)m0.frame_bytes)) {
        // the layout of felics_submit_batch_device: that call's path as it is, the event in front of its first kernel
        ctx->wait_before_submit = (hipEvent_t)ready_event;
        rc = felics_submit_batch_device(ctx, n, v.data, v.width, v.height, v.color, v.depth, d_out, d_out_cap, ticket);
        ctx->wait_before_submit = nullptr;
        if (rc) return rc;
        ctx->sstats.submissions++;
        (l.finished ? ctx->sstats.immediate : ctx->sstats.queued)++;
        ctx->sstats.frames_in_place += n;
        return FELICS_OK;
    }
    const bool readable = m0.npix && (rgb || (v.pixel_stride == bytes && v.row_stride >= bytes * (int64_t)v.width));
    const uint64_t slot = default_slot(m0.frame_bytes);
    const size_t per = std::min(MIX_MAX_IMAGES, max_images_per_pass((uint64_t)sort_tiles_of(m0.npix) * SORT_TILE, m0.planes, v.depth));
    l.p_n = n;
    l.p_out = (uint8_t *)d_out;
    l.p_cap = d_out_cap;
    l.finished = false;
    l.p_surfaces = false;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (readable && n <= per && n <= d_out_cap / slot && !ctx->two_pass) {
        l.s_im.assign(n, m0);
        l.s_off.resize(n);
        l.s_slot.assign(n, slot);
        std::vector<size_t> idx(n);
        for (size_t i = 0; i < n; i++) {
            MixImage &m = l.s_im[i];
            m.px = (const uint8_t *)v.data + (int64_t)i * s.frame_stride;
            m.view = true;
            m.vr = ViewRow{m.px, v.row_stride, v.pixel_stride, rgb ? v.channel_stride : 0};
            m.pitch = rgb ? 0 : (uint64_t)v.row_stride;  // (bytes)
            m.wide_in_place = wide;
            l.s_off[i] = i * slot;
            idx[i] = i;
        }
        const MixOut o{l.p_out, l.s_off.data(), l.s_slot.data(), nullptr, false};
        ctx->view_ready = (hipEvent_t)ready_event;  // (around the launch only)
        rc = wide ? launch_mixed_wide(ctx, l, l.s_im, idx, o, nullptr, ctx->slices_queued) : launch_mixed(ctx, l, l.s_im, idx, o, ctx->slices_queued);
        ctx->view_ready = nullptr;
        if (rc) {
            (void)sync_lane(ctx, l);
            return rc;
        }
        l.p_surfaces = true;
        ctx->sstats.queued++;
        ctx->sstats.frames_in_place += n;
    } else {
        // not the queued case: the n views through the views call's path now, on this lane alone, handed over at the wait
        std::vector<felics_view> views(n, v);
        for (size_t i = 0; i < n; i++) views[i].data = (const uint8_t *)v.data + (int64_t)i * s.frame_stride;
        l.r_off.assign(n, 0);
        l.r_len.assign(n, 0);
        felics_view_stats add = {};
        ctx->staged_bytes = &ctx->sstats.bytes_staged;
        ctx->only_lane = L;
        l.r_rc = views_device(ctx, n, views.data(), ready_event, d_out, d_out_cap, l.r_off.data(), l.r_len.data(), add);
        ctx->staged_bytes = nullptr;
        ctx->only_lane = -1;
        l.finished = true;
        ctx->sstats.immediate++;
        ctx->sstats.frames_in_place += add.in_place + add.dense;
        ctx->sstats.frames_gathered += add.gathered;
    }
    ctx->sstats.submissions++;
    l.pending = true;
    *ticket = L;
    ctx->next_lane = (L + 1) % ctx->nlanes;
    return FELICS_OK;
}

}  // namespace felics

extern "C" {

int felics_surfaces_extent(const felics_surfaces *s, int64_t *lo, int64_t *hi) {
    if (!s || !lo || !hi) return FELICS_E_INVALID_ARGUMENT;
    return check_surfaces(*s, *lo, *hi);
}

int felics_get_surface_stats(const felics_ctx *ctx, felics_surface_stats *out, size_t out_size) {
    return copy_stats(ctx, &felics_ctx::sstats, out, out_size);
}

constexpr uint64_t SURFACES_MAX_COUNT = 1ull << 24;  // frames of one descriptor (the host keeps a row per frame)

int felics_submit_surfaces_device(felics_ctx *ctx, const felics_surfaces *s, void *ready_event, void *d_out, size_t d_out_cap, int *ticket) {
    if (!ctx || !s || !ticket || !d_out) return FELICS_E_INVALID_ARGUMENT;
    if (ctx->failed) return FELICS_E_HIP;
    int64_t lo, hi;
    int rc = check_surfaces(*s, lo, hi);
    if (rc) return rc;
    if (s->count == 0) return FELICS_E_INVALID_ARGUMENT;
    if (s->count > SURFACES_MAX_COUNT) return FELICS_E_UNSUPPORTED;
    if (ctx->lanes[ctx->next_lane].pending) return FELICS_E_INVALID_ARGUMENT;  // every lane holds a ticket: wait for the oldest
    return submit_surfaces(ctx, *s, ready_event, d_out, d_out_cap, ticket);
}

int felics_compress_surfaces_device(felics_ctx *ctx, const felics_surfaces *s, void *ready_event, void *d_out, size_t d_out_cap,
                                    uint64_t *offsets, uint64_t *lens) {
    if (!ctx || !s || (s->count && (!d_out || !offsets || !lens))) return FELICS_E_INVALID_ARGUMENT;
    if (ctx->failed) return FELICS_E_HIP;
    int64_t lo, hi;
    int rc = check_surfaces(*s, lo, hi);
    if (rc) return rc;
    if (s->count == 0) return FELICS_OK;
    if (s->count > SURFACES_MAX_COUNT) return FELICS_E_UNSUPPORTED;
    if (any_pending(ctx)) return FELICS_E_INVALID_ARGUMENT;  // felics_wait_batch first
    int ticket = -1;
    if ((rc = submit_surfaces(ctx, *s, ready_event, d_out, d_out_cap, &ticket)) != 0) return rc;
    return felics_wait_batch(ctx, ticket, offsets, lens);
}

int felics_compress_images_device(felics_ctx *ctx, size_t n, const felics_image *images, void *d_out, size_t d_out_cap, uint64_t *offsets,
                                  uint64_t *lens) {
    if (!ctx || (n && (!images || !d_out || !offsets || !lens))) return FELICS_E_INVALID_ARGUMENT;
    if (ctx->failed) return FELICS_E_HIP;
    int rc = check_images(n, images);
    if (rc) return rc;
    if (n == 0) return FELICS_OK;
    if (any_pending(ctx)) return FELICS_E_INVALID_ARGUMENT;  // felics_wait_batch first
    std::vector<MixImage> im(n);
    for (size_t i = 0; i < n; i++) im[i] = mix_image(images[i]);
    return images_device(ctx, im, (uint8_t *)d_out, d_out_cap, offsets, lens);
}

int felics_view_extent(const felics_view *v, int64_t *lo, int64_t *hi) {
    if (!v || !lo || !hi) return FELICS_E_INVALID_ARGUMENT;
    return check_view(*v, *lo, *hi);
}

int felics_get_view_stats(const felics_ctx *ctx, felics_view_stats *out, size_t out_size) {
    return copy_stats(ctx, &felics_ctx::vstats, out, out_size);
}

int felics_compress_views_device(felics_ctx *ctx, size_t n, const felics_view *views, void *ready_event, void *d_out, size_t d_out_cap,
                                 uint64_t *offsets, uint64_t *lens) {
    if (!ctx || (n && (!views || !d_out || !offsets || !lens))) return FELICS_E_INVALID_ARGUMENT;
    if (ctx->failed) return FELICS_E_HIP;
    for (size_t i = 0; i < n; i++) {  // every view checked before anything is launched: the first error in view order
        int64_t lo, hi;
        int rc = check_view(views[i], lo, hi);
        if (rc) return rc;
    }
    if (n == 0) return FELICS_OK;
    if (any_pending(ctx)) return FELICS_E_INVALID_ARGUMENT;  // felics_wait_batch first
    felics_view_stats add = {};
    const int rc = views_device(ctx, n, views, ready_event, d_out, d_out_cap, offsets, lens, add);
    ctx->vstats.views += add.views;  // (bytes_staged: stage_frame has counted)
    ctx->vstats.dense += add.dense;
    ctx->vstats.in_place += add.in_place;
    ctx->vstats.gathered += add.gathered;
    return rc;
}

// A view's segment by felics_index_plan's rules (the view has passed check_view): the size of its index, 0 for segment 0.
static int index_ask_check(const felics_view &v, uint32_t seg, uint64_t &bytes) {
    bytes = 0;
    if (seg == 0) return FELICS_OK;
    if (!index_segment_ok(seg)) return FELICS_E_INVALID_ARGUMENT;
    if (v.depth != FELICS_DEPTH_8) return FELICS_E_UNSUPPORTED;  // 16-bit streams have no index
    bytes = index_layout(v.width, v.height, (uint32_t)v.color, seg).total;
    return FELICS_OK;
}

int felics_index_plan(size_t n, const felics_view *views, const uint32_t *segment_pixels, uint64_t *idx_offsets, uint64_t *idx_lens,
                      uint64_t *total) {
    if (!total || (n && (!views || !segment_pixels || !idx_offsets || !idx_lens))) return FELICS_E_INVALID_ARGUMENT;
    *total = 0;
    uint64_t at = 0;
    for (size_t i = 0; i < n; i++) {
        int64_t lo, hi;
        int rc = check_view(views[i], lo, hi);
        if (rc) return rc;
        if ((rc = index_ask_check(views[i], segment_pixels[i], idx_lens[i])) != 0) return rc;
        idx_offsets[i] = at;
        at += (idx_lens[i] + 15) & ~15ull;
    }
    *total = at;
    return FELICS_OK;
}

int felics_get_index_emit_stats(const felics_ctx *ctx, felics_index_emit_stats *out, size_t out_size) {
    return copy_stats(ctx, &felics_ctx::iestats, out, out_size);
}

int felics_compress_views_device_indexed(felics_ctx *ctx, size_t n, const felics_view *views, const uint32_t *segment_pixels,
                                         void *ready_event, void *d_out, size_t d_out_cap, void *d_index, size_t d_index_cap,
                                         const uint64_t *idx_offsets, uint64_t *offsets, uint64_t *lens) {
    if (!ctx || (n && (!views || !segment_pixels || !idx_offsets || !d_out || !offsets || !lens))) return FELICS_E_INVALID_ARGUMENT;
    if (ctx->failed) return FELICS_E_HIP;
    std::vector<std::pair<uint64_t, uint64_t>> ranges;  // the indexes asked for: offset, bytes
    for (size_t i = 0; i < n; i++) {  // every view and its segment checked before anything is launched: the first error in view order
        int64_t lo, hi;
        uint64_t bytes;
        int rc = check_view(views[i], lo, hi);
        if (rc) return rc;
        if ((rc = index_ask_check(views[i], segment_pixels[i], bytes)) != 0) return rc;
        if (bytes) ranges.emplace_back(idx_offsets[i], bytes);
    }
    if (!ranges.empty() && !d_index) return FELICS_E_INVALID_ARGUMENT;
    for (const auto &r : ranges)  // (the writers store aligned words)
        if (((uintptr_t)d_index + r.first) & 15u) return FELICS_E_INVALID_ARGUMENT;
    for (const auto &r : ranges)
        if (r.first > d_index_cap || r.second > d_index_cap - r.first) return FELICS_E_BUFFER_TOO_SMALL;
    std::sort(ranges.begin(), ranges.end());
    for (size_t k = 1; k < ranges.size(); k++)
        if (ranges[k - 1].first + ranges[k - 1].second > ranges[k].first) return FELICS_E_INVALID_ARGUMENT;
    if (n == 0) return FELICS_OK;
    if (any_pending(ctx)) return FELICS_E_INVALID_ARGUMENT;  // felics_wait_batch first
    felics_view_stats add = {};
    const IndexAsk ask{(uint8_t *)d_index, idx_offsets, segment_pixels};
    const int rc = views_device(ctx, n, views, ready_event, d_out, d_out_cap, offsets, lens, add, &ask);
    ctx->vstats.views += add.views;  // (bytes_staged: stage_frame has counted)
    ctx->vstats.dense += add.dense;
    ctx->vstats.in_place += add.in_place;
    ctx->vstats.gathered += add.gathered;
    return rc;
}

int felics_get_index_view_wide_emit_stats(const felics_ctx *ctx, felics_index16_view_emit_stats *out, size_t out_size) {
    return copy_stats(ctx, &felics_ctx::i16vestats, out, out_size);
}

int felics_compress_views_device_indexed_wide(felics_ctx *ctx, size_t n, const felics_view *views, const uint32_t *segment_pixels,
                                              void *ready_event, void *d_out, size_t d_out_cap, void *d_index, size_t d_index_cap,
                                              uint64_t *offsets, uint64_t *lens, uint64_t *idx_offsets, uint64_t *idx_lens, uint64_t *idx_total) {
    if (!ctx || (n && (!views || !segment_pixels || !d_out || !offsets || !lens || !idx_offsets || !idx_lens))) return FELICS_E_INVALID_ARGUMENT;
    if (ctx->failed) return FELICS_E_HIP;
    if (idx_total) *idx_total = 0;
    bool asked = false;
    for (size_t i = 0; i < n; i++) {  // every view and its segment checked before anything is launched: the first error in view order
        int64_t lo, hi;
        const int rc = check_view(views[i], lo, hi);
        if (rc) return rc;
        if (segment_pixels[i] == 0) continue;
        if (!index_segment_ok(segment_pixels[i])) return FELICS_E_INVALID_ARGUMENT;
        if (views[i].depth != FELICS_DEPTH_16) return FELICS_E_UNSUPPORTED;  // (its call is felics_compress_views_device_indexed)
        asked = true;
    }
    if (asked && (!d_index || ((uintptr_t)d_index & 63u))) return FELICS_E_INVALID_ARGUMENT;
    if (n == 0) return FELICS_OK;
    if (any_pending(ctx)) return FELICS_E_INVALID_ARGUMENT;  // felics_wait_batch first
    Index16Place ix{(uint8_t *)d_index, asked ? (uint64_t)d_index_cap : 0, idx_offsets, idx_lens, 0, 0};
    if (asked) {
        // the workspace per checkpoint bounds a sub-batch within the batch call's budget: a quarter of the free device memory and what
        // this context holds for it already; an image whose own checkpoints do not fit is refused
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        size_t free_b = 0, total_b = 0;
        HIP_TRY(ctx, hipMemGetInfo(&free_b, &total_b));
        ix.budget = free_b / 4;
        for (const Lane &l : ctx->lanes) ix.budget += l.i16_bitmap.cap + l.i16_prefix.cap;
        for (size_t i = 0; i < n; i++) {
            if (!segment_pixels[i]) continue;
            const felics_view &v = views[i];
            const uint64_t planes = v.color == FELICS_COLOR_RGB ? 3 : 1;
            const uint64_t K = index16_layout(v.width, v.height, (uint32_t)v.color, segment_pixels[i]).K;
            if (planes * K * index16_cp_bytes(v.color) + 24u > ix.budget) return FELICS_E_UNSUPPORTED;
        }
        if (const char *e = getenv("FELICS_TEST_INDEX16_EMIT_CPS")) ix.test_cps = (uint64_t)std::max(1, atoi(e));  // tests: several sub-batches
    }
    for (size_t i = 0; i < n; i++) idx_offsets[i] = idx_lens[i] = 0;
    felics_view_stats add = {};
    const IndexAsk ask{nullptr, nullptr, segment_pixels, &ix};
    const int rc = views_device(ctx, n, views, ready_event, d_out, d_out_cap, offsets, lens, add, &ask);
    ctx->vstats.views += add.views;  // (bytes_staged: stage_frame has counted)
    ctx->vstats.dense += add.dense;
    ctx->vstats.in_place += add.in_place;
    ctx->vstats.gathered += add.gathered;
    if (rc) return rc;  // (an error of the stream part: *idx_total stays 0)
    if (idx_total) *idx_total = ix.total;
    felics_index16_view_emit_stats &st = ctx->i16vestats;
    st.views += n;
    st.indexes += ix.indexes;
    st.rows_written += ix.rows;
    st.index_bytes += ix.bytes;
    st.sub_batches += ix.sub_batches;
    st.shapes_max = ix.shapes_max;
    st.redone += ix.redone;
    return ix.too_small ? FELICS_E_BUFFER_TOO_SMALL : FELICS_OK;
}

}  // extern "C"

namespace felics {

// felics_compress_views_device behind its checks; `add` = the classes of the views (counted once the gathering has succeeded).  Also
// the immediate case of felics_submit_surfaces_device (ctx->only_lane: the one lane it may use).
int views_device(felics_ctx *ctx, size_t n, const felics_view *views, void *ready_event, void *d_out, size_t d_out_cap, uint64_t *offsets,
                 uint64_t *lens, felics_view_stats &counted, const IndexAsk *ask) {
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    // the class of every view: dense, read in place, or gathered (gray8 now, into view_stage; 16-bit where its group is queued)
    std::vector<MixImage> im(n);
    std::vector<size_t> stage_at(n, 0);
    size_t stage_total = 0;
    felics_view_stats add = {};
    for (size_t i = 0; i < n; i++) {
        const felics_view &v = views[i];
        MixImage &m = im[i];
        m = mix_image(felics_image{v.data, v.width, v.height, v.color, v.depth});
        if (ask && ask->segment_pixels[i]) {
            if (ask->wide) m.index16 = true;
            else m.index = ask->d_index + ask->offsets[i];
            m.segment_pixels = ask->segment_pixels[i];
        }
        const int64_t bytes = v.depth == FELICS_DEPTH_16 ? 2 : 1;
        const bool rgb = v.color == FELICS_COLOR_RGB;
        add.views++;
        const bool dense = !m.npix || (v.pixel_stride == bytes * (rgb ? 3 : 1) && v.row_stride == (int64_t)v.width * v.pixel_stride &&
                                       (!rgb || v.channel_stride == bytes));
        if (dense) {
            add.dense++;
            continue;
        }
        m.view = true;
        m.vr = ViewRow{v.data, v.row_stride, v.pixel_stride, rgb ? v.channel_stride : 0};
        if (v.depth == FELICS_DEPTH_8 && rgb) {
            add.in_place++;
        } else if (v.depth == FELICS_DEPTH_8 && v.pixel_stride == 1 && v.row_stride >= (int64_t)v.width) {
            add.in_place++;
            m.pitch = (uint64_t)v.row_stride;
        } else {
            add.gathered++;
            if (v.depth == FELICS_DEPTH_8) {
                stage_at[i] = stage_total;
                stage_total += (m.frame_bytes + 255) & ~(size_t)255;
            }
        }
    }
    int rc;
    ctx->view_ready = (hipEvent_t)ready_event;
    ctx->wait_before_submit = (hipEvent_t)ready_event;  // (the uniform path's sub-batches: launch_sub_batch)
    auto leave = [&](int r) {
        ctx->view_ready = nullptr;
        ctx->wait_before_submit = nullptr;
        return r;
    };
    if (stage_total) {
        Lane &l = ctx->lanes[std::max(0, ctx->only_lane)];
        if ((rc = reserve(ctx, ctx->view_stage, stage_total + 64)) != 0) return leave(rc);
        if ((rc = wait_ready(ctx, l.stream)) != 0) return leave(rc);
        for (size_t i = 0; i < n; i++) {
            MixImage &m = im[i];
            if (!m.view || m.depth != FELICS_DEPTH_8 || m.planes == 3 || m.pitch) continue;
            uint8_t *dst = (uint8_t *)ctx->view_stage.p + stage_at[i];
            if ((rc = stage_frame(ctx, l.stream, dst, m)) != 0) return leave(rc);
            m.px = dst;
            m.view = false;
        }
        if (hipStreamSynchronize(l.stream) != hipSuccess) return leave(hip_fail(ctx, hipGetLastError(), "gathering views"));
    }
    counted = add;
    return leave(images_device(ctx, im, (uint8_t *)d_out, d_out_cap, offsets, lens, ask ? ask->wide : nullptr));
}

}  // namespace felics

extern "C" {

// Host frames in, host streams out: the frames are copied to the device (16-byte aligned, back to back), encoded as above into the
// context's own buffer, and every stream that fits its caller's buffer is copied back.
int felics_compress_images(felics_ctx *ctx, size_t n, const felics_image *images, uint8_t *const *outs, const size_t *caps, size_t *lens) {
    if (!ctx || (n && (!images || !outs || !caps || !lens))) return FELICS_E_INVALID_ARGUMENT;
    if (ctx->failed) return FELICS_E_HIP;
    int rc = check_images(n, images);
    if (rc) return rc;
    if (n == 0) return FELICS_OK;
    if (any_pending(ctx)) return FELICS_E_INVALID_ARGUMENT;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (!ctx->copy_in) {
        HIP_TRY(ctx, hipStreamCreateWithFlags(&ctx->copy_in, hipStreamNonBlocking));
        HIP_TRY(ctx, hipStreamCreateWithFlags(&ctx->copy_out, hipStreamNonBlocking));
    }
    std::vector<MixImage> im(n);
    std::vector<size_t> at(n);
    size_t in_total = 0;
    uint64_t out_total = 64;
    for (size_t i = 0; i < n; i++) {
        im[i] = mix_image(images[i]);
        at[i] = in_total;
        in_total += (im[i].frame_bytes + 15) & ~(size_t)15;
        out_total += default_slot(im[i].frame_bytes);
    }
    if ((rc = reserve(ctx, ctx->in, in_total + 64)) != 0) return rc;
    if ((rc = reserve(ctx, ctx->out, (size_t)out_total)) != 0) return rc;
    for (size_t i = 0; i < n; i++) {
        uint8_t *dst = (uint8_t *)ctx->in.p + at[i];
        if (im[i].frame_bytes) HIP_TRY(ctx, hipMemcpyAsync(dst, images[i].pixels, im[i].frame_bytes, hipMemcpyHostToDevice, ctx->copy_in));
        im[i].px = dst;
    }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->copy_in));
    std::vector<uint64_t> offs(n), sizes(n);
    rc = images_device(ctx, im, (uint8_t *)ctx->out.p, ctx->out.cap, offs.data(), sizes.data());
    if (rc == FELICS_E_BUFFER_TOO_SMALL) {  // a stream outgrew its slot and the slots' room: exact placement in a larger buffer
        if ((rc = reserve(ctx, ctx->out, (size_t)sizes[0] + 64)) != 0) return rc;
        rc = images_device(ctx, im, (uint8_t *)ctx->out.p, ctx->out.cap, offs.data(), sizes.data());
    }
    if (rc) return rc;
    int result = FELICS_OK;
    for (size_t i = 0; i < n; i++) {
        lens[i] = (size_t)sizes[i];
        if (sizes[i] > caps[i] || !outs[i]) {
            result = FELICS_E_BUFFER_TOO_SMALL;  // lens[] reports every size needed; nothing is written to this buffer
            continue;
        }
        HIP_TRY(ctx, hipMemcpyAsync(outs[i], (const uint8_t *)ctx->out.p + offs[i], (size_t)sizes[i], hipMemcpyDeviceToHost, ctx->copy_out));
    }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->copy_out));
    return result;
}

}  // extern "C"
