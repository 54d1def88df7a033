// felics_context.cpp -- the context of libfelics and its plumbing: HIP error handling, waits, the grow-only buffers, stage
// timing, and the entry points that only read or describe a context.
#include "felics_host.h"

namespace felics {

const char *const kStageNames[ST_COUNT] = {"planes", "hist", "offsets", "scatter", "spine", "assign", "lengths", "bitscan", "zero", "pack",
                                     "wide_keys", "wide_sort", "wide_chains"};

int lanes_from_env() {
    if (const char *e = getenv("FELICS_LANES")) return std::max(1, std::min(atoi(e), MAX_LANES));
    return DEFAULT_LANES;
}

int hip_fail(felics_ctx *ctx, hipError_t e, const char *what) {
    char buf[256];
    snprintf(buf, sizeof buf, "%s: %s", what, hipGetErrorString(e));
    if (ctx) ctx->err = buf;
    return FELICS_E_HIP;
}

// Wait for an event, but not forever: a kernel that does not return must surface as an error
// (FELICS_E_HIP, "timed out"), not as a caller that hangs.
int wait_event(felics_ctx *ctx, hipEvent_t ev, const char *what) {
    const auto t0 = std::chrono::steady_clock::now();
    if (ctx->test_timeout) {  // FELICS_TEST_TIMEOUT=1 (tests): behave as if the GPU did not answer in time
        ctx->err = std::string(what) + ": timed out waiting for the GPU; the context is unusable from here on";
        ctx->failed = true;
        ctx->stats.failed = 1;
        return FELICS_E_HIP;
    }
    for (uint32_t spins = 0;; spins++) {
        const hipError_t e = hipEventQuery(ev);
        if (e == hipSuccess) return FELICS_OK;
        if (e != hipErrorNotReady) return hip_fail(ctx, e, what);
        if (spins > 2000) std::this_thread::sleep_for(std::chrono::microseconds(50));
        if ((spins & 1023) == 1023 &&
            std::chrono::steady_clock::now() - t0 > std::chrono::seconds(ctx->timeout_s)) {
            ctx->err = std::string(what) + ": timed out waiting for the GPU; the context is unusable from here on";
            ctx->failed = true;
            ctx->stats.failed = 1;
            return FELICS_E_HIP;
        }
    }
}

// Waits for everything a lane has queued.  The tail stream is shared by the lanes (the single-pass pack
// kernels of two submissions must not run side by side), so this also waits for the other lane's packs:
// used on the synchronous, fallback and error paths only.
int sync_lane(felics_ctx *ctx, Lane &l) {
    if (l.front) HIP_TRY(ctx, hipStreamSynchronize(l.front));
    if (l.stream) HIP_TRY(ctx, hipStreamSynchronize(l.stream));
    if (l.kstream) HIP_TRY(ctx, hipStreamSynchronize(l.kstream));
    if (l.tail) HIP_TRY(ctx, hipStreamSynchronize(l.tail));
    return FELICS_OK;
}

// Grow-only device buffer.  Callers only grow a lane's buffer while that lane is idle.
int reserve(felics_ctx *ctx, DevBuf &b, size_t bytes) {
    if (bytes <= b.cap) return FELICS_OK;
    if (b.p) {
        HIP_TRY(ctx, hipFree(b.p));  // hipFree waits for the device
        b.p = nullptr;
        b.cap = 0;
    }
    size_t want = bytes + bytes / 8 + 256;  // a little slack so near-equal batches do not realloc
    HIP_TRY(ctx, hipMalloc(&b.p, want));
    b.cap = want;
    return FELICS_OK;
}

// served[] is compared against an epoch: a fresh buffer must not match by accident
int reserve_zeroed(felics_ctx *ctx, DevBuf &b, size_t bytes) {
    if (bytes <= b.cap) return FELICS_OK;
    int rc = reserve(ctx, b, bytes);
    if (rc) return rc;
    HIP_TRY(ctx, hipMemset(b.p, 0, b.cap));
    // (the memset of device memory may return before it has run, and the context's streams are non-blocking: without this wait a
    // kernel could read rows of a grown epoch table -- often the memory of the one just freed, small epochs and all -- before the
    // zeros arrive; seen as FELICS_E_INVALID_VALUE on the last good streams of a 64-stream k_decode16 call)
    HIP_TRY(ctx, hipStreamSynchronize(nullptr));
    return FELICS_OK;
}

static void release(DevBuf &b) {
    if (b.p) (void)hipFree(b.p);
    b.p = nullptr;
    b.cap = 0;
}

// Grow-only page-locked host buffer for `count` items in `bytes` bytes (a lane's sizes, its plane table): as reserve, the lane is idle.
int reserve_pinned(felics_ctx *ctx, void **p, size_t &cap, size_t count, size_t bytes) {
    if (count <= cap) return FELICS_OK;
    if (*p) HIP_TRY(ctx, hipHostFree(*p));
    *p = nullptr;
    HIP_TRY(ctx, hipHostMalloc(p, bytes, hipHostMallocDefault));
    cap = count;
    return FELICS_OK;
}

int check_args(uint32_t w, uint32_t h, int color, int depth) {
    if (color != FELICS_COLOR_GRAY && color != FELICS_COLOR_RGB) return FELICS_E_INVALID_COLOR_TYPE;
    if (depth != FELICS_DEPTH_8 && depth != FELICS_DEPTH_16) return FELICS_E_INVALID_PIXEL_DEPTH;
    // compress_channel unwraps width.checked_mul(height) (compression.rs:86): reported, not a panic
    if ((uint64_t)w * h > 0xFFFFFFFFull) return FELICS_E_INVALID_DIMENSIONS;
    return FELICS_OK;
}

void header_bytes(uint8_t *o, uint32_t w, uint32_t h, int color, int depth) {
    memcpy(o, "FLCS", 4);
    o[4] = (uint8_t)color;
    o[5] = (uint8_t)depth;
    for (int i = 0; i < 4; i++) {
        o[6 + i] = (uint8_t)(w >> (24 - 8 * i));
        o[10 + i] = (uint8_t)(h >> (24 - 8 * i));
    }
}

void collect_timing(felics_ctx *ctx, Lane &l) {
    if (!ctx->profiling) return;
    ctx->span_ms = 0.f;
    (void)hipEventElapsedTime(&ctx->span_ms, l.span_begin, l.span_end);
    for (int i = 0; i < ST_COUNT; i++) {
        ctx->stage_ms[i] = 0.f;  // sum of the launches' durations (launches overlap: the sum can exceed wall time)
        ctx->stage_launches[i] = 0;
        for (int k = 0; k < l.ev_used[i]; k++) {
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, l.ev[i][k][0], l.ev[i][k][1]) == hipSuccess) {
                ctx->stage_ms[i] += ms;
                ctx->stage_launches[i]++;
            }
        }
    }
}

bool any_pending(const felics_ctx *ctx) {
    for (const Lane &l : ctx->lanes)
        if (l.pending) return true;
    return false;
}

}  // namespace felics

extern "C" {

int felics_ctx_create(int device, felics_ctx **out) {
    if (!out) return FELICS_E_INVALID_ARGUMENT;
    *out = nullptr;
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count <= 0 || device < 0 || device >= count) return FELICS_E_HIP;
    felics_ctx *ctx = new (std::nothrow) felics_ctx();
    if (!ctx) return FELICS_E_IO;
    ctx->device = device;
    // Hardware queues: the HIP runtime keeps one pool of them PER STREAM PRIORITY (low, normal, high), each capped by
    // GPU_MAX_HW_QUEUES -- 4 unless the process was started with another value -- and a stream created beyond the cap shares the
    // in-order queue of an earlier one of its priority: its kernels then wait behind kernels they do not depend on (up to round 5
    // five high-priority streams: at the default cap one lane's assign launches stood behind its own next spine launch, +5 % per
    // step).  So the stage graph is cut to fit the default, and no environment variable is needed (profiles/hw_queues.txt):
    //   per lane  : `stream` (spine, high), `front` (front + enum, low), `kstream` (assign, low)
    //   all lanes : one `tail` (pack, high)
    //   two lanes 3 high + 4 low: a queue each.  Three lanes 4 high + 6 low: two pairs of low streams share, and which is the
    //   runtime's choice -- measured no slower than round 5's graph and faster than the sharing the library could choose (the first
    //   lane alone with a k stream, or none).  Four lanes: no `kstream` (the assign launches on the front stream, whose launches they
    //   follow anyway) and the tail at normal priority, since the spines fill the high pool: 4 high + 4 low + 1 normal.
    // The normal pool is otherwise the caller's (torch's streams), plus the host-buffer path's two copy streams.
    ctx->nlanes = lanes_from_env();
    ctx->poison = getenv("FELICS_POISON") != nullptr;
    ctx->two_pass = getenv("FELICS_TWO_PASS") != nullptr;
    ctx->test_lookback = getenv("FELICS_TEST_LOOKBACK_FAIL") != nullptr;
    if (const char *e = getenv("FELICS_SCATTER")) ctx->scatter_ballot = !strcmp(e, "ballot");
    ctx->test_tile_cap = getenv("FELICS_TEST_TILE_CAP") != nullptr;
    ctx->test_scatter_order = getenv("FELICS_TEST_SCATTER_ORDER") != nullptr;
    ctx->pack_tickets = ctx->own_tails = getenv("FELICS_OWN_TAILS") != nullptr;
    ctx->serial = getenv("FELICS_SERIAL") != nullptr;
    ctx->assign_on = ctx->nlanes > 3 ? ASSIGN_FRONT : ASSIGN_OWN;
    if (const char *e = getenv("FELICS_ASSIGN_STREAM")) ctx->assign_on = !strcmp(e, "tail") ? ASSIGN_TAIL : !strcmp(e, "front") ? ASSIGN_FRONT : ASSIGN_OWN;
    ctx->test_timeout = getenv("FELICS_TEST_TIMEOUT") != nullptr;
    // (tests of the epoch wraps, felics_epochs.h: the LAST epoch each counter pretends to have handed out when its buffer is fresh --
    // a lane's look-back status, dec_table, dec_lane16_table -- so that a few calls reach a wrap that is days or thousands of calls away)
    if (const char *e = getenv("FELICS_TEST_LOOKBACK_EPOCH"))
        for (Lane &l : ctx->lanes) l.epoch = (uint32_t)strtoull(e, nullptr, 0);
    if (const char *e = getenv("FELICS_TEST_DECODE16_EPOCH")) ctx->dec_epoch = ctx->dec_epoch_start = (uint32_t)strtoull(e, nullptr, 0);
    if (const char *e = getenv("FELICS_TEST_DECODE16_LANES_EPOCH"))
        ctx->dec_lane16_epoch = ctx->dec_lane16_epoch_start = (uint32_t)std::min<unsigned long long>(strtoull(e, nullptr, 0), DEC16L_EPOCH_MAX);
    if (const char *e = getenv("FELICS_SLICES")) ctx->slices_blocking = std::max(1, std::min(atoi(e), SLICES));
    if (const char *e = getenv("FELICS_SLICES_QUEUED")) ctx->slices_queued = std::max(1, std::min(atoi(e), SLICES));  // (tuning sweeps: profiles/tools/sweep_queue.sh)
    ctx->trace = getenv("FELICS_TRACE") != nullptr;
    ctx->trace_epochs = getenv("FELICS_TRACE_EPOCHS") != nullptr;
    if (const char *e = getenv("FELICS_TIMEOUT_S")) ctx->timeout_s = std::max(1, atoi(e));
    bool ok = hipSetDevice(device) == hipSuccess;
    // Oldest work first: the spine (the one sequential chain) and the tail, which finishes the submission that is
    // furthest along, go before the front (classification and event sort of the submission that has just started).  Measured
    // with two submissions in flight: 4.11 / 4.13 ms per step against 4.24 / 4.19 with the front preferred (round 1's choice)
    // and 4.12 / 4.17 with only the tail preferred; round 5, all eight combinations of high / low for spine, front and tail:
    // 2.53-2.65 ms, the differences inside the run-to-run spread (profiles/r05/experiments.txt); blocking calls do not care.
    int prio_low = 0, prio_high = 0;
    (void)hipDeviceGetStreamPriorityRange(&prio_low, &prio_high);  // numerically: low >= high
    int prio_spine = prio_high, prio_front = prio_low, prio_tail = ctx->nlanes > 3 && !ctx->own_tails ? (prio_low + prio_high) / 2 : prio_high;
    const int prio_assign = prio_low;  // (high up to round 5: the fifth stream of the high pool)
    for (int li = 0; li < ctx->nlanes; li++) {
        Lane &l = ctx->lanes[li];
        ok = ok && hipStreamCreateWithPriority(&l.stream, hipStreamNonBlocking, prio_spine) == hipSuccess;
        ok = ok && hipStreamCreateWithPriority(&l.front, hipStreamNonBlocking, prio_front) == hipSuccess;
        if (ctx->assign_on == ASSIGN_OWN) ok = ok && hipStreamCreateWithPriority(&l.kstream, hipStreamNonBlocking, prio_assign) == hipSuccess;
        // One tail stream for all lanes: the pack kernels of two submissions run one after the other (measured faster:
        // 4.6 vs 4.8 ms per step).  FELICS_OWN_TAILS=1 gives every lane its own; that is safe since the pack kernels hand
        // out their tiles by ticket (launch_pack_t's counter), it just is not faster.
        if (&l == &ctx->lanes[0] || ctx->own_tails)
            ok = ok && hipStreamCreateWithPriority(&l.tail, hipStreamNonBlocking, prio_tail) == hipSuccess;
        else
            l.tail = ctx->lanes[0].tail;
        for (int q = 0; q < SLICES && ok; q++) {
            ok = hipEventCreateWithFlags(&l.slice_done[q], hipEventDisableTiming) == hipSuccess;
            ok = ok && hipEventCreateWithFlags(&l.spine_done[q], hipEventDisableTiming) == hipSuccess;
            ok = ok && hipEventCreateWithFlags(&l.assign_done[q], hipEventDisableTiming) == hipSuccess;
        }
        ok = ok && hipEventCreateWithFlags(&l.sized, hipEventDisableTiming) == hipSuccess;
        ok = ok && hipEventCreate(&l.span_begin) == hipSuccess && hipEventCreate(&l.span_end) == hipSuccess;
        for (int i = 0; i < ST_COUNT && ok; i++)
            for (int k = 0; k < EV_PAIRS && ok; k++)
                for (int j = 0; j < 2 && ok; j++) ok = hipEventCreate(&l.ev[i][k][j]) == hipSuccess;
    }
    if (!ok) {
        felics_ctx_destroy(ctx);
        return FELICS_E_HIP;
    }
    *out = ctx;
    return FELICS_OK;
}

void felics_ctx_destroy(felics_ctx *ctx) {
    if (!ctx) return;
    if (ctx->failed) {  // kernels may still hold the streams and the workspace: leave everything to process exit
        delete ctx;
        return;
    }
    (void)hipSetDevice(ctx->device);
    // everything queued by any lane first (the lanes share the tail stream), then the teardown
    for (Lane &l : ctx->lanes) {
        if (l.front) (void)hipStreamSynchronize(l.front);
        if (l.stream) (void)hipStreamSynchronize(l.stream);
        if (l.kstream) (void)hipStreamSynchronize(l.kstream);
    }
    for (Lane &l : ctx->lanes)
        if (l.tail) (void)hipStreamSynchronize(l.tail);
    for (Lane &l : ctx->lanes) {
        DevBuf *bufs[] = {&l.planes, &l.counts, &l.scalars, &l.evs, &l.pix_of, &l.k_map, &l.k_sorted, &l.tile_slots, &l.desc,
                          &l.block_state, &l.group_bits, &l.tile_bits, &l.tile_bitoff, &l.plane_sums, &l.image_bytes, &l.image_off,
                          &l.partial, &l.status, &l.edge_first, &l.edge_last, &l.pscratch, &l.wrecs[0], &l.wrecs[1], &l.wtile_cnt, &l.wmeta, &l.whist, &l.wdigtot, &l.heads, &l.wlong,
                          &l.i16_bitmap, &l.i16_prefix, &l.i16_nrows, &l.i16_rows_off, &l.i16_totals, &l.i16_index_off, &l.i16_table};
        for (DevBuf *b : bufs) release(*b);
        if (l.h_sizes) (void)hipHostFree(l.h_sizes);
        release(l.mtable);
        if (l.h_table) (void)hipHostFree(l.h_table);
        for (int i = 0; i < ST_COUNT; i++)
            for (int k = 0; k < EV_PAIRS; k++)
                for (int j = 0; j < 2; j++)
                    if (l.ev[i][k][j]) (void)hipEventDestroy(l.ev[i][k][j]);
        if (l.sized) (void)hipEventDestroy(l.sized);
        if (l.span_begin) (void)hipEventDestroy(l.span_begin);
        if (l.span_end) (void)hipEventDestroy(l.span_end);
        for (int q = 0; q < SLICES; q++) {
            if (l.slice_done[q]) (void)hipEventDestroy(l.slice_done[q]);
            if (l.spine_done[q]) (void)hipEventDestroy(l.spine_done[q]);
            if (l.assign_done[q]) (void)hipEventDestroy(l.assign_done[q]);
        }
        if (l.front) (void)hipStreamDestroy(l.front);
        if (l.kstream) (void)hipStreamDestroy(l.kstream);
        if (l.stream) (void)hipStreamDestroy(l.stream);
        if (l.tail && (&l == &ctx->lanes[0] || l.tail != ctx->lanes[0].tail)) (void)hipStreamDestroy(l.tail);
    }
    release(ctx->in);
    if (ctx->copy_in) (void)hipStreamSynchronize(ctx->copy_in), (void)hipStreamDestroy(ctx->copy_in);
    if (ctx->copy_out) (void)hipStreamSynchronize(ctx->copy_out), (void)hipStreamDestroy(ctx->copy_out);
    for (hipEvent_t ev : ctx->h2d_done)
        if (ev) (void)hipEventDestroy(ev);
    release(ctx->out);
    release(ctx->own);
    release(ctx->mix_in);
    release(ctx->mix_stage);
    release(ctx->mix_out);
    release(ctx->mix_redo);
    release(ctx->mix_index);
    release(ctx->view_stage);
    release(ctx->dec_meta);
    release(ctx->dec_seg_status);
    release(ctx->dec_region_work);
    release(ctx->dec_planes);
    release(ctx->dec_planes16);
    release(ctx->dec_table);
    release(ctx->dec_lane_table);
    release(ctx->dec_lane16_table);
    delete ctx;
}

size_t felics_max_compressed_size(uint32_t w, uint32_t h, int color, int depth) {
    const uint64_t planes = color == FELICS_COLOR_RGB ? 3 : 1;
    const uint64_t emax = depth == FELICS_DEPTH_8 ? (color ? 509u : 254u) : (color ? 131069u : 65534u);
    const uint64_t px = (uint64_t)w * h;
    const uint64_t bits = planes * 64u + planes * px * (3u + emax);
    return (size_t)(14u + (bits + 7u) / 8u);
}

int felics_write_header(const felics_header *hdr, uint8_t *out, size_t cap) {
    if (!hdr || !out) return FELICS_E_INVALID_ARGUMENT;
    if (cap < FELICS_HEADER_BYTES) return FELICS_E_BUFFER_TOO_SMALL;
    if (hdr->color_type > 1) return FELICS_E_INVALID_COLOR_TYPE;
    if (hdr->pixel_depth > 1) return FELICS_E_INVALID_PIXEL_DEPTH;
    header_bytes(out, hdr->width, hdr->height, hdr->color_type, hdr->pixel_depth);
    return FELICS_OK;
}

const char *felics_strerror(int code) {
    switch (code) {
        case FELICS_OK: return "ok";
        case FELICS_E_IO: return "I/O error (truncated stream or allocation failure)";
        case FELICS_E_INVALID_VALUE: return "a decoded value does not fit the image bit depth";
        case FELICS_E_VALUE_OVERFLOW: return "arithmetic overflow while decoding";
        case FELICS_E_INVALID_DIMENSIONS: return "invalid channel dimensions";
        case FELICS_E_INVALID_COLOR_TYPE: return "invalid color type";
        case FELICS_E_INVALID_PIXEL_DEPTH: return "invalid pixel depth";
        case FELICS_E_INVALID_SIGNATURE: return "not a felics file (bad signature)";
        case FELICS_E_BUFFER_TOO_SMALL: return "output buffer too small";
        case FELICS_E_HIP: return "no usable HIP device or HIP runtime error";
        case FELICS_E_UNSUPPORTED: return "not supported by the GPU encoder in this build";
        case FELICS_E_INVALID_ARGUMENT: return "invalid argument";
        case FELICS_E_INVALID_INDEX: return "restart index is malformed or does not fit the stream";
        default: return "unknown error";
    }
}

const char *felics_last_error(const felics_ctx *ctx) { return ctx ? ctx->err.c_str() : ""; }

int felics_set_profiling(felics_ctx *ctx, int enabled) {
    if (!ctx) return FELICS_E_INVALID_ARGUMENT;
    ctx->profiling = enabled != 0;
    return FELICS_OK;
}

int felics_get_stats(const felics_ctx *ctx, felics_stats *out) {
    if (!ctx || !out) return FELICS_E_INVALID_ARGUMENT;
    *out = ctx->stats;
    out->two_pass = ctx->two_pass ? 1 : 0;
    out->failed = ctx->failed ? 1 : 0;
    return FELICS_OK;
}

int felics_stage_count(void) { return ST_COUNT; }

int felics_lane_count(void) { return lanes_from_env(); }

int felics_ctx_lane_count(const felics_ctx *ctx) { return ctx ? ctx->nlanes : FELICS_E_INVALID_ARGUMENT; }

int felics_get_stage_launches(const felics_ctx *ctx, int *launches, int cap) {
    if (!ctx || !launches) return FELICS_E_INVALID_ARGUMENT;
    int n = cap < ST_COUNT ? cap : (int)ST_COUNT;
    for (int i = 0; i < n; i++) launches[i] = ctx->stage_launches[i];
    return n;
}

const char *felics_stage_name(int stage) { return stage >= 0 && stage < ST_COUNT ? kStageNames[stage] : ""; }

int felics_get_span_ms(const felics_ctx *ctx, float *ms) {
    if (!ctx || !ms) return FELICS_E_INVALID_ARGUMENT;
    *ms = ctx->span_ms;
    return FELICS_OK;
}

int felics_get_stage_ms(const felics_ctx *ctx, float *ms, int cap) {
    if (!ctx || !ms) return FELICS_E_INVALID_ARGUMENT;
    int n = cap < ST_COUNT ? cap : (int)ST_COUNT;
    for (int i = 0; i < n; i++) ms[i] = ctx->stage_ms[i];
    return n;
}

}  // extern "C"
