// felics_api.cpp -- host side of libfelics: the C ABI of include/felics.h on top of the
// gfx950 kernels.  One context = one GPU + four HIP streams + a grow-only workspace in HBM.
//
// Encode is GPU-only by design: there is no CPU encode path in this library.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <type_traits>
#include <string>
#include <algorithm>
#include <new>
#include <tuple>
#include <vector>

#include "../../include/felics.h"
#include "felics_kernels.h"

using namespace felics;

namespace {

enum Stage { ST_PLANES = 0, ST_HIST, ST_OFFSETS, ST_SCATTER, ST_SPINE, ST_ASSIGN, ST_LENGTHS, ST_BITSCAN, ST_ZERO, ST_PACK,
             ST_WIDE_KEYS, ST_WIDE_SORT, ST_WIDE_CHAINS, ST_COUNT };
const char *kStageNames[ST_COUNT] = {"planes", "hist", "offsets", "scatter", "spine", "assign", "lengths", "bitscan", "zero", "pack",
                                     "wide_keys", "wide_sort", "wide_chains"};
static_assert(ST_COUNT <= FELICS_MAX_STAGES, "felics.h promises at most FELICS_MAX_STAGES stages");

constexpr int SLICES = 12;              // at most; a submission uses lane.nslices of them
constexpr uint64_t PASS_MAX_CHAINS = 1u << 23;  // chains (plane x context) of one 8-bit pass at most: max_images_per_pass
constexpr int EV_PAIRS = SLICES + 2;    // launches of one stage per sub-batch that can be timed
constexpr int MAX_LANES = 4;            // upper bound of the submissions in flight (felics_submit_batch_device), each with streams and workspace of its own
constexpr int DEFAULT_LANES = 2;        // what a context uses unless FELICS_LANES says otherwise (measured round 3: 2 lanes x 4 slices 3.03-3.06 ms per step,
                                        // 3 lanes x 3 slices 2.97-3.16, 4 lanes 3.18-3.47: the kernels are issue-bound, so more of them side by side gain nothing)
enum AssignOn { ASSIGN_OWN, ASSIGN_FRONT, ASSIGN_TAIL };  // the stream k_assign3 is queued on (felics_ctx_create)
int lanes_from_env() {
    if (const char *e = getenv("FELICS_LANES")) return std::max(1, std::min(atoi(e), MAX_LANES));
    return DEFAULT_LANES;
}

struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
};

// One pipeline lane: HIP streams, stage events and a workspace in HBM of its own.  A submission (or one pass of
// a huge one) runs on one lane; felics_submit_batch_device hands the lanes out in turn, so that the GPU starts
// on the next batch while it finishes the last pack slices of this one.
struct Lane {
    hipStream_t stream = nullptr;      // spine slices
    hipStream_t front = nullptr;       // planes, hist, offsets, scatter slices
    hipStream_t kstream = nullptr;     // assign slices (k of the events); with four lanes there is none and they go to the front stream (felics_ctx_create)
    hipStream_t tail = nullptr;        // lengths, bit scan, pack slices
    hipEvent_t slice_done[SLICES] = {};
    hipEvent_t spine_done[SLICES] = {};
    hipEvent_t assign_done[SLICES] = {};
    hipEvent_t ev[ST_COUNT][EV_PAIRS][2] = {};  // profiling: one start/stop pair per launch of a stage
    int ev_used[ST_COUNT] = {};                  // pairs used by the current sub-batch
    hipEvent_t sized = nullptr;       // stream sizes have landed in h_sizes
    hipEvent_t span_begin = nullptr, span_end = nullptr;  // profiling: in front of the sub-batch's first kernel / behind its last byte
    uint64_t *h_sizes = nullptr;      // pinned: image_bytes[n] followed by image_off[n + 1]
    size_t h_sizes_cap = 0;
    // 8-bit samples, tile-local layout (felics_kernels.h): ev / pix_of / k_sorted = the tiles' slots (event value, pixel, k), counts = the
    // run table, tile_slots, desc / block_state = the records of the chains in chain order (place + events, start state), partial =
    // the chains' record ranges per slice
    // (8-bit: image_bytes is the head of the lane's CLEARED BLOCK -- sizes, error word, counters, plane sums, chain_state: run_lane)
    DevBuf planes, counts, scalars, evs, pix_of, k_map, k_sorted, block_state, group_bits, tile_slots, desc,
        tile_bits, tile_bitoff, plane_sums, image_bytes, image_off, partial, status, edge_first, edge_last, pscratch;
    uint64_t *plane_base = nullptr;   // the sub-batch's plane bases (behind its plane carries; pack_exact reads them)
    DevBuf wrecs[2], wtile_cnt, wmeta, whist, wdigtot, heads, wlong;  // 16-bit samples: event records (sort double buffer), tile counts, plane ranges, digit histograms, chain heads
    uint32_t epoch = 0;               // sub-batches this lane has run: block tags are (epoch, slice)
    // the submission in flight on this lane (felics_submit_batch_device .. felics_wait_batch)
    bool pending = false;
    bool finished = false;            // it took the synchronous path: results are in r_off / r_len / r_rc
    size_t p_n = 0;
    const void *p_pixels = nullptr;
    uint32_t p_w = 0, p_h = 0;
    int p_color = 0, p_depth = 0;
    uint8_t *p_out = nullptr;
    size_t p_cap = 0;
    uint64_t p_slot = 0;
    std::vector<uint64_t> r_off, r_len;
    int r_rc = 0;
    // the sub-batch in flight
    int nslices = SLICES;             // slices its tiles are cut into (see felics_ctx::slices_*)
    bool m_tickets = false;           // the sub-batch's pack kernels took their tiles by ticket (what a look-back failure escalates from)
    bool m_fused = false;             // ... and were the single-pass kernels at all
    bool queued = false;              // this sub-batch came through felics_submit_batch_device (other submissions share the GPU with it)
    Geometry g;
    size_t first_image = 0;
    const void *d_planes = nullptr;
    // a mixed sub-batch (felics_compress_images*): its plane table, written on the host (pinned) and copied to the device
    DevBuf mtable;
    PlaneGeom *h_table = nullptr;
    size_t h_table_cap = 0;
};

}  // namespace

struct felics_ctx {
    int device = -1;
    int next_lane = 0;          // lane of the next felics_submit_batch_device
    int nlanes = DEFAULT_LANES; // lanes in use (FELICS_LANES)
    // Slices per sub-batch: the stages follow each other slice by slice, so more slices let assign / pack start earlier behind the
    // spine -- and every slice costs a launch, a hand-over per stage and a resume of every chain.  Round 5, blocking calls
    // (profiles/r05/experiments.txt): 64 S1 frames 2 / 3 / 4 / 6 / 8 slices 2.95 / 2.68 / 2.75 / 2.79 / 2.76 ms, noise 4.19 / 4.37 /
    // 4.52 / 4.96 / 5.37, one 4K frame 1.99 / 1.93 / 1.95 / 2.04 / 2.15 (round 4's pipeline wanted 6).
    int slices_blocking = 3;    // FELICS_SLICES
    int slices_queued = 2;      // (round 5, tile-local pipeline: 1 slice 3.05, 2 2.54, 3 2.90, 4 2.86, 6 2.82 ms per step with two lanes; round 3 measured 2-4 lanes x 1-6 slices within 3 % of each other: profiles/r03/experiments.txt;
                                // round 4, with k_scatter: 2 slices 2.94, 3 2.82-2.89, 4 2.78-2.80, 6 2.89-2.91, 8 2.96 ms; three lanes 3.06)
    // k_pack_g takes its tiles from the workgroup index while the lanes share the tail stream: one pack kernel then has the
    // look-back to itself.  With a tail stream per lane (FELICS_OWN_TAILS=1), and after a look-back has given up once, tiles are
    // handed out by a ticket counter instead: a tile then only ever waits for tiles held by workgroups that are already running,
    // whatever else shares the GPU.  The counter is one memory-side atomic per tile on one address -- 130 000 per step at the
    // ~88 per microsecond one address sustains (MI355X_MICROARCH.md, dequeue) -- measured 1.59 against 1.26 ms of pack launches per step.
    bool pack_tickets = false;
    bool two_pass = false;      // FELICS_TWO_PASS=1, or a look-back gave up with ticketed tiles as well: lengths + pack kernels
    bool own_tails = false;     // FELICS_OWN_TAILS=1: a tail stream per lane (pack kernels of two submissions side by side, tiles by ticket)
    int assign_on = ASSIGN_OWN; // up to three lanes; ASSIGN_FRONT with four (felics_ctx_create); FELICS_ASSIGN_STREAM=own|front|tail (tuning sweeps: profiles/hw_queues.txt)
    bool serial = false;        // FELICS_SERIAL=1 (profiling tools: every kernel alone): all stages of a lane on one stream
    bool test_timeout = false;  // FELICS_TEST_TIMEOUT=1: every wait for the GPU reports a time-out (tests of the failed state)
    bool test_lookback = false; // FELICS_TEST_LOOKBACK_FAIL=1: pretend the first single-pass submission gave up (tests)
    // The front kernel ranks a tile's events with returning LDS atomics and CHECKS the order it produced (felics_kernels.hip,
    // k_front); a context whose check fails once ranks with ballots from then on (FELICS_SCATTER=ballot starts that way: tests).
    bool scatter_ballot = false;
    // Slots per tile of the tile-local layout: the default covers anything but adversarial content; a tile that needs more
    // raises TL_FLAG_OVERFLOW, the batch is redone with the worst case and the context keeps to it (FELICS_TEST_TILE_CAP=1
    // starts with a cap so small that the first batch overflows: tests).
    bool cap_max = false;
    bool test_tile_cap = false;
    bool test_scatter_order = false; // FELICS_TEST_SCATTER_ORDER=1: k_scatter reports a violation whatever it produced (tests)
    bool poison = false;        // FELICS_POISON=1: overwrite the workspace before every sub-batch (tests)
    bool trace = false;         // FELICS_TRACE=1: synchronise and report after every stage (debugging)
    int timeout_s = 120;        // FELICS_TIMEOUT_S: give up waiting for a submission after this long
    // A wait for the GPU timed out: kernels of this context may still be running (or never return), so nothing
    // of it may be reused or freed.  Every later call fails with FELICS_E_HIP; the caller should exit (or run
    // further work in a fresh process).
    bool failed = false;
    felics_stats stats = {};
    Lane lanes[MAX_LANES];
    std::string err;
    bool profiling = false;
    float stage_ms[ST_COUNT] = {};
    float span_ms = 0.f;        // profiling: first kernel -> sizes on the host, of the last submission collected
    int stage_launches[ST_COUNT] = {};
    DevBuf in, out;  // staging of the host-pointer entry point: the batch's frames, the chunks' output slots
    hipStream_t copy_in = nullptr, copy_out = nullptr;  // felics_compress_batch: frames to the device / streams back, beside the kernels
    std::vector<hipEvent_t> h2d_done;                   // a chunk's frames have arrived (one per chunk of a host-buffer batch; grown on demand)
    hipEvent_t wait_before_submit = nullptr;            // the next sub-batch's first kernel waits for this event (set around one submit)
    DevBuf mix_in, mix_stage, mix_out, mix_redo;  // felics_compress_images*: 16-bit frames gathered per shape and their streams, the first
                                                  // run of a call whose buffer cannot hold the slots, frames gathered for a remedy
    // felics_compress_views_device: the caller's ready event (every stream waits for it before it first reads a view or writes the
    // output: wait_ready), the dense copies of gray8 views that cannot be read in place, the counts of felics_get_view_stats
    hipEvent_t view_ready = nullptr;
    DevBuf view_stage;
    felics_view_stats vstats = {};
    DevBuf own;      // encode_device's own output when the caller gives none (the host entry point's fall-back for a chunk whose streams outgrew their slots)
    DevBuf dec_meta, dec_planes;  // GPU decoder: offsets | lens | status of a batch; Y / Co / Cg planes of RGB streams
    DevBuf dec_planes16;          // mixed decode call: the int32 planes of its RGB16 streams (beside dec_planes, used at the same time)
    DevBuf dec_lane_table;        // gray streams decoded 64 to a wave: the estimator rows that do not fit in LDS (3 KB per stream, zeroed per call)
    DevBuf dec_table;             // 16-bit streams: estimator tables in HBM (8.4 MB per stream of a pass), zeroed once, rows tagged with an epoch
    uint32_t dec_epoch = 0;       // last epoch handed out (three per call: one per plane)
    DevBuf dec_lane16_table;      // 16-bit streams decoded 64 to a wave: their hashed estimator tables (felics_lanetable.h), zeroed once, rows tagged with an epoch
    uint32_t dec_lane16_epoch = 0;  // last epoch handed out on dec_lane16_table (three per launch, 1 .. DEC16L_EPOCH_MAX)
    felics_decode_stats dstats = {};  // felics_get_decode_stats
};

namespace {

int hip_fail(felics_ctx *ctx, hipError_t e, const char *what) {
    char buf[256];
    snprintf(buf, sizeof buf, "%s: %s", what, hipGetErrorString(e));
    if (ctx) ctx->err = buf;
    return FELICS_E_HIP;
}

#define HIP_TRY(ctx, call)                                          \
    do {                                                            \
        hipError_t e__ = (call);                                    \
        if (e__ != hipSuccess) return hip_fail(ctx, e__, #call);    \
    } while (0)

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

void release(DevBuf &b) {
    if (b.p) (void)hipFree(b.p);
    b.p = nullptr;
    b.cap = 0;
}

// Brackets one launch (or a few back-to-back launches) of a stage with HIP events on the stream it runs
// on; a stage's time is the sum over its launches of a sub-batch.
struct StageTimer {
    felics_ctx *ctx;
    Lane &lane;
    int st;
    hipStream_t stream;
    int slot = -1;
    bool exact;  // one kernel launch inside: record that kernel's own begin / end (see LaunchTiming)
    StageTimer(felics_ctx *c, Lane &l, int s, hipStream_t on, bool single_kernel = false)
        : ctx(c), lane(l), st(s), stream(on), exact(single_kernel) {
        if (ctx->profiling && lane.ev_used[st] < EV_PAIRS) {
            slot = lane.ev_used[st]++;
            if (exact)
                g_launch_timing = LaunchTiming{lane.ev[st][slot][0], lane.ev[st][slot][1]};
            else
                (void)hipEventRecord(lane.ev[st][slot][0], stream);
        }
    }
    ~StageTimer() {
        if (slot >= 0) {
            if (!exact) {
                (void)hipEventRecord(lane.ev[st][slot][1], stream);
            } else if (g_launch_timing.start) {  // nothing was launched: give the pair back
                g_launch_timing = LaunchTiming{};
                lane.ev_used[st]--;
            }
        }
        if (ctx->trace) {  // FELICS_TRACE: wait for the stage and say so (locating a kernel that does not return)
            hipError_t e = hipStreamSynchronize(stream);
            fprintf(stderr, "[felics] %s done (%s)\n", kStageNames[st], hipGetErrorString(e));
        }
    }
};

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

// Everything one sub-batch of 8-bit frames needs, queued without waiting for the host (tile-local layout, felics_kernels.h):
//   front stream : one fill that clears the sub-batch's counters, sums and chain states; then slice by slice the front kernel
//                  (classify + sort a tile's events, once) and the records of the slice's chains (k_enum)
//   spine stream : behind every k_enum the spine launch that walks the slice's chains
//   k stream     : behind every spine launch the k of the slice's events (k_assign3); a context of four lanes has no k stream
//                  and queues them on the front stream, behind the NEXT slice's two launches
//   tail stream  : behind every k launch -- when every stream has a fixed slot in the output -- the packed bits of that
//                  slice's tiles (k_pack_t: code lengths, tile offsets by look-back, packing in one kernel); RGB planes 1, 2
//                  go to scratch slots and are moved behind plane 0 at the end (the offset of planes 1 and 2 needs the size
//                  of the planes before them).
// The stream sizes are copied to the lane's pinned buffer and `sized` is recorded behind them.
// slot_stride == 0: no packing here (the caller places the streams exactly once it has the sizes).
template <typename T, typename ET>
int run_lane(felics_ctx *ctx, Lane &l, uint8_t *d_out, uint64_t slot_stride) {
    const Geometry &g = l.g;
    const int ns = l.nslices;
    const size_t nsamples = (size_t)g.nplanes * g.npix;
    int rc = 0;
    // Fixed slots: code lengths, tile offsets and packing in one kernel per slice (k_pack_t; one such kernel at a time unless the
    // tiles are handed out by ticket: the tiles of two of them waiting for each other's queued predecessors could hold all
    // workgroup slots, so the lanes share the tail stream).  Otherwise (exact placement, FELICS_TWO_PASS, after a look-back gave
    // up twice): k to a byte per pixel once every chain is replayed, then the lengths / bit scan / pack kernels over all tiles.
    const bool fused = (slot_stride != 0 || g.mixed != nullptr) && !ctx->two_pass;  // (a mixed sub-batch: slots from its table, never two-pass)
    const uint32_t cap = ctx->cap_max ? tile_cap_max(g.nctx, g.npix) : ctx->test_tile_cap ? std::min(4u * REC, tile_cap_max(g.nctx, g.npix)) : tile_cap_default(g.nctx, g.npix);
    const size_t ptiles = (size_t)g.nplanes * g.sort_tiles;
    const size_t slots = ptiles * cap, recs = slots / REC;
    const size_t nchains = (size_t)g.nplanes * g.nctx;
    if ((rc = reserve(ctx, l.evs, slots * sizeof(ET) + STAGE_PAD)) != 0) return rc;
    if ((rc = reserve(ctx, l.pix_of, slots * 2 + STAGE_PAD)) != 0) return rc;
    if ((rc = reserve(ctx, l.k_sorted, slots + STAGE_PAD)) != 0) return rc;
    if ((rc = reserve(ctx, l.counts, ptiles * g.nctx * 4)) != 0) return rc;        // the run table
    if ((rc = reserve(ctx, l.tile_slots, ptiles * 4)) != 0) return rc;
    if ((rc = reserve(ctx, l.desc, recs * 8 + 64)) != 0) return rc;
    if ((rc = reserve(ctx, l.block_state, recs * 16 + 64)) != 0) return rc;         // state16
    if ((rc = reserve(ctx, l.partial, (size_t)SLICES * nchains * 8)) != 0) return rc;  // chain_seg per slice
    if (!fused && (rc = reserve(ctx, l.k_map, nsamples + STAGE_PAD)) != 0) return rc;
    if (!fused && (rc = reserve(ctx, l.group_bits, (size_t)g.nplanes * g.pack_tiles * PACK_THREADS * 2)) != 0) return rc;
    if ((rc = reserve(ctx, l.tile_bits, (size_t)g.nplanes * g.pack_tiles * 4)) != 0) return rc;
    if ((rc = reserve(ctx, l.tile_bitoff, (size_t)g.nplanes * g.pack_tiles * 8)) != 0) return rc;
    // The cleared block: everything a sub-batch wants zero when it starts, in one allocation, so that ONE fill at the head of the
    // front stream clears it (the lane is idle then: its last sub-batch's sizes have been waited for) and ONE copy brings the
    // sizes, the error word and the flags back:
    //   image_bytes[nimages] | d_error, d_flags | d_tickets[SLICES + 2], d_nrec[SLICES] | carry[nplanes], base[nplanes] | chain_state
    const size_t o_words = (size_t)g.nimages * 8, o_counters = o_words + 8;
    const size_t o_sums = (o_counters + 4 * (2 * SLICES + 2) + 15) & ~(size_t)15;
    const size_t o_chain = (o_sums + (size_t)g.nplanes * 16 + 255) & ~(size_t)255;
    const size_t cleared = o_chain + nchains * 32;
    if ((rc = reserve(ctx, l.image_bytes, cleared)) != 0) return rc;
    if ((rc = reserve(ctx, l.image_off, (size_t)(g.nimages + 1) * 8)) != 0) return rc;
    if ((rc = reserve_zeroed(ctx, l.status, (size_t)g.nplanes * g.pack_tiles * 8)) != 0) return rc;
    if ((rc = reserve(ctx, l.edge_first, (size_t)g.nplanes * g.pack_tiles * 4)) != 0) return rc;
    if ((rc = reserve(ctx, l.edge_last, (size_t)g.nplanes * g.pack_tiles * 4)) != 0) return rc;
    const size_t hs = (size_t)g.nimages * 2 + 1;
    if (hs > l.h_sizes_cap) {
        if (l.h_sizes) HIP_TRY(ctx, hipHostFree(l.h_sizes));
        l.h_sizes = nullptr;
        HIP_TRY(ctx, hipHostMalloc((void **)&l.h_sizes, hs * 8 + 64, hipHostMallocDefault));
        l.h_sizes_cap = hs;
    }
    hipStream_t s = l.stream, f = l.front, tl = l.tail;
    // k_assign3 of slice q follows spine[q] and goes in front of pack[q]: on the lane's k stream, or -- four lanes: the low pool is
    // full of front streams -- on the front stream behind enum[q + 1], which does not wait for the spine
    hipStream_t ks = ctx->assign_on == ASSIGN_TAIL ? tl : l.kstream ? l.kstream : f;
    if (ctx->serial) f = ks = tl = s;  // FELICS_SERIAL (profiling: every kernel alone): one stream, same order of launches
    const T *d_planes = (const T *)l.d_planes;
    uint8_t *block = (uint8_t *)l.image_bytes.p;
    auto *chain_state = (uint32_t *)(block + o_chain);
    auto *plane_carry = (uint64_t *)(block + o_sums);
    auto *plane_base = plane_carry + g.nplanes;
    l.plane_base = plane_base;
    if (++l.epoch >= 0x03FFFFFFu) l.epoch = 1;
    if ((l.epoch & 0x3FFFFu) == 0) HIP_TRY(ctx, hipMemsetAsync(l.status.p, 0, l.status.cap, f));  // look-back tags: 18 epoch bits
    const uint32_t epoch = l.epoch;
    PackTarget target{d_out, slot_stride, nullptr, 0};
    if (fused && g.planes_per_image > 1) {
        target.plane_slot = ((uint64_t)g.npix + g.npix / 4 + 64 + 15) & ~15ull;
        if ((rc = reserve(ctx, l.pscratch, (size_t)(target.plane_slot * g.nimages * (g.planes_per_image - 1)))) != 0) return rc;
        target.scratch = (uint8_t *)l.pscratch.p;
    }
    uint32_t *d_error = (uint32_t *)(block + o_words);  // look-back watchdog of the single-pass pack
    uint32_t *d_flags = d_error + 1;  // TL_FLAG_*: the front kernel's order check and tile overflow, the spine's self-check (read back together with d_error)
    uint32_t *d_tickets = (uint32_t *)(block + o_counters);  // one per pack launch of this sub-batch: tiles are handed out in order
    uint32_t *d_nrec = d_tickets + SLICES + 2;  // records per slice
    const TileLocal<ET> tloc{(ET *)l.evs.p, (uint16_t *)l.pix_of.p, (uint8_t *)l.k_sorted.p, (uint32_t *)l.counts.p, (uint32_t *)l.tile_slots.p, cap};
    l.m_tickets = ctx->pack_tickets;
    l.m_fused = fused;

    uint32_t bounds[SLICES + 1];  // slice boundaries in sort tiles (= pack tiles)
    for (int q = 0; q <= ns; q++) bounds[q] = (uint32_t)((uint64_t)g.sort_tiles * q / ns);
    // the records of slice q live in their own region of desc: as many as its tiles can hold
    auto slice_of = [&](int q) {
        const size_t r0 = (size_t)bounds[q] * g.nplanes * (cap / REC);
        return ChainSlice{(uint2 *)l.desc.p + r0, (uint2 *)l.partial.p + (size_t)q * nchains, d_nrec + q, (uint4 *)l.block_state.p};
    };
    // ---- front stream
    if (ctx->poison) {  // FELICS_POISON: every intermediate buffer starts as garbage, as on a fresh context
        DevBuf *bufs[] = {&l.evs, &l.pix_of, &l.k_sorted, &l.counts, &l.tile_slots, &l.desc, &l.block_state, &l.partial, &l.k_map,
                          &l.group_bits, &l.tile_bits, &l.tile_bitoff, &l.edge_first, &l.edge_last, &l.pscratch};
        for (DevBuf *b : bufs)
            if (b->p) HIP_TRY(ctx, hipMemsetAsync(b->p, 0xA5, b->cap, f));
    }
    HIP_TRY(ctx, hipMemsetAsync(block, 0, cleared, f));  // (the tail's words too: every tail launch follows an assign launch, and that this fill)
    // (FELICS_TEST_SCATTER_ORDER: the atomically ranked kernel reports a violation whatever it produced; the ballot-ranked form is
    // the remedy and is checked for real)
    const uint32_t front_mode = ctx->scatter_ballot ? FRONT_SAFE_RANK : ctx->test_scatter_order ? FRONT_TEST_VIOLATION : 0u;
    if (!ctx->scatter_ballot) ctx->stats.sorted_event_sorts++;
    // behind every spine launch, k of the slice's events and -- when every stream has a fixed slot -- the packed bits of the slice's
    // tiles on the tail stream.  Queued one slice late, so that on the front stream the k launch stands behind the NEXT slice's
    // front and enum launches (which do not wait for the spine) and not in front of them.
    auto behind_spine = [&](int q) -> int {
        HIP_TRY(ctx, hipStreamWaitEvent(ks, l.spine_done[q], 0));
        if (bounds[q + 1] != bounds[q]) {
            StageTimer t(ctx, l, ST_ASSIGN, ks, true);
            launch_assign3<ET>(ks, tloc, (const uint4 *)l.block_state.p, g, bounds[q], bounds[q + 1]);
        }
        HIP_TRY(ctx, hipEventRecord(l.assign_done[q], ks));
        if (!fused) return FELICS_OK;
        HIP_TRY(ctx, hipStreamWaitEvent(tl, l.assign_done[q], 0));
        if (bounds[q + 1] == bounds[q]) return FELICS_OK;
        StageTimer t(ctx, l, ST_PACK, tl, true);
        launch_pack_t<T>(tl, d_planes, tloc.kq, tloc.pix, tloc.ev, tloc.tile_slots, cap, (uint64_t *)l.status.p, (uint64_t *)l.tile_bitoff.p,
                         (uint32_t *)l.tile_bits.p, plane_carry, (uint32_t *)l.edge_first.p, (uint32_t *)l.edge_last.p, d_error, target, g,
                         bounds[q], bounds[q + 1], epoch, ctx->pack_tickets ? d_tickets + q : nullptr);
        return FELICS_OK;
    };
    for (int q = 0; q < ns; q++) {
        if (bounds[q + 1] != bounds[q]) {
            {
                StageTimer t(ctx, l, ST_SCATTER, f, true);
                launch_front<T, ET>(f, d_planes, tloc, g, bounds[q], bounds[q + 1], d_flags, front_mode);
            }
            // the slice's records in chain order: here, not on the spine stream, so that it runs beside the previous slice's walk
            StageTimer t(ctx, l, ST_OFFSETS, f, true);
            launch_enum(f, tloc.runtab, slice_of(q), g, bounds[q], bounds[q + 1], cap);
        }
        HIP_TRY(ctx, hipEventRecord(l.slice_done[q], f));
        // ---- spine stream: the walk along every chain
        HIP_TRY(ctx, hipStreamWaitEvent(s, l.slice_done[q], 0));
        if (bounds[q + 1] != bounds[q]) {
            StageTimer t(ctx, l, ST_SPINE, s, true);
            launch_spine3<ET>(s, tloc.ev, slice_of(q), chain_state, d_flags, g);
        }
        HIP_TRY(ctx, hipEventRecord(l.spine_done[q], s));
        if (q > 0 && (rc = behind_spine(q - 1)) != 0) return rc;
    }
    if ((rc = behind_spine(ns - 1)) != 0) return rc;
    // ---- tail stream: the sizes, and the streams' last touches
    if (fused) {
        StageTimer t(ctx, l, ST_ZERO, tl);
        launch_finish_sizes(tl, plane_carry, plane_base, (uint64_t *)l.image_bytes.p, g);
        launch_join_edges(tl, (const uint64_t *)l.tile_bitoff.p, (const uint32_t *)l.tile_bits.p,
                          (const uint32_t *)l.edge_first.p, (const uint32_t *)l.edge_last.p, target, g);
        launch_concat_planes(tl, plane_base, plane_carry, target, g);
    } else {
        HIP_TRY(ctx, hipStreamWaitEvent(tl, l.assign_done[ns - 1], 0));
        {
            StageTimer t(ctx, l, ST_ASSIGN, tl, true);
            launch_k_to_pixels_tl(tl, tloc.kq, tloc.pix, tloc.tile_slots, cap, (uint8_t *)l.k_map.p, g);
        }
        {
            StageTimer t(ctx, l, ST_LENGTHS, tl, true);
            launch_lengths<T>(tl, d_planes, (const uint8_t *)l.k_map.p, (uint16_t *)l.group_bits.p,
                              (uint32_t *)l.tile_bits.p, g, 0, g.pack_tiles);
        }
        {
            StageTimer t(ctx, l, ST_BITSCAN, tl);
            launch_bitscan_slice(tl, (const uint32_t *)l.tile_bits.p, (uint64_t *)l.tile_bitoff.p, plane_carry, g, 0, g.pack_tiles);
            launch_finish_sizes(tl, plane_carry, plane_base, (uint64_t *)l.image_bytes.p, g);
        }
        if (slot_stride != 0) {
            {
                StageTimer t(ctx, l, ST_ZERO, tl);
                launch_zero_edges(tl, d_out, nullptr, slot_stride, (const uint64_t *)l.tile_bitoff.p,
                                  (const uint32_t *)l.tile_bits.p, plane_base, g, 0, g.pack_tiles);
            }
            StageTimer t(ctx, l, ST_PACK, tl, true);
            launch_pack<T>(tl, d_planes, (const uint8_t *)l.k_map.p, (const uint16_t *)l.group_bits.p,
                           (const uint64_t *)l.tile_bitoff.p, (const uint32_t *)l.tile_bits.p, plane_base, nullptr,
                           slot_stride, d_out, g, 0, g.pack_tiles);
        }
    }
    HIP_TRY(ctx, hipGetLastError());
    l.h_sizes[g.nimages] = 0;
    HIP_TRY(ctx, hipMemcpyAsync(l.h_sizes, block, o_counters, hipMemcpyDeviceToHost, tl));  // the sizes, then d_error | d_flags << 32
    HIP_TRY(ctx, hipEventRecord(l.sized, tl));
    if (ctx->profiling) HIP_TRY(ctx, hipEventRecord(l.span_end, tl));
    return FELICS_OK;
}

// 16-bit samples (T = u16 gray planes, i32 Y/Co/Cg planes): everything on the lane's main stream.
//   keys -> stable sort by (plane, context) -> chain heads -> estimator replay per chain (k_map)
//   -> lengths, bit scan, sizes -> pack (fixed slots) ; same contract as run_lane towards the caller.
template <typename T>
int run_wide(felics_ctx *ctx, Lane &l, uint8_t *d_out, uint64_t slot_stride) {
    const Geometry &g = l.g;
    const size_t nsamples = (size_t)g.nplanes * g.npix;
    const WideSizes z = wide_sizes(g);
    int rc;
    for (int i = 0; i < 2; i++)
        if ((rc = reserve(ctx, l.wrecs[i], z.rec_bytes)) != 0) return rc;
    if ((rc = reserve(ctx, l.wtile_cnt, z.tile_cnt_bytes)) != 0) return rc;
    if ((rc = reserve(ctx, l.wmeta, z.meta_bytes)) != 0) return rc;
    if ((rc = reserve(ctx, l.whist, z.hist_bytes)) != 0) return rc;
    if ((rc = reserve(ctx, l.wdigtot, z.digtot_bytes)) != 0) return rc;
    if ((rc = reserve(ctx, l.heads, z.heads_bytes)) != 0) return rc;
    if ((rc = reserve(ctx, l.scalars, 64)) != 0) return rc;
    uint32_t lane_limit = wide_lane_limit(g);
    if (const char *e = getenv("FELICS_WIDE_LANE")) lane_limit = (uint32_t)std::max(0, atoi(e));  // tests, A/B: 0 = wave-wide only
    const size_t nlong = wide_long_capacity(g, lane_limit);
    if ((rc = reserve(ctx, l.wlong, nlong * (8 + 64) + 64)) != 0) return rc;
    if ((rc = reserve(ctx, l.k_map, nsamples + STAGE_PAD)) != 0) return rc;
    if ((rc = reserve(ctx, l.group_bits, (size_t)g.nplanes * g.pack_tiles * PACK_THREADS * sizeof(group_bits_t<T>))) != 0) return rc;
    if ((rc = reserve(ctx, l.tile_bits, (size_t)g.nplanes * g.pack_tiles * 4)) != 0) return rc;
    if ((rc = reserve(ctx, l.tile_bitoff, (size_t)g.nplanes * g.pack_tiles * 8)) != 0) return rc;
    if ((rc = reserve(ctx, l.plane_sums, (size_t)g.nplanes * 16)) != 0) return rc;
    if ((rc = reserve(ctx, l.image_bytes, (size_t)g.nimages * 8)) != 0) return rc;
    if ((rc = reserve(ctx, l.image_off, (size_t)(g.nimages + 1) * 8)) != 0) return rc;
    const size_t hs = (size_t)g.nimages * 2 + 1;
    if (hs > l.h_sizes_cap) {
        if (l.h_sizes) HIP_TRY(ctx, hipHostFree(l.h_sizes));
        l.h_sizes = nullptr;
        HIP_TRY(ctx, hipHostMalloc((void **)&l.h_sizes, hs * 8 + 64, hipHostMallocDefault));
        l.h_sizes_cap = hs;
    }
    hipStream_t s = l.stream;
    const T *d_planes = (const T *)l.d_planes;
    auto *plane_carry = (uint64_t *)l.plane_sums.p;
    auto *plane_base = plane_carry + g.nplanes;
    l.plane_base = plane_base;
    auto *nheads = (uint32_t *)l.scalars.p;
    if (ctx->poison) {
        DevBuf *bufs[] = {&l.wrecs[0], &l.wrecs[1], &l.wtile_cnt, &l.wmeta, &l.whist, &l.heads, &l.k_map,
                          &l.group_bits, &l.tile_bits, &l.tile_bitoff};
        for (DevBuf *b : bufs) HIP_TRY(ctx, hipMemsetAsync(b->p, 0xA5, b->cap, s));
    }
    {
        StageTimer t(ctx, l, ST_WIDE_KEYS, s);
        launch_wide_events<T>(s, d_planes, (uint32_t *)l.wtile_cnt.p, (uint32_t *)l.wmeta.p, (uint64_t *)l.wrecs[0].p, g);
    }
    {
        StageTimer t(ctx, l, ST_WIDE_SORT, s);
        launch_wide_sort(s, (uint64_t *)l.wrecs[0].p, (uint64_t *)l.wrecs[1].p, (const uint32_t *)l.wmeta.p, (uint32_t *)l.whist.p,
                         (uint32_t *)l.wdigtot.p, g);
    }
    {
        StageTimer t(ctx, l, ST_WIDE_CHAINS, s);
        HIP_TRY(ctx, hipMemsetAsync(nheads, 0, 8, s));
        launch_wide_chains(s, (const uint64_t *)l.wrecs[0].p, (const uint32_t *)l.wmeta.p, (uint64_t *)l.heads.p, nheads,
                           (uint8_t *)l.k_map.p, g, lane_limit, (uint64_t *)l.wlong.p, (uint32_t *)((uint64_t *)l.wlong.p + nlong));
    }
    HIP_TRY(ctx, hipMemsetAsync(plane_carry, 0, (size_t)g.nplanes * 16, s));
    {
        StageTimer t(ctx, l, ST_LENGTHS, s, true);
        launch_lengths<T>(s, d_planes, (const uint8_t *)l.k_map.p, (group_bits_t<T> *)l.group_bits.p,
                          (uint32_t *)l.tile_bits.p, g, 0, g.pack_tiles);
    }
    {
        StageTimer t(ctx, l, ST_BITSCAN, s);
        launch_bitscan_slice(s, (const uint32_t *)l.tile_bits.p, (uint64_t *)l.tile_bitoff.p, plane_carry, g, 0,
                             g.pack_tiles);
        launch_finish_sizes(s, plane_carry, plane_base, (uint64_t *)l.image_bytes.p, g);
    }
    if (slot_stride != 0 || g.mixed) {  // (a mixed sub-batch: every stream into the slot its table row names)
        {
            StageTimer t(ctx, l, ST_ZERO, s);
            launch_zero_edges(s, d_out, nullptr, slot_stride, (const uint64_t *)l.tile_bitoff.p,
                              (const uint32_t *)l.tile_bits.p, plane_base, g, 0, g.pack_tiles);
        }
        {
            StageTimer t(ctx, l, ST_PACK, s, true);
            launch_pack<T>(s, d_planes, (const uint8_t *)l.k_map.p, (const group_bits_t<T> *)l.group_bits.p,
                           (const uint64_t *)l.tile_bitoff.p, (const uint32_t *)l.tile_bits.p, plane_base, nullptr,
                           slot_stride, d_out, g, 0, g.pack_tiles);
        }
    }
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(l.h_sizes, l.image_bytes.p, (size_t)g.nimages * 8, hipMemcpyDeviceToHost, s));
    HIP_TRY(ctx, hipEventRecord(l.sized, s));
    if (ctx->profiling) HIP_TRY(ctx, hipEventRecord(l.span_end, s));
    return FELICS_OK;
}

// Exact placement: streams back to back at image_off (computed on the device from the sizes), every
// byte of them zeroed, all tiles packed.  Used when the streams do not get fixed slots, and to redo a
// sub-batch in which a stream outgrew its slot.
template <typename T>
int pack_exact(felics_ctx *ctx, Lane &l, uint8_t *d_out) {
    const Geometry &g = l.g;
    hipStream_t s = l.tail;
    const uint64_t *plane_base = l.plane_base;
    {
        StageTimer t(ctx, l, ST_ZERO, s);
        launch_zero_streams(s, (uint32_t *)d_out, (const uint64_t *)l.image_off.p, g);
    }
    {
        StageTimer t(ctx, l, ST_PACK, s, true);
        launch_pack<T>(s, (const T *)l.d_planes, (const uint8_t *)l.k_map.p, (const group_bits_t<T> *)l.group_bits.p,
                       (const uint64_t *)l.tile_bitoff.p, (const uint32_t *)l.tile_bits.p, plane_base,
                       (const uint64_t *)l.image_off.p, 0, d_out, g, 0, g.pack_tiles);
    }
    HIP_TRY(ctx, hipGetLastError());
    return FELICS_OK;
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

// images per pass so that slots / chain bases (8-bit) or sample indices and sort keys (16-bit) stay below 2^32
size_t max_images_per_pass(uint64_t npix, uint32_t planes, int depth) {
    const uint64_t per_image = npix * planes;
    if (per_image == 0) return SIZE_MAX;
    if (const char *e = getenv("FELICS_TEST_PASS_IMAGES"))  // tests: several passes without a 100 GB batch
        return (size_t)std::max(1, atoi(e));
    if (depth == FELICS_DEPTH_16) {
        // ~30 bytes of workspace per sample: keep a pass near 2^30 samples -- and near 2^16 planes: the 16-bit front end scans
        // tiles x planes counts in one workgroup and searches the plane table per sort tile (a batch of many tiny frames)
        constexpr uint64_t WIDE_MAX_PLANES = 1u << 16;
        return (size_t)std::max<uint64_t>(1, std::min<uint64_t>(0x40000000ull / per_image, WIDE_MAX_PLANES / planes));
    }
    // the records of a pass are numbered with 32 bits: tiles x records per tile (worst case)
    const uint64_t tiles = (npix + SORT_TILE - 1) / SORT_TILE;
    const uint64_t rec_per_image = tiles * planes * (tile_cap_max(NCTX, (uint32_t)std::min<uint64_t>(npix, SORT_TILE)) / REC);
    // ... and a pass carries at most PASS_MAX_CHAINS = 2^23 chains (plane x context: 2^15 gray planes, 5 461 RGB images -- a batch
    // of many tiny frames).  partial / chain_prog hold SLICES * 8 + 32 bytes per chain, so the per-chain workspace of a pass stops
    // at 2^23 * 128 B = 1 GiB per lane (200 000 gray 8 x 8 frames as one pass held 9 GB), and felics_chain.hip numbers chains
    // (plane * nctx + ctx) and sizes k_enum's and k_spine3's grids by them in 32 bits.  Not 2^24: k_enum runs one 256-thread
    // workgroup per chain (planes rounded up to eight), and a grid of exactly 2^24 of them -- 2^32 work-items, a full pass of
    // 2^16 gray planes -- is refused by the runtime ("invalid configuration argument")
    const uint64_t chains_per_image = (uint64_t)planes * (planes == 3 ? nctx_of<int16_t>() : nctx_of<uint8_t>());
    return (size_t)std::max<uint64_t>(
        1, std::min<uint64_t>({0xE0000000ull / per_image, 0xE0000000ull / rec_per_image, PASS_MAX_CHAINS / chains_per_image}));
}

// Queues one sub-batch (cnt frames starting at frame `first` of d_pixels) on a lane: geometry, colour
// transform, and everything run_lane / run_wide enqueue.  Returns without waiting.
int launch_sub_batch(felics_ctx *ctx, Lane &l, size_t first, size_t cnt, const void *d_pixels, uint32_t w, uint32_t h,
                     int color, int depth, uint8_t *lane_out, uint64_t slot, int nslices, bool queued = false) {
    l.nslices = std::max(1, std::min(nslices, SLICES));
    l.queued = queued;
    ctx->stats.submissions++;
    const uint32_t planes = color == FELICS_COLOR_RGB ? 3 : 1;
    const uint64_t npix = (uint64_t)w * h;
    const bool wide = depth == FELICS_DEPTH_16;
    const size_t frame_bytes = (size_t)npix * planes * (wide ? 2 : 1);
    int rc;
    Geometry &g = l.g;
    g.mixed = nullptr;
    g.pitched = nullptr;
    g.W = w;
    g.H = h;
    g.npix = (uint32_t)npix;
    g.nimages = (uint32_t)cnt;
    g.planes_per_image = planes;
    g.nplanes = (uint32_t)(cnt * planes);
    g.sort_tiles = (uint32_t)((npix + SORT_TILE - 1) / SORT_TILE);
    g.pack_tiles = (uint32_t)((npix + PACK_TILE - 1) / PACK_TILE);
    g.color = (uint32_t)color;
    g.depth = (uint32_t)depth;
    g.nctx = planes == 3 ? nctx_of<int16_t>() : nctx_of<uint8_t>();  // (16-bit samples: run_wide has tables of its own)
    l.first_image = first;
    const uint8_t *src = (const uint8_t *)d_pixels + first * frame_bytes;
    l.d_planes = src;
    if (ctx->wait_before_submit)  // (felics_compress_batch: the frames are still on their way)
        HIP_TRY(ctx, hipStreamWaitEvent(wide || ctx->serial ? l.stream : l.front, ctx->wait_before_submit, 0));
    if (ctx->profiling)  // on the stream the sub-batch's first kernel runs on
        HIP_TRY(ctx, hipEventRecord(l.span_begin, wide || ctx->serial ? l.stream : l.front));
    if (planes == 3) {
        if ((rc = reserve(ctx, l.planes, (size_t)g.nplanes * npix * (wide ? 4 : 2) + STAGE_PAD)) != 0) return rc;
        hipStream_t fs = wide || ctx->serial ? l.stream : l.front;
        StageTimer t(ctx, l, ST_PLANES, fs, true);
        if (wide)
            launch_rgb16_to_planes(fs, (const uint16_t *)src, (int32_t *)l.planes.p, g.npix, g.nimages);
        else
            launch_rgb8_to_planes(fs, src, (int16_t *)l.planes.p, g.npix, g.nimages);
        l.d_planes = l.planes.p;
    }
    if (wide) return planes == 3 ? run_wide<int32_t>(ctx, l, lane_out, slot) : run_wide<uint16_t>(ctx, l, lane_out, slot);
    return planes == 3 ? run_lane<int16_t, uint16_t>(ctx, l, lane_out, slot) : run_lane<uint8_t, uint8_t>(ctx, l, lane_out, slot);
}

// What the sizes that came back say about a sub-batch packed into fixed slots.
struct SlotOutcome {
    bool lookback_failed = false;  // a tile of the single-pass pack gave up waiting for the tiles before it
    bool overflow = false;         // a stream outgrew its slot, or an RGB plane its scratch slot
    bool order_violation = false;  // the front kernel's check of its own output failed: nothing of this sub-batch is to be used
    bool tile_overflow = false;    // a tile's events did not fit its slots (tile_cap_default): nothing of this sub-batch is to be used
    bool spine_error = false;      // the spine's search lost its invariant (never seen): an internal error, reported as such
    bool redo() const { return lookback_failed || order_violation || tile_overflow; }
};

SlotOutcome read_sizes(felics_ctx *ctx, Lane &l, bool wide, uint64_t slot, uint64_t *offsets, uint64_t *lens) {
    SlotOutcome o;
    const uint32_t err = (uint32_t)l.h_sizes[l.g.nimages], flags = (uint32_t)(l.h_sizes[l.g.nimages] >> 32);
    if (!wide) {
        if ((err & 1u) != 0 || (ctx->test_lookback && l.m_fused)) o.lookback_failed = true;
        if ((err & 2u) != 0) o.overflow = true;
        if ((flags & TL_FLAG_ORDER) != 0) o.order_violation = true;
        if ((flags & TL_FLAG_OVERFLOW) != 0) o.tile_overflow = true;
        if ((flags & TL_FLAG_SPINE) != 0) o.spine_error = true;
    }
    for (size_t i = 0; i < l.g.nimages; i++) {
        lens[l.first_image + i] = l.h_sizes[i];
        offsets[l.first_image + i] = (uint64_t)(l.first_image + i) * slot;
        if (slot != 0 && l.h_sizes[i] > slot) o.overflow = true;
    }
    return o;
}

// A tile of the single-pass pack gave up waiting for the tiles before it.  With tiles taken from the workgroup index that can
// be this context's own doing (a predecessor's workgroup not started yet: XCDs dispatch their shares of a grid independently
// and the other lane's kernels share them), so the first remedy is the ticket counter -- same kernel, a tile then only waits
// for workgroups that are running.  If a ticketed pack gives up as well, something else holds the GPU for a second at a time:
// the context packs with the two-pass kernels from then on.
void note_lookback_failure(felics_ctx *ctx, const Lane &l) {
    ctx->stats.lookback_fallbacks++;
    if (!l.m_tickets) {  // (what the failed sub-batch itself ran with: two queued submissions that fail together both get here)
        if (!ctx->pack_tickets) ctx->stats.ticket_retries++;
        ctx->pack_tickets = true;
        ctx->err = "a tile gave up waiting for its predecessors: this context now hands its pack tiles out by ticket";
    } else {
        ctx->two_pass = true;
        ctx->stats.two_pass = 1;
        ctx->err = "a tile gave up waiting for its predecessors: this context now packs with the two-pass kernels (slower)";
    }
}

// k_front ranks a batch of events with one returning LDS atomic and relies on the lanes that name one address being served in
// lane order -- which this hardware does (profiles/tools/micro/lds_atomic_order.hip) and no document promises; so the kernel
// checks the order of what it wrote, and a context whose check fails once ranks with ballots from then on.
void note_scatter_order_violation(felics_ctx *ctx) {
    ctx->stats.scatter_fallbacks++;
    ctx->scatter_ballot = true;
    ctx->err = "the front kernel's order check failed: this context now ranks events with ballots";
}

// A tile's events did not fit the slots a tile gets by default: the worst case from now on (more memory, same kernels).
void note_tile_overflow(felics_ctx *ctx) {
    ctx->stats.tile_overflows++;
    ctx->cap_max = true;
    ctx->test_tile_cap = false;
    ctx->err = "a tile's events outgrew its slots: this context now sizes its tiles for the worst case";
}

int spine_failure(felics_ctx *ctx) {
    ctx->err = "internal error: the spine's halving search lost its invariant";
    return FELICS_E_HIP;
}

// Encode `n` same-shape frames resident in device memory into d_out (device), on one lane, and wait.
// If d_out is NULL the context's own output buffer is used (and grown).
int encode_device(felics_ctx *ctx, Lane &l, size_t n, const void *d_pixels, uint32_t w, uint32_t h, int color, int depth,
                  uint8_t *d_out, size_t d_out_cap, uint64_t *offsets, uint64_t *lens, uint8_t **used_out,
                  bool start_exact = false) {
    const uint32_t planes = color == FELICS_COLOR_RGB ? 3 : 1;
    const uint64_t npix = (uint64_t)w * h;
    const bool wide = depth == FELICS_DEPTH_16;
    if (npix * planes >= 0xE0000000ull) return FELICS_E_UNSUPPORTED;
    if (wide && npix > WIDE_MAX_PLANE_PIXELS) return FELICS_E_UNSUPPORTED;  // an event record keeps the sample index in 29 bits
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    for (int i = 0; i < ST_COUNT; i++) l.ev_used[i] = 0;
    const bool own_out = d_out == nullptr;

    if (npix == 0) {
        // (0,_) | (_,0): header + two zero i32 per plane (compression.rs:94-98); nothing to compute
        const size_t sz = 14 + 8 * planes;
        const size_t stride = (sz + 15) & ~(size_t)15;
        const size_t need = stride * n;
        if (own_out) {
            int rc = reserve(ctx, ctx->own, need);
            if (rc) return rc;
            d_out = (uint8_t *)ctx->own.p;
            d_out_cap = ctx->own.cap;
        }
        if (need > d_out_cap) {
            if (n) lens[0] = need;
            return FELICS_E_BUFFER_TOO_SMALL;
        }
        std::vector<uint8_t> tmp(need, 0);
        for (size_t i = 0; i < n; i++) {
            header_bytes(tmp.data() + i * stride, w, h, color, depth);
            offsets[i] = i * stride;
            lens[i] = sz;
        }
        if (need) HIP_TRY(ctx, hipMemcpy(d_out, tmp.data(), need, hipMemcpyHostToDevice));
        if (used_out) *used_out = d_out;
        return FELICS_OK;
    }

    const size_t frame_bytes = (size_t)npix * planes * (wide ? 2 : 1);
    const size_t per_pass = max_images_per_pass(npix, planes, depth);
    int rc;
    // Placement.  Preferred: every stream gets a fixed slot (stream i at i * slot), so packing needs no
    // size from the host and follows the spine slice by slice.  If a stream outgrows its slot, or the
    // caller's buffer is too small for sensible slots, the streams are placed back to back instead
    // (exact sizes first, then one pack pass).
    uint64_t slot = 0;
    if (own_out) {
        slot = ((uint64_t)frame_bytes + frame_bytes / 4 + 64 + 15) & ~15ull;
        if ((rc = reserve(ctx, ctx->own, (size_t)(slot * n))) != 0) return rc;
        d_out = (uint8_t *)ctx->own.p;
        d_out_cap = ctx->own.cap;
    } else {
        slot = (d_out_cap / n) & ~15ull;
        if (slot < 64 || slot < frame_bytes / 4) slot = 0;
    }
    if (start_exact) slot = 0;

    // (at most: ranks from ballots, worst-case tiles, tickets, two-pass, exact placement, and the run that succeeds; a loop that
    // runs out without one is reported, not passed off as a result)
    bool complete = false;
    for (int attempt = 0; attempt < 7 && !complete; attempt++) {
        size_t done = 0;
        uint64_t out_base = 0;  // exact placement: where the next pass's streams start
        SlotOutcome outcome;
        // passes of up to per_pass frames (one pass unless the batch is huge)
        while (done < n && !outcome.overflow && !outcome.redo()) {
            const size_t cnt = std::min(per_pass, n - done);
            const size_t first = done + cnt;
            if ((rc = launch_sub_batch(ctx, l, done, cnt, d_pixels, w, h, color, depth, d_out + done * slot, slot, ctx->slices_blocking)) != 0) {
                (void)sync_lane(ctx, l);
                return rc;
            }
            if ((rc = wait_event(ctx, l.sized, "stream sizes")) != 0) return rc;
            outcome = read_sizes(ctx, l, wide, slot, offsets, lens);
            if (outcome.spine_error) {
                (void)sync_lane(ctx, l);
                return spine_failure(ctx);
            }
            if (slot == 0 && !outcome.redo()) {
                // exact placement of this pass: back to back, 16-byte aligned, in image order
                uint64_t need = out_base;
                for (size_t i = done; i < first; i++) {
                    offsets[i] = need;
                    need += (lens[i] + 15) & ~15ull;
                }
                if (own_out) {
                    if (done != 0) return FELICS_E_UNSUPPORTED;  // the host entry points submit one pass at a time
                    if ((rc = reserve(ctx, ctx->own, (size_t)need)) != 0) return rc;  // waits for the device
                    d_out = (uint8_t *)ctx->own.p;
                    d_out_cap = ctx->own.cap;
                }
                if (need > d_out_cap) {
                    (void)sync_lane(ctx, l);
                    lens[0] = need;  // capacity needed so far (a lower bound if more passes would follow)
                    return FELICS_E_BUFFER_TOO_SMALL;
                }
                launch_place_streams(l.tail, (const uint64_t *)l.image_bytes.p, (uint64_t *)l.image_off.p, l.g);
                uint8_t *lane_out = d_out + offsets[l.first_image];
                if (wide)
                    rc = planes == 3 ? pack_exact<int32_t>(ctx, l, lane_out) : pack_exact<uint16_t>(ctx, l, lane_out);
                else
                    rc = planes == 3 ? pack_exact<int16_t>(ctx, l, lane_out) : pack_exact<uint8_t>(ctx, l, lane_out);
                if (rc) {
                    (void)sync_lane(ctx, l);
                    return rc;
                }
                out_base = need;
            }
            if ((rc = sync_lane(ctx, l)) != 0) return rc;
            done = first;
        }
        if (outcome.redo()) {
            if ((rc = sync_lane(ctx, l)) != 0) return rc;
            if (outcome.order_violation)
                note_scatter_order_violation(ctx);
            else if (outcome.tile_overflow)
                note_tile_overflow(ctx);
            else
                note_lookback_failure(ctx, l);
            continue;
        }
        if (!outcome.overflow) {
            complete = true;
            break;
        }
        ctx->stats.slot_overflows++;
        slot = 0;  // a stream outgrew its slot: do the batch again with exact placement
    }
    if (!complete) {
        ctx->err = "internal error: the batch was redone with every remedy and still did not complete";
        return FELICS_E_HIP;
    }
    collect_timing(ctx, l);
    if (used_out) *used_out = d_out;
    return FELICS_OK;
}

bool any_pending(const felics_ctx *ctx) {
    for (const Lane &l : ctx->lanes)
        if (l.pending) return true;
    return false;
}

// ---- mixed shapes (felics_compress_images*) ------------------------------------------------------------------------------
// 8-bit images go in BUCKETS of similar size: sorted by sort tiles T = ceil(w h / SORT_TILE), a bucket holds T_min .. ceil(1.25 T_min)
// (at most 25 % of a bucket's tiles are padding), and a bucket is one sub-batch whose tile count is uniform at its T_max; what
// differs per plane (samples, W, H, npix, the image's slot) comes from a table (Geometry::mixed).  16-bit images are bucketed by the
// same rule; a bucket (or a pass of one) of ONE shape takes the uniform path (frames gathered in mix_in, streams copied out of
// mix_stage), every other one is a mixed 16-bit sub-batch: run_wide with the table, frames read in place, streams straight into
// their slots.  The sub-batches are queued over the lanes like felics_compress_batch's chunks.

constexpr size_t MIX_MAX_IMAGES = 8192;  // images of one mixed sub-batch (k_concat_planes / k_rgb8_to_planes_mixed: one grid row per image)

struct MixImage {
    const uint8_t *px;  // device
    uint32_t w, h;
    int color, depth;
    uint64_t npix;
    uint32_t planes;
    size_t frame_bytes;
    // felics_compress_views_device: the frame is not dense at px but the view vr -- read where it lies by the mixed path (gray8
    // rows `pitch` bytes apart; RGB8 of any strides through the plane transform), gathered into a dense frame where a path wants
    // one (16-bit groups, remedies: stage_frame)
    bool view = false;
    uint64_t pitch = 0;
    ViewRow vr = {};
};

// The caller's ready event in front of a stream's first access to a view or to the output (felics_compress_views_device).
int wait_ready(felics_ctx *ctx, hipStream_t s) {
    if (ctx->view_ready) HIP_TRY(ctx, hipStreamWaitEvent(s, ctx->view_ready, 0));
    return FELICS_OK;
}

// Image m as a dense frame at dst: a copy, or the gather of its view (counted: felics_view_stats::bytes_staged).
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
    ctx->vstats.bytes_staged += m.frame_bytes;
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

// a stream's slot, as encode_device sizes one
uint64_t mix_slot(size_t frame_bytes) { return ((uint64_t)frame_bytes + frame_bytes / 4 + 64 + 15) & ~15ull; }
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
};

// The lane's pinned plane table, for nplanes rows (and one extra row per plane: launch_mixed)
int reserve_table(felics_ctx *ctx, Lane &l, uint32_t nplanes) {
    if (nplanes > l.h_table_cap) {
        if (l.h_table) HIP_TRY(ctx, hipHostFree(l.h_table));
        l.h_table = nullptr;
        HIP_TRY(ctx, hipHostMalloc((void **)&l.h_table, (size_t)nplanes * (sizeof(PlaneGeom) + sizeof(PitchedGeom)), hipHostMallocDefault));
        l.h_table_cap = nplanes;
    }
    return FELICS_OK;
}

// Queues a mixed 8-bit sub-batch on lane l (see launch_sub_batch).
int launch_mixed(felics_ctx *ctx, Lane &l, const std::vector<MixImage> &im, const std::vector<size_t> &idx, const MixOut &o, int nslices) {
    const MixImage &f = im[idx[0]];
    const uint32_t planes = f.planes;
    const size_t cnt = idx.size();
    uint32_t tmax = 0;
    uint64_t max_npix = 0;
    for (size_t i : idx) {
        tmax = std::max(tmax, sort_tiles_of(im[i].npix));
        max_npix = std::max(max_npix, im[i].npix);
    }
    l.nslices = std::max(1, std::min(nslices, SLICES));
    l.queued = true;
    ctx->stats.submissions++;
    for (int i = 0; i < ST_COUNT; i++) l.ev_used[i] = 0;
    Geometry &g = l.g;
    g.W = SORT_TILE;  // (the uniform fields describe the padded planes: T_max tiles of SORT_TILE pixels)
    g.H = tmax;
    g.npix = tmax * SORT_TILE;
    g.nimages = (uint32_t)cnt;
    g.planes_per_image = planes;
    g.nplanes = (uint32_t)(cnt * planes);
    g.sort_tiles = tmax;
    g.pack_tiles = tmax;
    g.color = (uint32_t)f.color;
    g.depth = FELICS_DEPTH_8;
    g.nctx = planes == 3 ? nctx_of<int16_t>() : nctx_of<uint8_t>();
    l.first_image = 0;
    int rc;
    const uint64_t pstride = g.npix;  // samples between two planes of the planes buffer (RGB)
    if (planes == 3 && (rc = reserve(ctx, l.planes, (size_t)g.nplanes * pstride * 2 + STAGE_PAD)) != 0) return rc;
    // (behind the table, room for what views add to it: the pitched policy's rows of a gray sub-batch, the views of an RGB one)
    static_assert(sizeof(PitchedGeom) >= sizeof(ViewRow) && sizeof(PlaneGeom) % 8 == 0, "one extra row per plane holds either");
    if ((rc = reserve_table(ctx, l, g.nplanes)) != 0) return rc;
    bool any_view = false;
    for (size_t i : idx) any_view = any_view || im[i].view;
    const size_t extra_off = (size_t)g.nplanes * sizeof(PlaneGeom);
    PitchedGeom *h_pitched = (PitchedGeom *)((uint8_t *)l.h_table + extra_off);  // gray
    ViewRow *h_views = (ViewRow *)((uint8_t *)l.h_table + extra_off);            // RGB
    for (size_t j = 0; j < cnt; j++) {
        const MixImage &m = im[idx[j]];
        for (uint32_t c = 0; c < planes; c++) {
            PlaneGeom &pg = l.h_table[j * planes + c];
            pg.samples = planes == 3 ? (const void *)((int16_t *)l.planes.p + (j * planes + c) * pstride) : (const void *)m.px;
            pg.image = m.px;
            pg.W = m.w;
            pg.H = m.h;
            pg.npix = (uint32_t)m.npix;
            pg.ntiles = (uint32_t)((m.npix + PACK_TILE - 1) / PACK_TILE);
            pg.out_off = o.off[idx[j]];
            pg.out_slot = o.slot[idx[j]];
            if (any_view && planes == 1) h_pitched[j] = PitchedGeom{pg, m.pitch ? m.pitch : (uint64_t)m.w};  // (a dense plane: pitch = W)
        }
        if (any_view && planes == 3) h_views[j] = m.view ? m.vr : ViewRow{m.px, 3ll * m.w, 3, 1};
    }
    const size_t tbytes = (size_t)g.nplanes * sizeof(PlaneGeom) + (any_view ? (planes == 1 ? cnt * sizeof(PitchedGeom) : cnt * sizeof(ViewRow)) : 0);
    if ((rc = reserve(ctx, l.mtable, tbytes)) != 0) return rc;
    hipStream_t fs = ctx->serial ? l.stream : l.front;
    if ((rc = wait_ready(ctx, fs)) != 0) return rc;
    if (ctx->profiling) HIP_TRY(ctx, hipEventRecord(l.span_begin, fs));
    HIP_TRY(ctx, hipMemcpyAsync(l.mtable.p, l.h_table, tbytes, hipMemcpyHostToDevice, fs));
    g.mixed = (const PlaneGeom *)l.mtable.p;
    g.pitched = any_view && planes == 1 ? (const PitchedGeom *)((const uint8_t *)l.mtable.p + extra_off) : nullptr;
    l.d_planes = planes == 3 ? l.planes.p : nullptr;  // (gray: every plane's samples come from the table)
    if (planes == 3) {
        StageTimer t(ctx, l, ST_PLANES, fs, true);
        if (any_view)  // (views read where they lie, whatever their strides; the dense images of the sub-batch as views of their own)
            launch_rgb8_view_to_planes(fs, g.mixed, (const ViewRow *)((const uint8_t *)l.mtable.p + extra_off), pstride, (uint32_t)max_npix, (uint32_t)cnt);
        else
            launch_rgb8_to_planes_mixed(fs, g.mixed, pstride, (uint32_t)max_npix, (uint32_t)cnt);
    }
    return planes == 3 ? run_lane<int16_t, uint16_t>(ctx, l, o.base, 0) : run_lane<uint8_t, uint8_t>(ctx, l, o.base, 0);
}

// a view's dense copy in a mixed 16-bit job's part of mix_in: 256-byte steps
size_t gather_step(const MixImage &m) { return m.view ? (m.frame_bytes + 255) & ~(size_t)255 : 0; }

// Queues a mixed 16-bit sub-batch on lane l: run_wide on the padded geometry (npix = T_max * SORT_TILE: the stride of k_map and, RGB16, of
// the i32 planes) with the plane table.  gray16 frames are read where the caller has them, RGB16 frames by the plane transform; a
// view is gathered to `gathered` first (stage_frame: counted in bytes_staged) and its rows point there.  Everything on the lane's
// one stream, behind the caller's ready event.
int launch_mixed_wide(felics_ctx *ctx, Lane &l, const std::vector<MixImage> &im, const std::vector<size_t> &idx, const MixOut &o, uint8_t *gathered,
                      int nslices) {
    const MixImage &f = im[idx[0]];
    const uint32_t planes = f.planes;
    const size_t cnt = idx.size();
    uint32_t tmax = 0;
    uint64_t max_npix = 0;
    for (size_t i : idx) {
        tmax = std::max(tmax, sort_tiles_of(im[i].npix));
        max_npix = std::max(max_npix, im[i].npix);
    }
    l.nslices = std::max(1, std::min(nslices, SLICES));
    l.queued = true;
    ctx->stats.submissions++;
    for (int i = 0; i < ST_COUNT; i++) l.ev_used[i] = 0;
    Geometry &g = l.g;
    g.W = SORT_TILE;  // (the uniform fields describe the padded planes, as in launch_mixed)
    g.H = tmax;
    g.npix = tmax * SORT_TILE;
    g.nimages = (uint32_t)cnt;
    g.planes_per_image = planes;
    g.nplanes = (uint32_t)(cnt * planes);
    g.sort_tiles = tmax;
    g.pack_tiles = tmax;
    g.color = (uint32_t)f.color;
    g.depth = FELICS_DEPTH_16;
    g.nctx = planes == 3 ? nctx_of<int16_t>() : nctx_of<uint8_t>();  // (unused: run_wide has tables of its own)
    g.pitched = nullptr;
    l.first_image = 0;
    int rc;
    const uint64_t pstride = g.npix;
    if (planes == 3 && (rc = reserve(ctx, l.planes, (size_t)g.nplanes * pstride * 4 + STAGE_PAD)) != 0) return rc;
    if ((rc = reserve_table(ctx, l, g.nplanes)) != 0) return rc;
    const size_t tbytes = (size_t)g.nplanes * sizeof(PlaneGeom);
    if ((rc = reserve(ctx, l.mtable, tbytes)) != 0) return rc;
    hipStream_t s = l.stream;
    if ((rc = wait_ready(ctx, s)) != 0) return rc;
    if (ctx->profiling) HIP_TRY(ctx, hipEventRecord(l.span_begin, s));
    size_t at = 0;
    for (size_t j = 0; j < cnt; j++) {
        const MixImage &m = im[idx[j]];
        const uint8_t *frame = m.px;
        if (m.view) {
            frame = gathered + at;
            if ((rc = stage_frame(ctx, s, gathered + at, m)) != 0) return rc;
            at += gather_step(m);
        }
        for (uint32_t c = 0; c < planes; c++) {
            PlaneGeom &pg = l.h_table[j * planes + c];
            pg.samples = planes == 3 ? (const void *)((int32_t *)l.planes.p + (j * planes + c) * pstride) : (const void *)frame;
            pg.image = frame;
            pg.W = m.w;
            pg.H = m.h;
            pg.npix = (uint32_t)m.npix;
            pg.ntiles = (uint32_t)((m.npix + PACK_TILE - 1) / PACK_TILE);
            pg.out_off = o.off[idx[j]];
            pg.out_slot = o.slot[idx[j]];
        }
    }
    HIP_TRY(ctx, hipMemcpyAsync(l.mtable.p, l.h_table, tbytes, hipMemcpyHostToDevice, s));
    g.mixed = (const PlaneGeom *)l.mtable.p;
    l.d_planes = planes == 3 ? l.planes.p : nullptr;  // (the mixed kernels take every plane from the table)
    if (planes == 3) {
        StageTimer t(ctx, l, ST_PLANES, s, true);
        launch_rgb16_to_planes_mixed(s, g.mixed, (uint32_t)max_npix, (uint32_t)cnt);
    }
    return planes == 3 ? run_wide<int32_t>(ctx, l, o.base, 0) : run_wide<uint16_t>(ctx, l, o.base, 0);
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
            (m.w == f.w && m.h == f.h && m.color == f.color && m.depth == f.depth ? grp : other).push_back(i);
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
        if ((rc = encode_device(ctx, l, cnt, ctx->mix_redo.p, f.w, f.h, f.color, f.depth, nullptr, 0, offs.data(), lens.data(), &used)) != 0)
            return rc;
        for (size_t j = 0; j < cnt; j++) {
            const size_t i = grp[j];
            o.lens[i] = lens[j];
            if (lens[j] > o.slot[i]) {
                o.overflow = true;
                continue;
            }
            HIP_TRY(ctx, hipMemcpyAsync(o.base + o.off[i], used + offs[j], (size_t)lens[j], hipMemcpyDeviceToDevice, l.stream));
        }
        HIP_TRY(ctx, hipStreamSynchronize(l.stream));  // (ctx->own is reused by the next group)
    }
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
        if (so.overflow) {  // a stream outgrew its slot: the group again with exact placement (encode_device)
            ctx->stats.slot_overflows++;
            const MixImage &f = im[j.idx[0]];
            if ((rc = encode_device(ctx, l, cnt, (uint8_t *)ctx->mix_in.p + j.in_off, f.w, f.h, f.color, f.depth, nullptr, 0, offs.data(),
                                    lens.data(), &from, true)) != 0)
                return rc;
        }
        for (size_t k = 0; k < cnt; k++) {
            const size_t i = j.idx[k];
            o.lens[i] = lens[k];
            if (lens[k] > o.slot[i]) {
                o.overflow = true;
                continue;
            }
            HIP_TRY(ctx, hipMemcpyAsync(o.base + o.off[i], from + offs[k], (size_t)lens[k], hipMemcpyDeviceToDevice, l.stream));
        }
        HIP_TRY(ctx, hipStreamSynchronize(l.stream));
        collect_timing(ctx, l);
        return FELICS_OK;
    }
    if (j.wide_mixed) {  // (run_wide copies the sizes and nothing else: no error / flags word to read)
        bool overflow = false;
        for (size_t k = 0; k < cnt; k++) {
            const size_t i = j.idx[k];
            o.lens[i] = l.h_sizes[k];
            if (l.h_sizes[k] > o.slot[i]) overflow = true;
        }
        if (!overflow) {
            if (ctx->profiling && (rc = sync_lane(ctx, l)) != 0) return rc;  // (span_end is recorded behind `sized`)
            collect_timing(ctx, l);
            return FELICS_OK;
        }
        if ((rc = sync_lane(ctx, l)) != 0) return rc;
        ctx->stats.slot_overflows++;
        return redo_by_shape(ctx, l, im, j.idx, o);
    }
    const uint32_t err = (uint32_t)l.h_sizes[cnt], flags = (uint32_t)(l.h_sizes[cnt] >> 32);
    SlotOutcome so;
    so.lookback_failed = (err & 1u) != 0 || (ctx->test_lookback && l.m_fused);
    so.overflow = (err & 2u) != 0;
    so.order_violation = (flags & TL_FLAG_ORDER) != 0;
    so.tile_overflow = (flags & TL_FLAG_OVERFLOW) != 0;
    so.spine_error = (flags & TL_FLAG_SPINE) != 0;
    for (size_t k = 0; k < cnt; k++) {  // (the table lists the sub-batch's images in the order of j.idx)
        const size_t i = j.idx[k];
        o.lens[i] = l.h_sizes[k];
        if (l.h_sizes[k] > o.slot[i]) so.overflow = true;
    }
    if (!so.redo() && !so.overflow && !so.spine_error) {
        collect_timing(ctx, l);
        return FELICS_OK;
    }
    if ((rc = sync_lane(ctx, l)) != 0) return rc;
    if (so.spine_error) return spine_failure(ctx);
    if (so.order_violation)
        note_scatter_order_violation(ctx);
    else if (so.tile_overflow)
        note_tile_overflow(ctx);
    else if (so.lookback_failed)
        note_lookback_failure(ctx, l);
    else
        ctx->stats.slot_overflows++;
    return redo_by_shape(ctx, l, im, j.idx, o);
}

// Every image of the call into the slots of `o`: zero-sized images on the host path, the jobs queued over the lanes.
int run_images(felics_ctx *ctx, const std::vector<MixImage> &im, MixOut &o) {
    const size_t n = im.size();
    int rc;
    o.overflow = false;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    std::vector<MixJob> jobs;
    for (int color : {FELICS_COLOR_GRAY, FELICS_COLOR_RGB}) {  // 8-bit: buckets of similar tile counts
        std::vector<size_t> v;
        for (size_t i = 0; i < n; i++)
            if (im[i].npix && im[i].depth == FELICS_DEPTH_8 && im[i].color == color) v.push_back(i);
        std::stable_sort(v.begin(), v.end(), [&](size_t a, size_t b) { return sort_tiles_of(im[a].npix) < sort_tiles_of(im[b].npix); });
        for (size_t a = 0; a < v.size();) {
            const uint64_t tmin = sort_tiles_of(im[v[a]].npix), lim = (5 * tmin + 3) / 4;  // ceil(1.25 T_min)
            size_t b = a;
            while (b < v.size() && sort_tiles_of(im[v[b]].npix) <= lim) b++;
            const uint32_t planes = color == FELICS_COLOR_RGB ? 3 : 1;
            const size_t per = std::min(MIX_MAX_IMAGES, max_images_per_pass((uint64_t)sort_tiles_of(im[v[b - 1]].npix) * SORT_TILE, planes, FELICS_DEPTH_8));
            for (size_t c = a; c < b; c += per) {
                MixJob j;
                j.idx.assign(v.begin() + c, v.begin() + std::min(b, c + per));
                jobs.push_back(std::move(j));
            }
            a = b;
        }
    }
    size_t in_total = 0, stage_total = 0;
    // 16-bit: the same buckets.  One shape: the uniform path, frames gathered back to back; else a mixed 16-bit sub-batch.
    auto uniform_job = [&](std::vector<size_t> idx) {
        const MixImage &f = im[idx[0]];
        MixJob j;
        j.wide = true;
        j.idx = std::move(idx);
        j.slot = mix_slot(f.frame_bytes);
        j.in_off = in_total;
        j.stage_off = stage_total;
        in_total += ((f.frame_bytes * j.idx.size()) + 255) & ~(size_t)255;
        stage_total += (size_t)(j.slot * j.idx.size());
        jobs.push_back(std::move(j));
    };
    auto one_shape = [&](const size_t *first, const size_t *last) {
        for (const size_t *p = first; p != last; p++)
            if (im[*p].w != im[*first].w || im[*p].h != im[*first].h) return false;
        return true;
    };
    for (int color : {FELICS_COLOR_GRAY, FELICS_COLOR_RGB}) {
        std::vector<size_t> v;
        for (size_t i = 0; i < n; i++)
            if (im[i].npix && im[i].depth == FELICS_DEPTH_16 && im[i].color == color) v.push_back(i);
        std::stable_sort(v.begin(), v.end(), [&](size_t a, size_t b) { return sort_tiles_of(im[a].npix) < sort_tiles_of(im[b].npix); });
        const uint32_t planes = color == FELICS_COLOR_RGB ? 3 : 1;
        for (size_t a = 0; a < v.size();) {
            const uint64_t tmin = sort_tiles_of(im[v[a]].npix), lim = (5 * tmin + 3) / 4;  // ceil(1.25 T_min)
            size_t b = a;
            while (b < v.size() && sort_tiles_of(im[v[b]].npix) <= lim) b++;
            const bool uniform = one_shape(&v[a], &v[a] + (b - a));
            // The pass bound with the padded npix = T_max * SORT_TILE keeps planes * npix of a mixed sub-batch <= 2^30 samples, so the
            // chain kernels' 32-bit kbase = plane * npix (k_map is strided by the padded npix) stays valid.  (A bucket of one shape:
            // its own npix, the passes that shape always had.)
            const size_t per = uniform ? max_images_per_pass(im[v[a]].npix, planes, FELICS_DEPTH_16)
                                       : std::min(MIX_MAX_IMAGES, max_images_per_pass((uint64_t)sort_tiles_of(im[v[b - 1]].npix) * SORT_TILE, planes,
                                                                                      FELICS_DEPTH_16));
            for (size_t c = a; c < b; c += per) {
                const size_t e = std::min(b, c + per);
                if (uniform || one_shape(&v[c], &v[c] + (e - c))) {
                    uniform_job(std::vector<size_t>(v.begin() + c, v.begin() + e));
                    continue;
                }
                MixJob j;
                j.wide_mixed = true;
                j.idx.assign(v.begin() + c, v.begin() + e);
                j.in_off = in_total;
                for (size_t i : j.idx) in_total += gather_step(im[i]);
                jobs.push_back(std::move(j));
            }
            a = b;
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
    }
    const int nslices = jobs.size() > 1 ? ctx->slices_queued : ctx->slices_blocking;
    std::vector<size_t> flying;  // jobs in flight, oldest first (lanes handed out in turn: the oldest holds the next lane)
    auto drain = [&](int r) {
        for (size_t f : flying) {
            (void)wait_event(ctx, ctx->lanes[jobs[f].lane].sized, "stream sizes");
            (void)sync_lane(ctx, ctx->lanes[jobs[f].lane]);
        }
        return r;
    };
    for (size_t q = 0; q < jobs.size(); q++) {
        if ((int)flying.size() == ctx->nlanes) {
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
            if ((rc = redo_by_shape(ctx, ctx->lanes[ctx->next_lane], im, j.idx, o)) != 0) return rc;
            continue;
        }
        j.lane = ctx->next_lane;
        Lane &l = ctx->lanes[j.lane];
        ctx->next_lane = (ctx->next_lane + 1) % ctx->nlanes;
        if (j.wide) {
            const MixImage &f = im[j.idx[0]];
            uint8_t *in = (uint8_t *)ctx->mix_in.p + j.in_off;
            if ((rc = wait_ready(ctx, l.stream)) != 0) return drain(rc);
            for (size_t k = 0; k < j.idx.size(); k++)  // (a view is gathered by a kernel instead of copied)
                if ((rc = stage_frame(ctx, l.stream, in + k * f.frame_bytes, im[j.idx[k]])) != 0) return drain(rc);
            for (int i = 0; i < ST_COUNT; i++) l.ev_used[i] = 0;
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
int images_device(felics_ctx *ctx, const std::vector<MixImage> &im, uint8_t *d_out, size_t d_out_cap, uint64_t *offsets, uint64_t *lens) {
    const size_t n = im.size();
    std::vector<uint64_t> off(n), slot(n);
    uint64_t total = 0;
    for (size_t i = 0; i < n; i++) {
        slot[i] = mix_slot(im[i].frame_bytes);
        off[i] = total;
        total += slot[i];
    }
    MixOut o{d_out, off.data(), slot.data(), lens, false};
    int rc;
    if (total > d_out_cap) {  // the sizes first, into a buffer of the library's own
        if ((rc = reserve(ctx, ctx->mix_out, (size_t)total + 64)) != 0) return rc;
        o.base = (uint8_t *)ctx->mix_out.p;
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
    if ((rc = run_images(ctx, im, o)) != 0) return rc;
    if (o.overflow) {
        ctx->err = "internal error: a stream outgrew the exact size it had before";
        return FELICS_E_HIP;
    }
    for (size_t i = 0; i < n; i++) offsets[i] = off[i];
    return FELICS_OK;
}

// ---- GPU decoder helpers shared by felics_decompress_batch_device and felics_decompress_images_device -----------------------

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
        if (table_bytes > ctx->dec_table.cap) ctx->dec_epoch = 0;  // a fresh (zeroed) buffer: epochs start over
        const int rc = reserve_zeroed(ctx, ctx->dec_table, table_bytes);
        if (rc == 0) return FELICS_OK;
        (void)hipGetLastError();
        if (per == 1) return rc;
        per = (per + 1) / 2;
    }
}

// the first of the three epochs (one per plane) of the next pass on stream s
int dec16_epoch(felics_ctx *ctx, hipStream_t s, uint32_t &epoch0) {
    if (ctx->dec_epoch > 0xFFFFFFF0u) {  // epochs used up: clear the tables, start over
        HIP_TRY(ctx, hipMemsetAsync(ctx->dec_table.p, 0, ctx->dec_table.cap, s));
        ctx->dec_epoch = 0;
    }
    epoch0 = ctx->dec_epoch + 1;
    ctx->dec_epoch += 3;
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
        if (bytes > ctx->dec_lane16_table.cap) ctx->dec_lane16_epoch = 0;  // a fresh (zeroed) buffer: epochs start over
        const int rc = reserve_zeroed(ctx, ctx->dec_lane16_table, bytes);
        if (rc == 0) return FELICS_OK;
        (void)hipGetLastError();
        if (bytes <= least) return rc;
        bytes = std::max(least, bytes / 2);
    }
}

// the first of the three epochs (one per plane) of the next lane-form launch on stream s
int dec16_lanes_epoch(felics_ctx *ctx, hipStream_t s, uint32_t &epoch0) {
    if (ctx->dec_lane16_epoch + 3 > DEC16L_EPOCH_MAX) {  // epochs used up: clear the tables, start over
        HIP_TRY(ctx, hipMemsetAsync(ctx->dec_lane16_table.p, 0, ctx->dec_lane16_table.cap, s));
        ctx->dec_lane16_epoch = 0;
    }
    epoch0 = ctx->dec_lane16_epoch + 1;
    ctx->dec_lane16_epoch += 3;
    return FELICS_OK;
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
int decompress_images(felics_ctx *ctx, size_t n, const void *d_streams, const uint64_t *offsets, const uint64_t *lens, uint8_t *d_pixels,
                      size_t cap, uint64_t *pix_offsets, felics_header *hdrs, int *status) {
    Lane &l0 = ctx->lanes[0];
    hipStream_t s = l0.stream;
    felics_decode_stats &ds = ctx->dstats;
    ds.streams += n;
    ds.lanes16_table_bytes = 0;
    auto fail_all = [&](int code) {
        for (size_t i = 0; i < n; i++) status[i] = code;
        ds.undecoded += n;
        return code;
    };
    std::vector<DecodeHeader> rec;
    int rc = read_headers(ctx, n, d_streams, offsets, lens, rec, s);
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
    std::vector<size_t> wave8, rows16, host;
    size_t n8 = 0;
    for (size_t i = 0; i < n; i++) {
        const DecodeHeader &h = rec[i];
        if (status[i] != FELICS_OK) continue;
        if (!h.depth && decode8_lds_bytes(h.W, h.color) <= DECODE_LDS_LIMIT) n8++;
        else if (h.depth && decode16_lds_bytes(h.W) <= DECODE_LDS_LIMIT) rows16.push_back(i);
        else host.push_back(i);
    }
    // lane groups: 8-bit GPU streams of one shape, in stream order within a group
    std::vector<std::vector<size_t>> lane_groups[2];  // [colour]
    {
        std::vector<size_t> idx8;
        for (size_t i = 0; i < n; i++)
            if (status[i] == FELICS_OK && !rec[i].depth && decode8_lds_bytes(rec[i].W, rec[i].color) <= DECODE_LDS_LIMIT) idx8.push_back(i);
        std::stable_sort(idx8.begin(), idx8.end(), [&](size_t a, size_t b) {
            return std::make_tuple(rec[a].color, rec[a].W, rec[a].H) < std::make_tuple(rec[b].color, rec[b].W, rec[b].H);
        });
        for (size_t k = 0; k < idx8.size();) {
            size_t e = k;
            while (e < idx8.size() && rec[idx8[e]].color == rec[idx8[k]].color && rec[idx8[e]].W == rec[idx8[k]].W && rec[idx8[e]].H == rec[idx8[k]].H) e++;
            const DecodeHeader &h = rec[idx8[k]];
            const size_t cnt = e - k;
            size_t take = 0;
            if (h.W >= 8) {
                if (forced >= 0) take = forced ? cnt : 0;
                else if (n8 >= (h.color ? DECODE8_LANES_MIN_STREAMS_RGB : DECODE8_LANES_MIN_STREAMS)) take = cnt / 64 * 64;
            }
            if (take) lane_groups[h.color].emplace_back(idx8.begin() + k, idx8.begin() + k + take);
            wave8.insert(wave8.end(), idx8.begin() + k + take, idx8.begin() + e);
            k = e;
        }
    }
    // 16-bit lane groups: whole waves of 64 streams of one shape and colour, W >= 8, in a call with as many 16-bit GPU streams as the
    // same-shape entry point wants for that form (FELICS_TEST_DECODE16_LANES=1: in any call; =0: none); the rest of a group and
    // every other 16-bit stream keep the wave form
    std::vector<std::vector<size_t>> lane16_groups[2];  // [colour]
    const int forced16 = dec16_lanes_forced();
    if (forced16 != 0 && rows16.size() >= 64) {
        std::vector<size_t> idx16 = rows16, rest;
        std::stable_sort(idx16.begin(), idx16.end(), [&](size_t a, size_t b) {
            return std::make_tuple(rec[a].color, rec[a].W, rec[a].H) < std::make_tuple(rec[b].color, rec[b].W, rec[b].H);
        });
        for (size_t k = 0; k < idx16.size();) {
            size_t e = k;
            while (e < idx16.size() && rec[idx16[e]].color == rec[idx16[k]].color && rec[idx16[e]].W == rec[idx16[k]].W && rec[idx16[e]].H == rec[idx16[k]].H) e++;
            const DecodeHeader &h = rec[idx16[k]];
            size_t take = 0;
            if (h.W >= 8 && (forced16 == 1 || rows16.size() >= (h.color ? DECODE16_LANES_MIN_STREAMS_RGB : DECODE16_LANES_MIN_STREAMS)))
                take = (e - k) / 64 * 64;
            if (take) lane16_groups[h.color].emplace_back(idx16.begin() + k, idx16.begin() + k + take);
            rest.insert(rest.end(), idx16.begin() + k + take, idx16.begin() + e);
            k = e;
        }
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
    struct Launch {
        size_t first, cnt;
        uint32_t lds;
        uint64_t max_npix;
        bool rgb;
    };
    std::vector<Launch> classes;
    for (int c = 0; c < NCLASS; c++) {
        Launch L{rows.size(), 0, 0, 0, false};
        for (size_t i : wave8) {
            const uint32_t lds = decode8_lds_bytes(rec[i].W, rec[i].color);
            if (lds > LDS_CLASS[c] || (c > 0 && lds <= LDS_CLASS[c - 1])) continue;
            const uint64_t poff = rec[i].color ? plane8_of(i) : 0;
            rows.push_back(DecodeRow{(uint32_t)i, rec[i].W, rec[i].H, rec[i].color, pix_offsets[i], poff});
            L.cnt++;
            L.lds = std::max(L.lds, lds);
            L.max_npix = std::max(L.max_npix, npix[i]);
            L.rgb = L.rgb || rec[i].color;
        }
        if (L.cnt) classes.push_back(L);
    }
    // lane form: waves of up to 64 slots of one shape; gray slots first, then RGB (each colour one launch, its tables behind the other's)
    std::vector<LaneWave> waves;
    std::vector<LaneSlot> slots;
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
                    slots.push_back(LaneSlot{(uint32_t)i, 0, col ? poff : pix_offsets[i]});
                    if (col) {
                        if (!conv.cnt) conv.first = rows.size();
                        rows.push_back(DecodeRow{(uint32_t)i, rec[i].W, rec[i].H, 1, pix_offsets[i], poff});
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
                        slots.push_back(LaneSlot{(uint32_t)i, (uint32_t)used_rows, col ? poff : pix_offsets[i] / 2});
                        if (col) {
                            rows.push_back(DecodeRow{(uint32_t)i, rec[i].W, rec[i].H, 1, pix_offsets[i], poff});
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
                rows.push_back(DecodeRow{(uint32_t)i, rec[i].W, rec[i].H, rec[i].color, pix_offsets[i], poff});
                if (rec[i].color) poff += 3 * npix[i];
            }
            planes16 = std::max(planes16, poff);
        }
    }
    // device side: offsets | lens | status | rows | waves | slots (offsets and lens again: the buffer may have moved)
    auto al = [](size_t b) { return (b + 15) & ~(size_t)15; };
    const size_t o_status = n * 16, o_rows = o_status + al(n * 4), o_waves = o_rows + al(rows.size() * sizeof(DecodeRow)),
                 o_slots = o_waves + al(waves.size() * sizeof(LaneWave)), o_end = o_slots + slots.size() * sizeof(LaneSlot);
    if ((rc = reserve(ctx, ctx->dec_meta, o_end)) != 0) return fail_all(rc);
    uint8_t *meta = (uint8_t *)ctx->dec_meta.p;
    uint64_t *d_off = (uint64_t *)meta, *d_len = d_off + n;
    int *d_status = (int *)(meta + o_status);
    DecodeRow *d_rows = (DecodeRow *)(meta + o_rows);
    LaneWave *d_waves = (LaneWave *)(meta + o_waves);
    LaneSlot *d_slots = (LaneSlot *)(meta + o_slots);
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
                for (size_t k = p; k < p + cnt; k++) {
                    const size_t i = rows16[k];
                    lds = std::max(lds, decode16_lds_bytes(rec[i].W));
                    mx = std::max(mx, npix[i]);
                    rgb = rgb || rec[i].color;
                }
                int r = dec16_epoch(ctx, w, epoch0);
                if (r) return r;
                HIP_TRY(ctx, launch_decode16_rows(w, st, d_off, d_len, d_rows + rows16_first + p, (uint32_t)cnt, lds, mx, rgb, (uint16_t *)d_pixels,
                                                  (int32_t *)ctx->dec_planes16.p, (uint32_t *)ctx->dec_table.p, epoch0, d_status));
            }
        }
        if (nslots8) {
            hipStream_t w = stream_for();
            HIP_TRY(ctx, hipMemsetAsync(ctx->dec_lane_table.p, 0, lt_bytes, w));
            for (int col = 0; col < 2; col++)
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
                HIP_TRY(ctx, launch_decode16_lanes_waves(w, st, d_off, d_len, d_waves + P.wave_first, (uint32_t)P.wave_cnt, d_slots + P.slot_first, P.col,
                                                         d_rows + P.conv_first, (uint32_t)P.conv_cnt, P.max_npix, (uint16_t *)d_pixels,
                                                         (int32_t *)ctx->dec_planes16.p, (uint32_t *)ctx->dec_lane16_table.p, epoch0, d_status));
            }
        }
        for (const Launch &L : classes)
            HIP_TRY(ctx, launch_decode8_rows(stream_for(), st, d_off, d_len, d_rows + L.first, (uint32_t)L.cnt, L.lds, L.max_npix, L.rgb, d_pixels,
                                             (int16_t *)ctx->dec_planes.p, d_status));
        // the host decoder meanwhile (into frames no kernel writes)
        std::vector<uint8_t> sbuf, pbuf;
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

}  // namespace

// --------------------------------------------------------------------------------------------
// C ABI
// --------------------------------------------------------------------------------------------

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
    if (const char *e = getenv("FELICS_SLICES")) ctx->slices_blocking = std::max(1, std::min(atoi(e), SLICES));
    if (const char *e = getenv("FELICS_SLICES_QUEUED")) ctx->slices_queued = std::max(1, std::min(atoi(e), SLICES));  // (tuning sweeps: profiles/tools/sweep_queue.sh)
    ctx->trace = getenv("FELICS_TRACE") != nullptr;
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
        // out their tiles by ticket (FusedArgs::ticket), it just is not faster.
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
                          &l.partial, &l.status, &l.edge_first, &l.edge_last, &l.pscratch, &l.wrecs[0], &l.wrecs[1], &l.wtile_cnt, &l.wmeta, &l.whist, &l.wdigtot, &l.heads, &l.wlong};
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
    release(ctx->view_stage);
    release(ctx->dec_meta);
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

int felics_compress_batch_device(felics_ctx *ctx, size_t n, const void *d_pixels, uint32_t w, uint32_t h, int color,
                                 int depth, void *d_out, size_t d_out_cap, uint64_t *offsets, uint64_t *lens) {
    if (!ctx || !offsets || !lens || !d_out || (!d_pixels && n && (uint64_t)w * h)) return FELICS_E_INVALID_ARGUMENT;
    if (ctx->failed) return FELICS_E_HIP;
    int rc = check_args(w, h, color, depth);
    if (rc) return rc;
    if (n == 0) return FELICS_OK;
    if (any_pending(ctx)) return FELICS_E_INVALID_ARGUMENT;  // felics_wait_batch first
    return encode_device(ctx, ctx->lanes[0], n, d_pixels, w, h, color, depth, (uint8_t *)d_out, d_out_cap, offsets, lens,
                         nullptr);
}

int felics_submit_batch_device(felics_ctx *ctx, size_t n, const void *d_pixels, uint32_t w, uint32_t h, int color,
                               int depth, void *d_out, size_t d_out_cap, int *ticket) {
    if (!ctx || !ticket || !d_out || n == 0 || (!d_pixels && (uint64_t)w * h)) return FELICS_E_INVALID_ARGUMENT;
    if (ctx->failed) return FELICS_E_HIP;
    int rc = check_args(w, h, color, depth);
    if (rc) return rc;
    const int L = ctx->next_lane;
    Lane &l = ctx->lanes[L];
    if (l.pending) return FELICS_E_INVALID_ARGUMENT;  // MAX_LANES submissions are in flight: wait for the oldest
    l.p_n = n;
    l.p_pixels = d_pixels;
    l.p_w = w;
    l.p_h = h;
    l.p_color = color;
    l.p_depth = depth;
    l.p_out = (uint8_t *)d_out;
    l.p_cap = d_out_cap;
    l.finished = false;
    const uint32_t planes = color == FELICS_COLOR_RGB ? 3 : 1;
    const uint64_t npix = (uint64_t)w * h;
    const size_t frame_bytes = (size_t)npix * planes * (depth == FELICS_DEPTH_16 ? 2 : 1);
    uint64_t slot = (d_out_cap / n) & ~15ull;
    if (slot < 64 || slot < frame_bytes / 4) slot = 0;
    if (npix == 0 || npix * planes >= 0xE0000000ull || n > max_images_per_pass(npix, planes, depth) || slot == 0) {
        // not the plain case (fixed slots, one pass): do it now, hand the result over at the wait
        l.r_off.assign(n, 0);
        l.r_len.assign(n, 0);
        l.r_rc = encode_device(ctx, l, n, d_pixels, w, h, color, depth, l.p_out, d_out_cap, l.r_off.data(), l.r_len.data(),
                               nullptr);
        l.finished = true;
    } else {
        HIP_TRY(ctx, hipSetDevice(ctx->device));
        for (int i = 0; i < ST_COUNT; i++) l.ev_used[i] = 0;
        l.p_slot = slot;
        if ((rc = launch_sub_batch(ctx, l, 0, n, d_pixels, w, h, color, depth, l.p_out, slot, ctx->slices_queued, true)) != 0) {
            (void)sync_lane(ctx, l);
            return rc;
        }
    }
    l.pending = true;
    *ticket = L;
    ctx->next_lane = (L + 1) % ctx->nlanes;
    return FELICS_OK;
}

int felics_wait_batch(felics_ctx *ctx, int ticket, uint64_t *offsets, uint64_t *lens) {
    if (!ctx || ticket < 0 || ticket >= ctx->nlanes || !offsets || !lens) return FELICS_E_INVALID_ARGUMENT;
    if (ctx->failed) return FELICS_E_HIP;
    Lane &l = ctx->lanes[ticket];
    if (!l.pending) return FELICS_E_INVALID_ARGUMENT;
    if (!l.finished) {
        // the lane stays marked busy until its kernels are known to have finished: after a timeout nothing may
        // reuse or free its workspace
        const int wrc = wait_event(ctx, l.sized, "stream sizes");
        if (wrc) return wrc;
    }
    l.pending = false;
    if (l.finished) {
        for (size_t i = 0; i < l.p_n; i++) {
            offsets[i] = l.r_off[i];
            lens[i] = l.r_len[i];
        }
        return l.r_rc;
    }
    int rc;
    const SlotOutcome o = read_sizes(ctx, l, l.p_depth == FELICS_DEPTH_16, l.p_slot, offsets, lens);
    if (!o.redo() && !o.overflow && !o.spine_error) {
        collect_timing(ctx, l);
        return FELICS_OK;
    }
    // the rare cases: pack again on this lane, synchronously (two-pass kernels / exact placement)
    if ((rc = sync_lane(ctx, l)) != 0) return rc;
    if (o.spine_error) return spine_failure(ctx);
    if (o.order_violation) {
        note_scatter_order_violation(ctx);
    } else if (o.tile_overflow) {
        note_tile_overflow(ctx);
    } else if (o.lookback_failed) {
        note_lookback_failure(ctx, l);
    } else {
        ctx->stats.slot_overflows++;
    }
    return encode_device(ctx, l, l.p_n, l.p_pixels, l.p_w, l.p_h, l.p_color, l.p_depth, l.p_out, l.p_cap, offsets, lens,
                         nullptr, o.overflow && !o.redo());
}

// The reference's own call shape: images in host memory in, .felics bytes in host memory out (compression.rs:255-282, :322-371;
// cfelics.rs:24-31).  The batch goes through the submission queue in CHUNKS: the frames of chunk c + 1 are copied to the device
// on a copy stream of its own while chunk c is encoded and the streams of chunk c - 1 are copied back on a third stream, so the
// link is busy in both directions under the kernels (measured, 64 4K gray8 frames from and to page-locked memory: 13.8 ms per
// batch; with the copies on the lanes' own streams 15.6).  (The copies are hipMemcpyAsync from / to the caller's pointers: at the
// link's rate, and asynchronous, if that memory is page-locked -- hipHostMalloc, hipHostRegister, a pinned torch tensor -- and
// through the runtime's staging otherwise.)  A chunk whose streams outgrow their slots and the room the slots leave for exact
// placement is encoded once more, blocking, into a buffer that grows.
int felics_compress_batch(felics_ctx *ctx, size_t n, const void *const *pixels, uint32_t w, uint32_t h, int color,
                          int depth, uint8_t *const *outs, const size_t *caps, size_t *lens) {
    if (!ctx || (n && (!pixels || !outs || !caps || !lens))) return FELICS_E_INVALID_ARGUMENT;
    if (ctx->failed) return FELICS_E_HIP;
    int rc = check_args(w, h, color, depth);
    if (rc) return rc;
    if (n == 0) return FELICS_OK;
    if (any_pending(ctx)) return FELICS_E_INVALID_ARGUMENT;  // felics_wait_batch first
    const uint32_t planes = color == FELICS_COLOR_RGB ? 3 : 1;
    const size_t frame_bytes = (size_t)w * h * planes * (depth == FELICS_DEPTH_16 ? 2 : 1);
    for (size_t i = 0; i < n && frame_bytes; i++)
        if (!pixels[i]) return FELICS_E_INVALID_ARGUMENT;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    if (!ctx->copy_in) {
        HIP_TRY(ctx, hipStreamCreateWithFlags(&ctx->copy_in, hipStreamNonBlocking));
        HIP_TRY(ctx, hipStreamCreateWithFlags(&ctx->copy_out, hipStreamNonBlocking));
    }
    const size_t per_pass = max_images_per_pass((uint64_t)w * h, planes, depth);
    // chunks: eight per batch (the first chunk's way in and the last one's way out are what the kernels cannot cover), none larger
    // than a pass; a stream's slot as encode_device sizes it
    const size_t chunk = std::max<size_t>(1, std::min(per_pass, (n + 7) / 8));
    const uint64_t slot = ((uint64_t)frame_bytes + frame_bytes / 4 + 64 + 15) & ~15ull;
    if ((rc = reserve(ctx, ctx->in, frame_bytes * n + 64)) != 0) return rc;
    if ((rc = reserve(ctx, ctx->out, (size_t)(slot * n) + 64)) != 0) return rc;
    struct Flying {
        int ticket;
        size_t first, cnt;
    };
    std::vector<Flying> flying;
    std::vector<uint64_t> offs(chunk), sizes(chunk);
    int result = FELICS_OK;
    auto land = [&](const Flying &f) -> int {  // wait for a chunk and start its streams on their way to the caller
        int r = felics_wait_batch(ctx, f.ticket, offs.data(), sizes.data());
        const uint8_t *from = (const uint8_t *)ctx->out.p + f.first * slot;
        hipStream_t cs = ctx->copy_out;
        if (r == FELICS_E_BUFFER_TOO_SMALL) {
            // The chunk's streams outgrew their slots AND the room the slots leave for exact placement (16-bit noise: a code can be
            // 2^17 bits): once more, blocking, into a buffer of the library's own that grows to what the streams need.
            Lane &l = ctx->lanes[f.ticket];
            uint8_t *d_own = nullptr;
            r = encode_device(ctx, l, f.cnt, (const uint8_t *)ctx->in.p + f.first * frame_bytes, w, h, color, depth, nullptr, 0, offs.data(),
                              sizes.data(), &d_own);
            from = d_own;
            cs = l.stream;  // (copied out before anything else may touch ctx->own: synchronised below)
        }
        if (r) return r;
        for (size_t i = 0; i < f.cnt; i++) {
            lens[f.first + i] = (size_t)sizes[i];
            if (sizes[i] > caps[f.first + i] || !outs[f.first + i]) {
                result = FELICS_E_BUFFER_TOO_SMALL;  // lens[] still reports every size needed
                continue;
            }
            HIP_TRY(ctx, hipMemcpyAsync(outs[f.first + i], from + offs[i], (size_t)sizes[i], hipMemcpyDeviceToHost, cs));
        }
        if (from != (const uint8_t *)ctx->out.p + f.first * slot) HIP_TRY(ctx, hipStreamSynchronize(cs));
        return FELICS_OK;
    };
    auto drain = [&](int r) {  // an error: nothing of this context may be left in flight behind the caller's back
        for (const Flying &f : flying) (void)felics_wait_batch(ctx, f.ticket, offs.data(), sizes.data());
        (void)hipStreamSynchronize(ctx->copy_in);
        (void)hipStreamSynchronize(ctx->copy_out);
        return r;
    };
    // All frames are put on their way at once, chunk by chunk with an event behind each chunk: the copy stream then runs back to
    // back at the link's rate whatever the host is waiting for (with a chunk's copies queued only when its turn came, the stream
    // stood idle while the host waited for an older chunk's kernels: 35 GB/s instead of the link's ~50).
    // All frames are put on their way at once, chunk by chunk with an event behind each chunk: the copy stream then runs back to
    // back at the link's rate whatever the host is waiting for (with a chunk's copies queued only when its turn came, the stream
    // stood idle while the host waited for an older chunk's kernels: 35 GB/s instead of the link's ~50).
    // (Eight chunks of a 64-frame batch: a chunk's kernels take ~2 ms whatever its size -- the chain of a single frame -- so with two
    // chunks in flight sixteen chunks are 16 ms of kernels, four leave the first and the last chunk's 2.5 ms of copying uncovered;
    // a short last chunk changed nothing: profiles/r05/experiments.txt.)
    std::vector<size_t> starts;
    for (size_t first = 0; first < n; first += chunk) starts.push_back(first);
    const size_t nchunks = starts.size();
    starts.push_back(n);
    while (ctx->h2d_done.size() < nchunks) {
        hipEvent_t ev = nullptr;
        HIP_TRY(ctx, hipEventCreateWithFlags(&ev, hipEventDisableTiming));
        ctx->h2d_done.push_back(ev);
    }
    for (size_t c = 0; c < nchunks; c++) {
        const size_t first = starts[c], cnt = starts[c + 1] - first;
        for (size_t i = 0; i < cnt && frame_bytes; i++) {
            const hipError_t e = hipMemcpyAsync((uint8_t *)ctx->in.p + (first + i) * frame_bytes, pixels[first + i], frame_bytes,
                                                hipMemcpyHostToDevice, ctx->copy_in);
            if (e != hipSuccess) return drain(hip_fail(ctx, e, "copying frames to the device"));
        }
        if (hipEventRecord(ctx->h2d_done[c], ctx->copy_in) != hipSuccess) return drain(hip_fail(ctx, hipGetLastError(), "hipEventRecord"));
    }
    for (size_t c = 0; c < nchunks; c++) {
        const size_t first = starts[c], cnt = starts[c + 1] - first;
        if ((int)flying.size() == ctx->nlanes) {  // every lane is busy: the oldest chunk first (its lane is the next to be used)
            rc = land(flying.front());
            flying.erase(flying.begin());
            if (rc) return drain(rc);
        }
        ctx->wait_before_submit = ctx->h2d_done[c];  // the chunk's first kernel waits for its frames (launch_sub_batch)
        int ticket = -1;
        rc = felics_submit_batch_device(ctx, cnt, (const uint8_t *)ctx->in.p + first * frame_bytes, w, h, color, depth,
                                        (uint8_t *)ctx->out.p + first * slot, (size_t)(slot * cnt), &ticket);
        ctx->wait_before_submit = nullptr;
        if (rc) return drain(rc);
        flying.push_back(Flying{ticket, first, cnt});
    }
    while (!flying.empty()) {
        rc = land(flying.front());
        flying.erase(flying.begin());
        if (rc) return drain(rc);
    }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->copy_out));  // the streams have landed
    return result;
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

namespace {

// A view's checks (felics_view_extent and felics_compress_views_device alike) and the hull of its samples' bytes relative to data.
int check_view(const felics_view &v, int64_t &lo, int64_t &hi) {
    lo = hi = 0;
    int rc = check_args(v.width, v.height, v.color, v.depth);
    if (rc) return rc;
    const uint64_t npix = (uint64_t)v.width * v.height;
    const uint32_t planes = v.color == FELICS_COLOR_RGB ? 3 : 1;
    const int bytes = v.depth == FELICS_DEPTH_16 ? 2 : 1;
    if (!v.data && npix) return FELICS_E_INVALID_ARGUMENT;
    if (bytes == 2 && (((uintptr_t)v.data | (uint64_t)v.row_stride | (uint64_t)v.pixel_stride | (planes == 3 ? (uint64_t)v.channel_stride : 0u)) & 1u))
        return FELICS_E_INVALID_ARGUMENT;
    if (npix * planes >= 0xE0000000ull) return FELICS_E_UNSUPPORTED;
    if (v.depth == FELICS_DEPTH_16 && npix > WIDE_MAX_PLANE_PIXELS) return FELICS_E_UNSUPPORTED;
    if (!npix) return FELICS_OK;
    __int128 l = 0, h = bytes;
    const int64_t steps[3] = {(int64_t)v.height - 1, (int64_t)v.width - 1, (int64_t)planes - 1};
    const int64_t strides[3] = {v.row_stride, v.pixel_stride, planes == 3 ? v.channel_stride : 0};
    for (int d = 0; d < 3; d++) {
        const __int128 span = (__int128)steps[d] * strides[d];
        (span < 0 ? l : h) += span;
    }
    if (l < INT64_MIN || h > INT64_MAX) return FELICS_E_INVALID_ARGUMENT;  // (addresses are computed in 64 bits)
    lo = (int64_t)l;
    hi = (int64_t)h;
    return FELICS_OK;
}

}  // namespace

int felics_view_extent(const felics_view *v, int64_t *lo, int64_t *hi) {
    if (!v || !lo || !hi) return FELICS_E_INVALID_ARGUMENT;
    return check_view(*v, *lo, *hi);
}

int felics_get_decode_stats(const felics_ctx *ctx, felics_decode_stats *out, size_t out_size) {
    if (!ctx || !out) return FELICS_E_INVALID_ARGUMENT;
    memcpy(out, &ctx->dstats, std::min(out_size, sizeof(felics_decode_stats)));
    return FELICS_OK;
}

uint32_t felics_decode_lanes_min_streams(int depth, int color) {
    if (depth) return color ? DECODE16_LANES_MIN_STREAMS_RGB : DECODE16_LANES_MIN_STREAMS;
    return color ? DECODE8_LANES_MIN_STREAMS_RGB : DECODE8_LANES_MIN_STREAMS;
}

int felics_get_view_stats(const felics_ctx *ctx, felics_view_stats *out, size_t out_size) {
    if (!ctx || !out) return FELICS_E_INVALID_ARGUMENT;
    memcpy(out, &ctx->vstats, std::min(out_size, sizeof(felics_view_stats)));
    return FELICS_OK;
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
        Lane &l = ctx->lanes[0];
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
    ctx->vstats.views += add.views;
    ctx->vstats.dense += add.dense;
    ctx->vstats.in_place += add.in_place;
    ctx->vstats.gathered += add.gathered;
    return leave(images_device(ctx, im, (uint8_t *)d_out, d_out_cap, offsets, lens));
}

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
        out_total += mix_slot(im[i].frame_bytes);
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

int felics_compress(felics_ctx *ctx, const void *pixels, uint32_t w, uint32_t h, int color, int depth, uint8_t *out,
                    size_t cap, size_t *out_len) {
    if (!out_len) return FELICS_E_INVALID_ARGUMENT;
    const void *px[1] = {pixels};
    uint8_t *outs[1] = {out};
    size_t caps[1] = {cap};
    size_t lens[1] = {0};
    if (!pixels && (uint64_t)w * h != 0) return FELICS_E_INVALID_ARGUMENT;
    static const uint8_t dummy = 0;
    if (!pixels) px[0] = &dummy;
    int rc = felics_compress_batch(ctx, 1, px, w, h, color, depth, outs, caps, lens);
    *out_len = lens[0];
    return rc;
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
    // every stream gets a status on every path out of here (felics.h): a call that ends before the streams are decoded
    // reports its own error for all of them
    felics_decode_stats &ds = ctx->dstats;
    ds.streams += n;
    ds.lanes16_table_bytes = 0;
    auto fail_all = [&](int code) {
        for (size_t i = 0; i < n; i++) status[i] = code;
        ds.undecoded += n;
        return code;
    };
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
        if ((rc = reserve(ctx, ctx->dec_meta, most * 8 * 2 + most * 4)) != 0) return fail_all(rc);
        int32_t *d_planes32 = nullptr;
        if (planes == 3) {
            if ((rc = reserve(ctx, ctx->dec_planes, (size_t)(npix * 3 * 4 * most) + 64)) != 0) return fail_all(rc);
            d_planes32 = (int32_t *)ctx->dec_planes.p;
        }
        ds.lanes16 += n;
        ds.lanes16_table_bytes = most * tb1;
        hipStream_t s = l.stream;
        for (size_t i = 0; i < n; i++) status[i] = FELICS_E_HIP;  // until the kernel's own word arrives
        int first_rc = FELICS_OK;
        for (size_t first = 0; first < n; first += per) {
            const size_t cnt = std::min(per, n - first);
            uint32_t epoch0 = 0;
            if ((rc = dec16_lanes_epoch(ctx, s, epoch0)) != 0) return rc;
            uint64_t *d_off = (uint64_t *)ctx->dec_meta.p, *d_len = d_off + cnt;
            int *d_status = (int *)(d_len + cnt);
            HIP_TRY(ctx, hipMemcpyAsync(d_off, offsets + first, cnt * 8, hipMemcpyHostToDevice, s));
            HIP_TRY(ctx, hipMemcpyAsync(d_len, lens + first, cnt * 8, hipMemcpyHostToDevice, s));
            HIP_TRY(ctx, hipMemsetAsync(d_status, 0xFF, cnt * 4, s));
            HIP_TRY(ctx, launch_decode16_lanes(s, (const uint8_t *)d_streams, d_off, d_len, (uint32_t)cnt, hdr.width, hdr.height, hdr.color_type,
                                               (uint16_t *)d_pixels + first * (frame_bytes / 2), d_planes32,
                                               (uint32_t *)ctx->dec_lane16_table.p, epoch0, d_status));
            HIP_TRY(ctx, hipMemcpyAsync(status + first, d_status, cnt * 4, hipMemcpyDeviceToHost, s));
            HIP_TRY(ctx, hipStreamSynchronize(s));
            for (size_t i = first; i < first + cnt && !first_rc; i++)
                if (status[i]) first_rc = status[i];
        }
        return first_rc;
    }
    if (bps == 2 && decode16_lds_bytes(hdr.width) <= DECODE_LDS_LIMIT) {
        // 16-bit streams on the device: passes of at most DEC16_PASS streams (a stream's estimator table is 8.4 MB of HBM)
        // (and of at most a quarter of the free HBM; an allocation that fails all the same halves the pass)
        size_t per = 0;
        if ((rc = dec16_tables(ctx, n, per)) != 0) return fail_all(rc);
        if ((rc = reserve(ctx, ctx->dec_meta, per * 8 * 2 + per * 4)) != 0) return fail_all(rc);
        int32_t *d_planes32 = nullptr;
        if (planes == 3) {
            if ((rc = reserve(ctx, ctx->dec_planes, (size_t)(npix * 3 * 4 * per) + 64)) != 0) return fail_all(rc);
            d_planes32 = (int32_t *)ctx->dec_planes.p;
        }
        ds.wave16 += n;
        hipStream_t s = l.stream;
        for (size_t i = 0; i < n; i++) status[i] = FELICS_E_HIP;  // until the kernel's own word arrives
        int first_rc = FELICS_OK;
        for (size_t first = 0; first < n; first += per) {
            const size_t cnt = std::min(per, n - first);
            uint32_t epoch0 = 0;
            if ((rc = dec16_epoch(ctx, s, epoch0)) != 0) return rc;
            uint64_t *d_off = (uint64_t *)ctx->dec_meta.p, *d_len = d_off + cnt;
            int *d_status = (int *)(d_len + cnt);
            HIP_TRY(ctx, hipMemcpyAsync(d_off, offsets + first, cnt * 8, hipMemcpyHostToDevice, s));
            HIP_TRY(ctx, hipMemcpyAsync(d_len, lens + first, cnt * 8, hipMemcpyHostToDevice, s));
            HIP_TRY(ctx, hipMemsetAsync(d_status, 0xFF, cnt * 4, s));
            HIP_TRY(ctx, launch_decode16(s, (const uint8_t *)d_streams, d_off, d_len, (uint32_t)cnt, hdr.width, hdr.height, hdr.color_type,
                                         (uint16_t *)d_pixels + first * (frame_bytes / 2), d_planes32, (uint32_t *)ctx->dec_table.p, epoch0,
                                         d_status));
            HIP_TRY(ctx, hipMemcpyAsync(status + first, d_status, cnt * 4, hipMemcpyDeviceToHost, s));
            HIP_TRY(ctx, hipStreamSynchronize(s));
            for (size_t i = first; i < first + cnt && !first_rc; i++)
                if (status[i]) first_rc = status[i];
        }
        return first_rc;
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
    for (size_t i = 0; i < n; i++)
        if (status[i]) return status[i];
    return FELICS_OK;
}

int felics_read_headers_device(felics_ctx *ctx, size_t n, const void *d_streams, const uint64_t *offsets, const uint64_t *lens,
                               felics_header *hdrs, int *status) {
    if (!ctx || (n && (!d_streams || !offsets || !lens || !hdrs || !status))) return FELICS_E_INVALID_ARGUMENT;
    auto fail_all = [&](int code) {
        for (size_t i = 0; i < n; i++) {
            status[i] = code;
            hdrs[i] = felics_header{};
        }
        return code;
    };
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
    auto fail_all = [&](int code) {
        for (size_t i = 0; i < n; i++) {
            status[i] = code;
            pix_offsets[i] = 0;
            if (hdrs) hdrs[i] = felics_header{};
        }
        return code;
    };
    if (ctx->failed) return fail_all(FELICS_E_HIP);
    if (n == 0) return FELICS_OK;
    if (any_pending(ctx)) return fail_all(FELICS_E_INVALID_ARGUMENT);  // felics_wait_batch first
    if (n > 0xFFFFFFFFull) return fail_all(FELICS_E_INVALID_ARGUMENT);
    if (hipSetDevice(ctx->device) != hipSuccess) return fail_all(hip_fail(ctx, hipGetLastError(), "hipSetDevice"));
    return decompress_images(ctx, n, d_streams, offsets, lens, (uint8_t *)d_pixels, d_pixels_cap, pix_offsets, hdrs, status);
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
