// felics_host.h -- what the host side of libfelics shares between its translation units (felics_context.cpp, felics_encode.cpp,
// felics_mixed.cpp, felics_decode_device.cpp): the context, a lane's streams and workspace, and the helpers that cross files.
// Internal: everything declared here has hidden visibility, the library exports the C ABI of include/felics.h only.
#pragma once
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
#include "felics_epochs.h"
#include "felics_kernels.h"

using namespace felics;

#pragma GCC visibility push(hidden)

namespace felics {

enum Stage { ST_PLANES = 0, ST_HIST, ST_OFFSETS, ST_SCATTER, ST_SPINE, ST_ASSIGN, ST_LENGTHS, ST_BITSCAN, ST_ZERO, ST_PACK,
             ST_WIDE_KEYS, ST_WIDE_SORT, ST_WIDE_CHAINS, ST_COUNT };
extern const char *const kStageNames[ST_COUNT];
static_assert(ST_COUNT <= FELICS_MAX_STAGES, "felics.h promises at most FELICS_MAX_STAGES stages");

constexpr int SLICES = 12;              // at most; a submission uses lane.nslices of them
constexpr uint64_t PASS_MAX_CHAINS = 1u << 23;  // chains (plane x context) of one 8-bit pass at most: max_images_per_pass
constexpr int EV_PAIRS = SLICES + 2;    // launches of one stage per sub-batch that can be timed
constexpr int MAX_LANES = 4;            // upper bound of the submissions in flight (felics_submit_batch_device), each with streams and workspace of its own
constexpr int DEFAULT_LANES = 2;        // what a context uses unless FELICS_LANES says otherwise (measured round 3: 2 lanes x 4 slices 3.03-3.06 ms per step,
                                        // 3 lanes x 3 slices 2.97-3.16, 4 lanes 3.18-3.47: the kernels are issue-bound, so more of them side by side gain nothing)
enum AssignOn { ASSIGN_OWN, ASSIGN_FRONT, ASSIGN_TAIL };  // the stream k_assign3 is queued on (felics_ctx_create)
int lanes_from_env();  // FELICS_LANES

struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
};

// One image of a mixed sub-batch (felics_mixed.cpp): a dense frame at px, or a view read where it lies / gathered.
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
    // felics_submit_surfaces_device: a 16-bit view the mixed 16-bit path reads where it lies (gray16: rows `pitch` BYTES apart, RGB16
    // through the plane transform) instead of gathering it
    bool wide_in_place = false;
    // felics_compress_views_device_indexed: where the restart index of this image's stream goes (device, 16-byte aligned, checked by
    // the entry point) and its segment; nullptr / 0: no index (every 16-bit image)
    uint8_t *index = nullptr;
    uint32_t segment_pixels = 0;
    // felics_compress_views_device_indexed16: this 16-bit image wants a version-2 index with segment_pixels; the library places it
    // (Index16Place) once its size is known
    bool index16 = false;
};

// felics_compress_views_device_indexed16: where a call's version-2 indexes go and what has been placed so far.  The size of an index
// depends on the content, so the indexes are placed in the order their sub-batches land, each a multiple of 64 bytes behind the one
// before; an index whose end lies behind `cap` is not begun.  A run that places the streams anew starts again from zero (begin_run).
struct Index16Place {
    uint8_t *d_index;
    uint64_t cap;
    uint64_t *idx_offsets, *idx_lens;  // [n], host
    uint64_t budget;                   // bytes of per-checkpoint workspace a sub-batch may take
    uint64_t test_cps;                 // FELICS_TEST_INDEX16_EMIT_CPS: checkpoints of a sub-batch at most (0: no cap)
    uint64_t total = 0;                // bytes placed so far
    bool too_small = false;            // an index did not fit and was not written
    // what felics_index16_view_emit_stats counts, over every run of the call
    uint64_t indexes = 0, rows = 0, bytes = 0, sub_batches = 0, shapes_max = 0, redone = 0;
    void begin_run() {
        total = 0;
        too_small = false;
    }
};

// One pipeline lane: HIP streams, stage events and a workspace in HBM of its own.  A submission (or one pass of
// a huge one) runs on one lane; felics_submit_batch_device hands the lanes out in turn, so that the GPU starts
// on the next batch while it finishes the last pack slices of this one.
struct Lane {
    hipStream_t stream = nullptr;      // spine slices; everything of a 16-bit sub-batch (run_wide)
    hipStream_t front = nullptr;       // colour planes; per slice the front kernel (classify + sort a tile's events) and the chains' records (k_enum)
    hipStream_t kstream = nullptr;     // assign slices (k of the events); with four lanes there is none and they go to the front stream (felics_ctx_create)
    hipStream_t tail = nullptr;        // pack slices (k_pack_t), sizes; the two-pass kernels (lengths, bit scan, pack); shared by the lanes unless FELICS_OWN_TAILS
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
    // felics_compress_batch_device_indexed16: per (plane, checkpoint) the contexts' bitmap and its popcount prefix, n_rows and rows_off;
    // per image the index's bytes and rows (totals) and where it goes (index_off, written by the host): Index16Emit, felics_kernels.h
    DevBuf i16_bitmap, i16_prefix, i16_nrows, i16_rows_off, i16_totals, i16_index_off;
    DevBuf i16_table;                 // felics_compress_views_device_indexed16: the sub-batch's Index16Geom rows (the same workspace otherwise)
    uint32_t epoch = 0;               // 8-bit sub-batches this lane has run (FELICS_TEST_LOOKBACK_EPOCH: plus a start value): its low 18 bits tag the look-back status words (felics_epochs.h)
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
    // ... of felics_submit_surfaces_device (p_n, p_out, p_cap as above): what landing needs -- the frames and their slots
    bool p_surfaces = false;
    std::vector<MixImage> s_im;
    std::vector<uint64_t> s_off, s_slot;
    // the sub-batch in flight
    int nslices = SLICES;             // slices its tiles are cut into (see felics_ctx::slices_*)
    bool m_tickets = false;           // the sub-batch's pack kernels took their tiles by ticket (what a look-back failure escalates from)
    bool m_fused = false;             // ... and were the single-pass kernels at all
    uint32_t m_cap = 0;               // slots per tile of its tile-local layout (8-bit: what indexes state16; launch_index_emit)
    bool queued = false;              // this sub-batch came through felics_submit_batch_device (other submissions share the GPU with it)
    Geometry g;
    size_t first_image = 0;
    const void *d_planes = nullptr;
    // a mixed sub-batch (felics_compress_images*): its plane table, written on the host (pinned) and copied to the device
    DevBuf mtable;
    PlaneGeom *h_table = nullptr;
    size_t h_table_cap = 0;
    // ... whose images want restart indexes (felics_compress_views_device_indexed; set by launch_mixed, cleared by begin_sub_batch):
    // the IndexGeom rows in mtable and their largest K, and the index ranges run_lane zeroes in front of the two emit kernels
    const IndexGeom *idx_rows = nullptr;
    uint32_t idx_max_K = 0;
    std::vector<std::pair<uint8_t *, size_t>> idx_zero;
};

}  // namespace felics

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
                                // round 4's pipeline: 2 slices 2.94, 3 2.82-2.89, 4 2.78-2.80, 6 2.89-2.91, 8 2.96 ms; three lanes 3.06)
    // k_pack_t takes its tiles from the workgroup index while the lanes share the tail stream: one pack kernel then has the
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
    bool test_scatter_order = false; // FELICS_TEST_SCATTER_ORDER=1: k_front reports a violation whatever it produced (tests)
    bool poison = false;        // FELICS_POISON=1: overwrite the workspace before every sub-batch (tests)
    bool trace = false;         // FELICS_TRACE=1: synchronise and report after every stage (debugging)
    bool trace_epochs = false;  // FELICS_TRACE_EPOCHS=1: a line on stderr for every epoch handed out (felics_epochs.h) and whether it clears; nothing is synchronised (tests)
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
    // felics_submit_surfaces_device: its counts; where stage_frame counts the bytes it writes (vstats.bytes_staged unless a surfaces
    // call is at work); the one lane run_images may use while other lanes hold tickets (-1: all of them)
    felics_surface_stats sstats = {};
    uint64_t *staged_bytes = nullptr;
    int only_lane = -1;
    DevBuf own;      // encode_device's own output when the caller gives none (the host entry point's fall-back for a chunk whose streams outgrew their slots)
    DevBuf dec_meta, dec_planes;  // GPU decoder: offsets | lens | status of a batch; Y / Co / Cg planes of RGB streams
    DevBuf dec_planes16;          // mixed decode call: the int32 planes of its RGB16 streams (beside dec_planes, used at the same time)
    DevBuf dec_lane_table;        // gray streams decoded 64 to a wave: the estimator rows that do not fit in LDS (3 KB per stream, zeroed per call)
    DevBuf dec_table;             // 16-bit streams: estimator tables in HBM (8.4 MB per stream of a pass), zeroed once, rows tagged with an epoch
    uint32_t dec_epoch = 0;       // last epoch handed out (three per call: one per plane)
    uint32_t dec_epoch_start = 0; // what dec_epoch starts from on a fresh (zeroed) dec_table: 0, or FELICS_TEST_DECODE16_EPOCH (tests: close to the wrap)
    DevBuf dec_lane16_table;      // 16-bit streams decoded 64 to a wave: their hashed estimator tables (felics_lanetable.h), zeroed once, rows tagged with an epoch
    uint32_t dec_lane16_epoch = 0;  // last epoch handed out on dec_lane16_table (three per launch, 1 .. DEC16L_EPOCH_MAX)
    uint32_t dec_lane16_epoch_start = 0;  // what it starts from on a fresh (zeroed) table: 0, or FELICS_TEST_DECODE16_LANES_EPOCH (tests; at most DEC16L_EPOCH_MAX)
    felics_decode_stats dstats = {};  // felics_get_decode_stats
    // felics_decompress_views_device: view_ready is its ready event too (every stream waits for it before it first reads a stream byte
    // or writes a view: wait_ready), view_stage holds the dense frames of its scattered class, dvstats the counts of
    // felics_get_decode_view_stats
    felics_decode_view_stats dvstats = {};
    // felics_decompress_batch_device_indexed: a status word per (stream, plane, segment); the counts of felics_get_index_stats
    DevBuf dec_seg_status;
    felics_index_stats istats = {};
    // felics_decompress_batch_device_indexed16: its tables are dec_table (epochs: dec_epoch), its words dec_meta and dec_seg_status, its
    // int32 planes dec_planes; the counts of felics_get_index16_stats
    felics_index16_stats i16stats = {};
    // felics_decompress_regions_device_indexed: its region table and work list (RegionRow[] | RegionItem[]; the items' status words
    // are dec_seg_status, the crop-sized planes dec_planes); the counts of felics_get_region_stats
    DevBuf dec_region_work;
    felics_region_stats rstats = {};
    // felics_decompress_regions_device_indexed16: the same buffers (dec_region_work, dec_seg_status, crop-sized int32 planes in
    // dec_planes), the tables and epochs of felics_decompress_batch_device_indexed16 (dec_table, dec_epoch); the counts of
    // felics_get_region16_stats
    felics_region16_stats r16stats = {};
    // felics_decompress_views_device_indexed: its tables live in the buffers above (offsets | lens | index offsets | index lens | the
    // two kinds of headers in dec_meta; rows, items and the finish tables in dec_region_work; item and row status words in
    // dec_seg_status; a pass's planes in dec_planes); view_ready is its ready event; the counts of felics_get_index_view_stats
    felics_index_view_stats ivstats = {};
    // felics_decompress_views_device_indexed16: the same buffers (int32 planes in dec_planes, the rows-loaded counter behind the
    // status words), the tables and epochs of felics_decompress_batch_device_indexed16 (dec_table, dec_epoch); the counts of
    // felics_get_index16_view_stats
    felics_index16_view_stats iv16stats = {};
    // felics_decompress_region_views_device_indexed and its 16-bit form: the buffers of the indexed views calls (the stream rows,
    // region rows, their views, the work list and the conversion rows in dec_region_work; a pass's crop-sized planes in dec_planes);
    // the counts of felics_get_region_view_stats and felics_get_region16_view_stats
    felics_region_view_stats rvstats = {};
    felics_region16_view_stats rv16stats = {};
    // felics_compress_views_device_indexed: the indexes of a remedy's group (redo_by_shape: written back to back by the uniform
    // writer, copied to where the caller wants them); the counts of felics_get_index_emit_stats
    DevBuf mix_index;
    felics_index_emit_stats iestats = {};
    felics_index16_emit_stats i16estats = {};  // felics_compress_batch_device_indexed16: the counts of felics_get_index16_emit_stats
    felics_index16_view_emit_stats i16vestats = {};  // felics_compress_views_device_indexed16: the counts of felics_get_index16_view_emit_stats
};

namespace felics {

#define HIP_TRY(ctx, call)                                          \
    do {                                                            \
        hipError_t e__ = (call);                                    \
        if (e__ != hipSuccess) return hip_fail(ctx, e__, #call);    \
    } while (0)

int hip_fail(felics_ctx *ctx, hipError_t e, const char *what);  // sets ctx->err, returns FELICS_E_HIP

// What every felics_get_*_stats(ctx, out, out_size) does: the context's counts `member`, as many bytes as both sides know
template <typename S>
int copy_stats(const felics_ctx *ctx, S felics_ctx::*member, S *out, size_t out_size) {
    if (!ctx || !out) return FELICS_E_INVALID_ARGUMENT;
    memcpy(out, &(ctx->*member), std::min(out_size, sizeof(S)));
    return FELICS_OK;
}

// ---- felics_context.cpp
int wait_event(felics_ctx *ctx, hipEvent_t ev, const char *what);
int sync_lane(felics_ctx *ctx, Lane &l);
int reserve(felics_ctx *ctx, DevBuf &b, size_t bytes);
int reserve_zeroed(felics_ctx *ctx, DevBuf &b, size_t bytes);
int reserve_pinned(felics_ctx *ctx, void **p, size_t &cap, size_t count, size_t bytes);
void collect_timing(felics_ctx *ctx, Lane &l);
int check_args(uint32_t w, uint32_t h, int color, int depth);
void header_bytes(uint8_t *o, uint32_t w, uint32_t h, int color, int depth);
bool any_pending(const felics_ctx *ctx);

// ---- felics_mixed.cpp
// A view's checks (felics_view_extent's) and the hull [lo, hi) of its samples' bytes relative to data.  encode_limits: the size
// limits of felics_compress_images as well (FELICS_E_UNSUPPORTED); the decoder has its own.
int check_view(const felics_view &v, int64_t &lo, int64_t &hi, bool encode_limits = true);
// the caller's ready event (ctx->view_ready, if any) in front of whatever is queued on s next
int wait_ready(felics_ctx *ctx, hipStream_t s);
// felics_wait_batch for a queued ticket of felics_submit_surfaces_device (the lane's `sized` has been waited for)
int land_surfaces(felics_ctx *ctx, Lane &l, uint64_t *offsets, uint64_t *lens);

// ---- felics_encode.cpp
struct SlotOutcome;
size_t max_images_per_pass(uint64_t npix, uint32_t planes, int depth);
Geometry &begin_sub_batch(felics_ctx *ctx, Lane &l, size_t first, size_t cnt, uint32_t w, uint32_t h, int color, int depth, int nslices, bool queued);
int run_sub_batch(felics_ctx *ctx, Lane &l, uint8_t *d_out, uint64_t slot_stride);
int launch_sub_batch(felics_ctx *ctx, Lane &l, size_t first, size_t cnt, const void *d_pixels, uint32_t w, uint32_t h, int color, int depth,
                     uint8_t *lane_out, uint64_t slot, int nslices, bool queued = false);
SlotOutcome decode_status(const felics_ctx *ctx, const Lane &l, uint64_t word);
SlotOutcome read_sizes(felics_ctx *ctx, Lane &l, bool wide, uint64_t slot, uint64_t *offsets, uint64_t *lens);
int apply_remedy(felics_ctx *ctx, const Lane &l, const SlotOutcome &o);
// (index: felics_compress_batch_device_indexed -- 8-bit frames; every pass that comes out usable leaves the restart indexes of its images)
struct IndexRequest {
    uint8_t *d_index;         // image i's index at d_index + i * bytes
    uint64_t bytes;           // felics_index_size of the shape
    uint32_t segment_pixels;
};
// (index16: felics_compress_batch_device_indexed16 -- 16-bit frames; every pass that comes out usable leaves the version-2 indexes of its
// images one behind the other, as far as they fit, and what all of them need.  An attempt that redoes the batch starts the counts again.)
struct Index16Request {
    uint8_t *d_index;
    uint64_t cap;             // bytes at d_index
    uint32_t segment_pixels;
    size_t pass_images;       // images of a pass at most: what the per-checkpoint workspace allows
    uint64_t *idx_offsets, *idx_lens;  // [n], host
    // the outcome of the last attempt
    uint64_t total = 0;       // bytes all indexes need (each a multiple of 64)
    uint64_t written = 0, bytes = 0, rows = 0, passes = 0;  // indexes written, their bytes and rows; passes that wrote any
    bool too_small = false;   // an index did not fit and was not written
};
int encode_device(felics_ctx *ctx, Lane &l, size_t n, const void *d_pixels, uint32_t w, uint32_t h, int color, int depth, uint8_t *d_out,
                  size_t d_out_cap, uint64_t *offsets, uint64_t *lens, uint8_t **used_out, bool start_exact = false,
                  const IndexRequest *index = nullptr, Index16Request *index16 = nullptr);

// the slot a stream gets unless the caller's buffer dictates another: the frame's size and a quarter, 16-byte aligned
inline uint64_t default_slot(size_t frame_bytes) { return ((uint64_t)frame_bytes + frame_bytes / 4 + 64 + 15) & ~15ull; }

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

// What the sizes that came back say about a sub-batch packed into fixed slots.
struct SlotOutcome {
    bool lookback_failed = false;  // a tile of the single-pass pack gave up waiting for the tiles before it
    bool overflow = false;         // a stream outgrew its slot, or an RGB plane its scratch slot
    bool order_violation = false;  // the front kernel's check of its own output failed: nothing of this sub-batch is to be used
    bool tile_overflow = false;    // a tile's events did not fit its slots (tile_cap_default): nothing of this sub-batch is to be used
    bool spine_error = false;      // the spine's search lost its invariant (never seen): an internal error, reported as such
    bool redo() const { return lookback_failed || order_violation || tile_overflow; }
};

}  // namespace felics

#pragma GCC visibility pop
