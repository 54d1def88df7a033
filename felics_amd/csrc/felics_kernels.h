// felics_kernels.h -- launch interface between the host pipeline (felics_api.cpp)
// and the gfx950 kernels (felics_kernels.hip).  Not part of the public C ABI.
#pragma once

#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stdint.h>

#include <algorithm>

#include "felics_index.h"
#include "felics_lanetable.h"

namespace felics {

// Contexts (H - L of a pixel's two neighbours, traits.rs:28): 0..255 for u8 samples, 0..510 for the Y/Co/Cg planes of
// RGB8 (table padded to 512).  NCTX sizes what is shared by both (upper bounds); the run table, the chain tables and the
// spine's grid use the sample type's own count, nctx_of<T>() = Geometry::nctx.
constexpr uint32_t NCTX = 512;
template <typename T>
constexpr uint32_t nctx_of() {
    return sizeof(T) == 1 ? 256u : 512u;  // T = sample type (u8 / i16) or event type (u8 / u16)
}
// pixels one workgroup sorts by context in the front stage.  Equal to the pack tile: the pack stage reads back k for exactly
// its own tile's events (k_pack_t), one look-back per workgroup.
constexpr uint32_t SORT_TILE = 4096;
// pack stage: 256 threads x 16 consecutive pixels
constexpr uint32_t PACK_THREADS = 256;
constexpr uint32_t PACK_PER_THREAD = 16;
constexpr uint32_t PACK_TILE = PACK_THREADS * PACK_PER_THREAD;
// LDS bit window of the pack stage: 2048 words = 8 KiB = 16 bits per pixel of a tile (more bits: more windows)
constexpr uint32_t PACK_WIN_WORDS = 2048;

// Sample type of a plane -> type of the per-group bit counts k_lengths hands to k_pack.
// 8-bit samples (u8 gray, i16 Y/Co/Cg): a 16-pixel group is at most 16 * 513 bits.  16-bit samples
// (u16 gray, i32 Y/Co/Cg): one code can be 2^17 bits long.
template <typename T> struct GroupBits { using type = uint16_t; };
template <> struct GroupBits<uint16_t> { using type = uint32_t; };
template <> struct GroupBits<int32_t> { using type = uint32_t; };
template <typename T> using group_bits_t = typename GroupBits<T>::type;

// Profiling: the host pipeline sets g_launch_timing around ONE launch to have that kernel's own begin and
// end recorded in the two events (hipExtLaunchKernel: the dispatch's timestamps, what rocprofv3 reports),
// instead of bracketing the launch with event records, which also measure the launch's wait for free
// compute resources.  The launcher that consumes it clears it.
struct LaunchTiming {
    hipEvent_t start = nullptr, stop = nullptr;
};
extern thread_local LaunchTiming g_launch_timing;

#define FELICS_LAUNCH(KERNEL, GRID, BLOCK, STREAM, ...)                                                    \
    do {                                                                                                   \
        const ::felics::LaunchTiming lt_ = ::felics::g_launch_timing;                                      \
        ::felics::g_launch_timing = ::felics::LaunchTiming{};                                              \
        if (lt_.start)                                                                                     \
            hipExtLaunchKernelGGL(KERNEL, GRID, BLOCK, 0, STREAM, lt_.start, lt_.stop, 0, __VA_ARGS__);   \
        else                                                                                               \
            hipLaunchKernelGGL(KERNEL, GRID, BLOCK, 0, STREAM, __VA_ARGS__);                               \
    } while (0)

struct Geometry {
    uint32_t W, H;
    uint32_t npix;              // W*H, pixels per plane
    uint32_t nimages;
    uint32_t planes_per_image;  // 1 gray, 3 rgb
    uint32_t nplanes;           // nimages * planes_per_image
    uint32_t sort_tiles;        // ceil(npix / SORT_TILE)
    uint32_t pack_tiles;        // ceil(npix / PACK_TILE)
    uint32_t color, depth;      // header fields
    uint32_t nctx;              // contexts per plane: nctx_of<sample type>()
    // A MIXED sub-batch (images of one depth and colour but different sizes, felics_compress_images*): the tile count stays uniform
    // (sort_tiles = pack_tiles = the largest image's, npix = sort_tiles * SORT_TILE), what differs per plane is read from this device
    // table (nullptr: the uniform geometry above).  16-bit samples: launch_wide_events, launch_lengths, launch_zero_edges and
    // launch_pack take their mixed kernels, the planes pointer they are given is unused, and npix is the stride of k_map (and of the
    // record's plane in the chain kernels).
    const struct PlaneGeom *mixed = nullptr;
    // A mixed sub-batch of gray8 planes some of which are PITCHED (views read where they lie): beside `mixed`, which the kernels
    // that see bits and not pixels go on reading, a table of the pitched policy's own row type for k_front and k_pack_t
    // (nullptr: every plane is dense).
    const struct PitchedGeom *pitched = nullptr;
    // A mixed sub-batch of gray16 planes read where they lie (felics_submit_surfaces_device): the 16-bit pitched row type, for
    // launch_wide_events, launch_lengths and launch_pack, which then take their pitched kernels (nullptr: every plane is dense).
    const struct PitchedGeom16 *pitched16 = nullptr;
};

// One plane of a mixed sub-batch.  The kernels index it by plane (wave-uniform: scalar loads).  Tiles past the plane's own end
// produce no events and no bits; the plane's size is still published by the last of the sub-batch's tiles.
struct PlaneGeom {
    const void *samples;   // the plane's first sample: the caller's frame (gray), or its Y / Co / Cg plane in the lane's planes buffer
    const void *image;     // the image's interleaved pixels as the caller gave them (RGB: what the plane transform reads)
    uint32_t W, H, npix;   // the image's size
    uint32_t ntiles;       // the plane's own pack tiles, ceil(npix / PACK_TILE) (<= Geometry::pack_tiles)
    uint64_t out_off;      // the image's slot in the output: byte offset from PackTarget::out, and size (writes beyond it are dropped)
    uint64_t out_slot;
};

// A view (felics_view): sample (x, y, c) at data + y * row_stride + x * pixel_stride + c * channel_stride, strides in bytes, signed
struct ViewRow {
    const void *data;
    int64_t row_stride, pixel_stride, channel_stride;
};
// mixed sub-batch of RGB8 views: image i read through rows[i] (a dense image: strides 3 W, 3, 1), its planes as launch_rgb8_to_planes_mixed
void launch_rgb8_view_to_planes(hipStream_t s, const PlaneGeom *table, const ViewRow *rows, uint64_t plane_stride, uint32_t max_npix, uint32_t nimg);
// a view copied to a dense frame (W * H * channels samples of T = u8 / u16): felics_wide.hip
template <typename T>
void launch_gather_view(hipStream_t s, const ViewRow &v, uint32_t W, uint32_t H, uint32_t channels, T *dst);

// One plane of a sub-batch with pitched planes: the plane as in the mixed table, and the bytes between two of its rows (>= W; W: a
// dense plane).  A row type of its own: PlaneGeom, which the mixed kernels load, stays as it is.
struct PitchedGeom {
    PlaneGeom g;
    uint64_t pitch;
};

// The same for a plane of u16 samples: the pitch in SAMPLES (>= W).  A row type of its own, as PitchedGeom is.
struct PitchedGeom16 {
    PlaneGeom g;
    uint64_t pitch;
};

void launch_rgb8_to_planes(hipStream_t s, const uint8_t *rgb, int16_t *planes, uint32_t npix, uint32_t nimg);
// mixed sub-batch: image i's pixels from table[3 i].image, its planes to table[3 i + c].samples (planes `plane_stride` samples apart)
void launch_rgb8_to_planes_mixed(hipStream_t s, const PlaneGeom *table, uint64_t plane_stride, uint32_t max_npix, uint32_t nimg);

// ------------------------------------------------------------------------------------------
// The 8-bit pipeline in TILE-LOCAL layout (round 5).  A pixel is classified once: the front kernel sorts the events of
// a tile (SORT_TILE pixels) by context in LDS and writes them as ONE contiguous piece at a fixed place,
//     slot (plane * sort_tiles + tile) * cap + s,
// contexts ascending, raster order inside a context, every context's run starting on a multiple of REC slots (the slots
// between a run's end and the next multiple are padding: pix = 0xFFFF).  A RECORD is REC = 16 consecutive slots of one
// run: the unit of the chain stage -- the spine leaves the estimator's state at the start of every record, the assign
// kernel replays a record per lane -- and of the k bytes the pack kernel reads back, contiguous per tile.  No histogram
// pass, no tile offsets, no chain bases, no global scatter: the chain of a context is the sequence of its runs over the
// tiles, listed per slice by k_enum (record descriptors in chain order).
// ------------------------------------------------------------------------------------------
constexpr uint32_t REC = 16;  // events per record
// Slots per tile.  Worst case SORT_TILE + (REC - 1) * nctx (every context one event over a multiple of REC); the default
// covers anything but adversarial content (uniform noise: 216 runs of a 4096-pixel tile, ~4400 slots); a tile that needs
// more raises TL_FLAG_OVERFLOW and the host redoes the batch with the worst case (felics_api.cpp).
// (npix: pixels per plane -- a plane smaller than a tile needs less)
inline uint32_t tile_cap_max(uint32_t nctx, uint32_t npix) {
    const uint32_t px = std::min(npix, SORT_TILE);
    return (px + (REC - 1) * std::min(nctx, px) + REC - 1) / REC * REC;
}
inline uint32_t tile_cap_default(uint32_t nctx, uint32_t npix) { return std::min(nctx == 256 ? 6144u : 8192u, tile_cap_max(nctx, npix)); }
constexpr uint32_t TL_FLAG_ORDER = 1u, TL_FLAG_OVERFLOW = 2u, TL_FLAG_SPINE = 4u;
constexpr uint32_t FRONT_TEST_VIOLATION = 1u, FRONT_SAFE_RANK = 2u;  // launch_front's `mode` bits (FRONT_SAFE_RANK: which k_front instantiation)

template <typename ET>
struct TileLocal {
    ET *ev;                // [slot] value to Rice-code
    uint16_t *pix;         // [slot] the event's pixel: offset in its tile (12 bits) | above << 12 (the sample lies above its neighbours); 0xFFFF in padding slots
    uint8_t *kq;           // [slot] k of the event (k_assign3)
    uint32_t *runtab;      // [(plane * nctx + c) * sort_tiles + tile] = first record of the tile's run of c (in the tile) | events << 16
    uint32_t *tile_slots;  // [plane * sort_tiles + tile] slots in use (a multiple of REC)
    uint32_t cap;          // slots per tile
};
// classify + sort the tiles [tile_begin, tile_end) of every plane (compression.rs:124-145, misc.rs:6-24)
template <typename T, typename ET>
void launch_front(hipStream_t s, const T *planes, const TileLocal<ET> &tl, const Geometry &g, uint32_t tile_begin, uint32_t tile_end,
                  uint32_t *flags, uint32_t mode);

// The chain stage of one slice: records [0, *nrec) of the slice's region of desc.
struct ChainSlice {
    uint2 *desc;           // [rec] {record's first slot / REC (over the whole sub-batch), events in it}: chain order
    uint2 *chain_seg;      // [chain] {first record, records} of the chain in this slice
    uint32_t *nrec;        // records of the slice (device counter, zeroed per sub-batch)
    uint4 *state16;        // [slot / REC, over the whole sub-batch: the same array for every slice] {S0 | S1 << 16, S2 | S3 << 16, S4 | S5 << 16, slot / REC}: the estimator's state at the record's first event
};
void launch_enum(hipStream_t s, const uint32_t *runtab, const ChainSlice &cs, const Geometry &g, uint32_t tile_begin, uint32_t tile_end,
                 uint32_t cap);
// chain_state: 8 words per chain (zeroed per sub-batch): the state behind the chain's last event so far
template <typename ET>
void launch_spine3(hipStream_t s, const ET *ev, const ChainSlice &cs, uint32_t *chain_state, uint32_t *flags, const Geometry &g);
// k of the events of the tiles [tile_begin, tile_end) of every plane, from the states k_spine3 left
template <typename ET>
void launch_assign3(hipStream_t s, const TileLocal<ET> &tl, const uint4 *state16, const Geometry &g, uint32_t tile_begin, uint32_t tile_end);
// two-pass pack: k from the tiles' slots to a byte per pixel
void launch_k_to_pixels_tl(hipStream_t s, const uint8_t *kq, const uint16_t *pix, const uint32_t *tile_slots, uint32_t cap, uint8_t *k_map,
                           const Geometry &g);

// The restart index of every image of an 8-bit same-shape pass (felics_index.hip; format: felics.h, felics_index.h), from what the pass
// leaves behind: runtab and state16 (the contexts' states at the checkpoints), tile_bitoff / plane_base / plane_carry (the bit
// positions), the planes' samples (the windows).  index: image i's at index + i * felics_index_size(...), 16-byte aligned and
// ZEROED beforehand.  Everything of the pass, packing included, has been queued on s or is complete.
struct IndexEmit {
    uint8_t *index;
    uint64_t index_bytes, cp_bytes, win_off;  // bytes of an index, of a checkpoint; where its window starts
    uint32_t W, H, npix, tiles, nctx, planes_per_image;
    uint32_t K, seg_tiles;                    // checkpoints per plane, tiles between two of them
    uint32_t color;
};
void launch_index_emit(hipStream_t s, const void *planes, const uint32_t *runtab, const uint4 *state16, uint32_t cap, const uint64_t *tile_bitoff,
                       const uint64_t *plane_base, const uint64_t *plane_carry, const Geometry &g, uint8_t *index, uint32_t segment_pixels);

// The same for a MIXED 8-bit sub-batch (felics_compress_views_device_indexed): every plane has a row of its own beside its PlaneGeom
// row -- a row type of its own, the tables the encode kernels load stay as they are.  index: the IMAGE's index (16-byte aligned,
// zeroed beforehand; nullptr: this image gets none), the rest its layout (index_layout of the image's own W, H and segment).
struct IndexGeom {
    uint8_t *index;
    uint32_t K, seg_tiles;       // checkpoints per plane, tiles between two of them
    uint64_t cp_bytes, win_off;  // bytes of a checkpoint; where its window starts
};
void launch_index_emit_mixed(hipStream_t s, const uint32_t *runtab, const uint4 *state16, uint32_t cap, const uint64_t *tile_bitoff,
                             const uint64_t *plane_base, const uint64_t *plane_carry, const Geometry &g, const IndexGeom *rows, uint32_t max_K);

// The version-2 restart index of every image of a 16-bit same-shape pass (felics_index16.hip; format: felics.h, felics_index.h), from what
// run_wide leaves behind: the sorted records, their plane ranges (meta) and the chain heads, tile_bitoff / plane_base / plane_carry,
// the planes' samples.  Two steps with the host between them, because an index's size depends on the content:
//   launch_index16_scan   clears the bitmaps, marks, ranks and plans: n_rows and rows_off of every checkpoint, totals[2 i] = the bytes of
//                         image i's index and totals[2 i + 1] = its rows
//   launch_index16_write  image i's index to index + index_off[i] (64-byte aligned; ~0: this image's index is not written), every byte
//                         of it -- nothing need be cleared beforehand
// Workspace: bitmap and prefix hold wpc words per (plane, checkpoint) -- index16_words_per_checkpoint, a bit per context --,
// n_rows a word and rows_off two.
struct Index16Emit {
    uint8_t *index;
    const uint64_t *index_off;  // [nimages], device
    uint32_t *bitmap, *prefix, *n_rows;
    uint64_t *rows_off, *totals;
    uint32_t W, H, npix, color, planes_per_image, nplanes, nimages;
    uint32_t K, segment_pixels, wpc;
};
uint32_t index16_words_per_checkpoint(uint32_t color);
void launch_index16_scan(hipStream_t s, const uint64_t *recs, const uint32_t *meta, const Geometry &g, const Index16Emit &e);
void launch_index16_write(hipStream_t s, const void *planes, const uint64_t *recs, const uint32_t *meta, const uint64_t *heads, const uint32_t *nheads,
                          const uint64_t *tile_bitoff, const uint64_t *plane_base, const uint64_t *plane_carry, const Geometry &g,
                          const Index16Emit &e);

// The same two steps for a sub-batch whose images differ in shape or segment (felics_compress_views_device_indexed16): every plane has
// a row of its own beside its PlaneGeom row -- a row type of its own, as IndexGeom is; the tables the encode kernels load stay as
// they are.  The kernels index it by plane (wave-uniform: scalar loads).  The planes of an image follow each other and share
// everything but c and samples.  The workspace is Index16Emit's, with checkpoint (plane, j) at cp0 + j.
struct Index16Geom {
    const void *samples;      // the plane's first sample: u16 with row length W (gray: the dense frame), or the i32 Y / Co / Cg plane
    uint32_t image, c;        // the image's ordinal in the sub-batch (indexes index_off / totals), the plane's index in the image
    uint32_t W, H, npix;
    uint32_t segment_pixels;
    uint32_t K;               // checkpoints per plane; 0: this image gets no index, every kernel skips its planes
    uint32_t cp0;             // the plane's first checkpoint: the sum of K over the planes in front of it
    uint64_t win_base, win_bytes, rows_base;  // the image's Index16Layout
};
struct Index16TableEmit {
    uint8_t *index;
    const uint64_t *index_off;  // [nimages], device; ~0: this image's index is not written
    uint32_t *bitmap, *prefix, *n_rows;
    uint64_t *rows_off, *totals;
    const Index16Geom *rows;    // [nplanes], device
    uint32_t color, planes_per_image, nplanes, nimages;
    uint32_t ncps, wpc;         // the sub-batch's checkpoints (the sum of K over all planes); words per checkpoint
};
// max_npix: the largest plane's pixels; max_rows_base: the largest rows_base (they size grids, nothing else)
void launch_index16_scan_table(hipStream_t s, const uint64_t *recs, const uint32_t *meta, const Index16TableEmit &t, uint32_t max_npix);
void launch_index16_write_table(hipStream_t s, const uint64_t *recs, const uint32_t *meta, const uint64_t *heads, const uint32_t *nheads,
                                const uint64_t *tile_bitoff, const uint64_t *plane_base, const uint64_t *plane_carry, uint32_t pack_tiles,
                                const Index16TableEmit &t, uint64_t max_rows_base);

// k_map / plane / slot buffers are read in whole 16-byte chunks by the tile staging
constexpr size_t STAGE_PAD = 64;

// lengths / bit scan / pack work on a range [t0, t1) of every plane's PACK tiles, so they can follow the
// spine slice by slice.  tile_bitoff is relative to the plane; plane_base (zero for gray, set by
// launch_finish_sizes for the later planes of an RGB image) makes it relative to the image stream.
template <typename T>
void launch_lengths(hipStream_t s, const T *planes, const uint8_t *k_map, group_bits_t<T> *group_bits,
                    uint32_t *tile_bits, const Geometry &g, uint32_t t0, uint32_t t1);

void launch_bitscan_slice(hipStream_t s, const uint32_t *tile_bits, uint64_t *tile_bitoff, uint64_t *plane_carry,
                          const Geometry &g, uint32_t t0, uint32_t t1);

void launch_finish_sizes(hipStream_t s, const uint64_t *plane_carry, uint64_t *plane_base, uint64_t *image_bytes,
                         const Geometry &g);

// exact placement (streams back to back, 16-byte aligned) and zeroing of exactly those bytes
void launch_place_streams(hipStream_t s, const uint64_t *image_bytes, uint64_t *image_off, const Geometry &g);
void launch_zero_streams(hipStream_t s, uint32_t *out, const uint64_t *image_off, const Geometry &g);

// Placement of the streams in `out`: slot_stride != 0 -> stream i at i * slot_stride (bytes), writes
// beyond the slot are dropped; slot_stride == 0 -> stream i at image_off[i].
void launch_zero_edges(hipStream_t s, uint8_t *out, const uint64_t *image_off, uint64_t slot_stride,
                       const uint64_t *tile_bitoff, const uint32_t *tile_bits, const uint64_t *plane_base,
                       const Geometry &g, uint32_t t0, uint32_t t1);

template <typename T>
void launch_pack(hipStream_t s, const T *planes, const uint8_t *k_map, const group_bits_t<T> *group_bits,
                 const uint64_t *tile_bitoff, const uint32_t *tile_bits, const uint64_t *plane_base,
                 const uint64_t *image_off, uint64_t slot_stride, uint8_t *out, const Geometry &g, uint32_t t0,
                 uint32_t t1);

// Single-pass pack for 8-bit frames with fixed output slots (image i's stream at out + i * slot_stride):
// code lengths, tile offsets (decoupled look-back through `status`, one u64 per tile, zero-initialised
// once, `epoch` distinguishes submissions) and packing in one kernel per slice of tiles.  Writes
// tile_bitoff / tile_bits / plane_carry like the lengths + bitscan kernels.  The words two tiles share are
// left in edge_first / edge_last; launch_join_edges stores them once every tile is done.  Planes 1, 2 of
// an RGB image are packed into scratch slots (plane c of image i at scratch + (2 i + c - 1) * plane_slot)
// and moved behind plane 0 by launch_concat_planes after launch_finish_sizes.
// *error: bit 0 = a look-back gave up waiting, bit 1 = a plane outgrew its scratch slot.
struct PackTarget {
    uint8_t *out;
    uint64_t slot_stride;
    uint8_t *scratch;
    uint64_t plane_slot;
};
// the single-pass pack on the tile-local layout: the events' codes built from the tile's own slots (kq / pix / ev / tile_slots of TileLocal)
template <typename T>
void launch_pack_t(hipStream_t s, const T *planes, const uint8_t *kq, const uint16_t *pix, const void *ev, const uint32_t *tile_slots, uint32_t cap,
                   uint64_t *status, uint64_t *tile_bitoff, uint32_t *tile_bits, uint64_t *plane_carry, uint32_t *edge_first,
                   uint32_t *edge_last, uint32_t *error, const PackTarget &to, const Geometry &g, uint32_t st0, uint32_t st1, uint32_t epoch,
                   uint32_t *ticket);
void launch_join_edges(hipStream_t s, const uint64_t *tile_bitoff, const uint32_t *tile_bits, const uint32_t *edge_first,
                       const uint32_t *edge_last, const PackTarget &to, const Geometry &g);
void launch_concat_planes(hipStream_t s, const uint64_t *plane_base, const uint64_t *plane_carry, const PackTarget &to,
                          const Geometry &g);

// Where the single-pass pack puts a plane's bits.  Plane 0 of an image goes to the image's slot of the
// output (header first); planes 1, 2 of an RGB image are packed as bit strings of their own into scratch
// slots and moved behind plane 0 by k_concat_planes once every size is known (compression.rs:365-367:
// the planes of an image follow each other without alignment).
struct PlaneOut {
    uint8_t *out;
    uint64_t slot_stride;  // image i's stream starts at out + i * slot_stride
    uint8_t *scratch;
    uint64_t plane_slot;   // plane c >= 1 of image i at scratch + (i * (planes_per_image - 1) + c - 1) * plane_slot
    uint32_t planes_per_image;
};


// join_edges for a given tile count
void launch_join_edges_tiles(hipStream_t s, const uint64_t *tile_bitoff, const uint32_t *tile_bits, const uint32_t *edge_first,
                             const uint32_t *edge_last, const PackTarget &to, const Geometry &g, uint32_t ntiles);

constexpr uint32_t DECODE_LDS_LIMIT = 160u * 1024u;  // LDS of one CU (MI355X_MICROARCH.md): what a decoder workgroup may ask for
// ---- GPU decoder for 8-bit streams (felics_gpudecode.hip): one wave per stream.  status[i] = FELICS_OK or an error
// code; gray pixels go straight to `pixels`, RGB through int16 planes (image i at i * 3 * npix) + a conversion kernel.
uint32_t decode8_lds_bytes(uint32_t W, uint32_t color);
// 16-bit streams: the estimator tables live in HBM (decode16_table_bytes(n): 8.4 MB per stream, zero-initialised ONCE: rows carry
// the epoch they were written in; a call uses epochs epoch0 .. epoch0 + 2, never 0 and never reused on the same buffer)
uint32_t decode16_lds_bytes(uint32_t W);
size_t decode16_table_bytes(uint32_t n);
hipError_t launch_decode16(hipStream_t s, const uint8_t *streams, const uint64_t *offsets, const uint64_t *lens, uint32_t n,
                           uint32_t W, uint32_t H, uint32_t color, uint16_t *pixels, int32_t *planes, uint32_t *table,
                           uint32_t epoch0, int *status);
// The same for large batches of 8-bit streams, gray or RGB (felics_gpudecode.hip, k_decode8_lanes): 64 streams per wave, lane = stream;
// needs W >= 8 and a zeroed table of decode8_lanes_table_bytes(n, color) bytes (3 KB per gray stream, 18 KB per RGB stream: the
// estimator rows that do not live in LDS); RGB: `planes` as for launch_decode8.
constexpr uint32_t DECODE8_LANES_MIN_STREAMS = 1536;  // measured (profiles/r04/decode_scaling.txt): one wave per stream saturates at ~2.3 GPix/s from ~1000
                                                       // streams, a lane decodes 1.47 MPix/s whatever the batch: the forms cross at ~1500 streams
constexpr uint32_t DECODE8_LANES_MIN_STREAMS_RGB = 2048;  // RGB8 (profiles/r05/decode_scaling_rgb.txt, 1080p frames): 0.88 against 0.94 GPix/s at 2048 streams, 0.97 / 1.88 at 4096
size_t decode8_lanes_table_bytes(uint32_t n, uint32_t color);
hipError_t launch_decode8_lanes(hipStream_t s, const uint8_t *streams, const uint64_t *offsets, const uint64_t *lens, uint32_t n,
                                uint32_t W, uint32_t H, uint32_t color, uint8_t *pixels, int16_t *planes, uint32_t *table, int *status);
hipError_t launch_decode8(hipStream_t s, const uint8_t *streams, const uint64_t *offsets, const uint64_t *lens, uint32_t n,
                          uint32_t W, uint32_t H, uint32_t color, uint8_t *pixels, int16_t *planes, int *status);
// n streams of one shape, each with its restart index (felics.h; index i at index + i * index_stride, 16-byte aligned): one wave per
// (stream, plane, segment), grid n * C * max(K, 1) < 2^31.  seg_status: a word per wave; status[i] = stream i's first failing one.
// k_decode8_seg (the walk from a checkpoint with the segment sink: pixel `at` of a segment to out[at]), then launch_seg_finish.
hipError_t launch_decode8_seg(hipStream_t s, const uint8_t *streams, const uint64_t *offsets, const uint64_t *lens, const uint8_t *index,
                              uint64_t index_stride, uint32_t n, uint32_t W, uint32_t H, uint32_t color, uint32_t segment_pixels, uint32_t K,
                              uint8_t *pixels, int16_t *planes, int *seg_status, int *status);
// The same call on large batches (k_decode8_seg_lanes): 64 segments per wave, lane = stream.  Wave w of the n / 64 * C * K waves of a
// call is (group of 64 consecutive streams, plane, segment) = (w / (C K), w / K % C, w % K); a launch takes waves wave0 .. wave0 +
// nwaves - 1 and a table of index8_lanes_table_bytes(64 * nwaves, color) bytes (3 KB per gray item, 6 KB per RGB item: the estimator
// rows that do not live in LDS, loaded from the checkpoints: nothing to zero).  Needs W >= 8 and K >= 1.  It writes seg_status as
// launch_decode8_seg's kernel does; launch_seg_finish is that launcher's tail for streams 0 .. n - 1: status[i] = stream i's first
// failing word, then the RGB conversion of the clean ones.
// The lane form is taken from this many lane-form items (n / 64 * 64 * C * K) on.  INDEX8_LANES_NEVER: no call takes the form by
// itself (FELICS_TEST_INDEX_LANES=1 still does).  The values are to come from the sweep of profiles/tools/indexed_lanes.py, and that
// sweep HAS NOT RUN YET (profiles/indexed_lanes.txt says so): until it has, neither colour takes the form by itself.  Where the sweep
// is expected to put them: DECODE8_LANES_MIN_STREAMS (1536) and DECODE8_LANES_MIN_STREAMS_RGB (2048), an item being a stream as far as
// both kernels are concerned.
constexpr uint32_t INDEX8_LANES_NEVER = 0xFFFFFFFFu;
constexpr uint32_t INDEX8_LANES_MIN_ITEMS = INDEX8_LANES_NEVER;
constexpr uint32_t INDEX8_LANES_MIN_ITEMS_RGB = INDEX8_LANES_NEVER;
size_t index8_lanes_table_bytes(uint64_t items, uint32_t color);
hipError_t launch_decode8_seg_lanes(hipStream_t s, const uint8_t *streams, const uint64_t *offsets, const uint64_t *lens, const uint8_t *index,
                                    uint64_t index_stride, uint32_t W, uint32_t H, uint32_t color, uint32_t segment_pixels, uint32_t K,
                                    uint32_t wave0, uint32_t nwaves, uint8_t *pixels, int16_t *planes, uint32_t *table, int *seg_status);
// The finishes of the three indexed call kinds, for both depths: P is the type of an RGB plane's sample, T the pixel's -- <int16_t,
// uint8_t> for 8-bit streams, <int32_t, uint16_t> for 16-bit ones (the instantiations felics_gpudecode.hip holds).  Each is
// k_seg_status, then the conversion of the clean RGB rows in grid rows of at most 65 535.
// Dense (streams 0 .. n - 1 of one shape): status[i] = stream i's first failing word in (plane, segment) order.
template <typename P, typename T>
hipError_t launch_seg_finish(hipStream_t s, uint32_t n, uint32_t W, uint32_t H, uint32_t color, uint32_t K, T *pixels, P *planes, const int *seg_status,
                             int *status);
// Regions of such streams (felics_decompress_regions_device_indexed, felics.h "Restart index: regions"): one wave per work item =
// (region, plane, needed segment) of the call's plan (felics_index.h: region_plan, RegionRow, RegionItem, REGION_HEADER_ONLY),
// k_decode8_region: k_decode8_seg's walk with the region sink (it stops behind the region's last pixel and writes the samples inside
// the region to the crop).  Gray crops at pixels + out_off, RGB ones through crop-sized int16 planes at planes + plane_off.
// nitems < 2^31 items; item_status: a word per item.
hipError_t launch_decode8_regions(hipStream_t s, const uint8_t *streams, const uint64_t *offsets, const uint64_t *lens, const uint8_t *index,
                                  uint64_t index_stride, uint32_t W, uint32_t H, uint32_t color, uint32_t segment_pixels, uint32_t K,
                                  const RegionRow *rows, const RegionItem *items, uint32_t nitems, uint8_t *pixels, int16_t *planes,
                                  int *item_status);
// The region calls' finish, once behind the last launch: status[r] = region r's first failing item (k_seg_status over the rows'
// items), then the conversion of the clean RGB crops; max_crop: the largest w * h of an RGB region (0: gray).
template <typename P, typename T>
hipError_t launch_regions_finish(hipStream_t s, const RegionRow *rows, uint32_t nregions, uint64_t max_crop, T *pixels, P *planes,
                                 const int *item_status, int *status);
// Indexed streams of ANY shapes into views (felics_decompress_views_device_indexed, felics.h "Restart index: views and mixed shapes"):
// one wave per work item = (row, plane, segment), k_decode8_seg_views: k_decode8_seg's walk with the view sink.  A row is one stream
// of the call that passed the host's checks; the walk's geometry, segment_pixels and K come from the row (what the host read out of
// the stream's and the index's own headers; the walk checks both again), so every row has its own.  Gray samples go through the
// row's view, one byte each: data + y * row_stride + col * pixel_stride (view_sample_offset, felics_index.h), any strides; RGB rows
// write int16 planes at planes + plane_off (three planes of W * H samples), converted through the view by k_ycocg8_to_rgb<ConvStrided>.
// A row's items are contiguous, in (plane, segment) order; an empty image (K = 0) has one pseudo item per plane, segment 0.
struct IndexViewRow {
    uint32_t stream;             // index into offsets / lens
    uint32_t W, H, color;
    uint32_t segment_pixels, K;
    uint32_t item0, nitems;      // its items in the call's work list: item0 .. item0 + nitems - 1, nitems = C * max(K, 1)
    uint64_t index_off;          // byte offset of its index in `index` (index + index_off is a multiple of 16)
    uint64_t plane_off;          // RGB: element offset of its planes in `planes`
    ViewRow view;                // gray: where its samples go
};
struct IndexViewItem {
    uint32_t row, plane, seg;
};
// One launch: `nitems` < 2^31 consecutive items of the work list, whose rows all fit `lds` bytes of dynamic LDS (decode8_lds_bytes of
// the widest); item_status: a word per item of the launch.
hipError_t launch_decode8_seg_views(hipStream_t s, const uint8_t *streams, const uint64_t *offsets, const uint64_t *lens, const uint8_t *index,
                                    const IndexViewRow *rows, const IndexViewItem *items, uint32_t nitems, uint32_t lds, int16_t *planes,
                                    int *item_status);
// The tail of a pass of that call for rows 0 .. n - 1 of its tables: status[r] = row r's first failing word (k_seg_status over
// `regions`, a RegionRow per row of which item0 / nitems are read), then the conversion of the clean RGB rows through their views
// (conv[r].stream = r: status is per row; a gray row has nothing to convert).  max_npix: the largest W * H of an RGB row (0: none).
struct DecodeRow;  // (below, with the mixed decode call)
template <typename P, typename T>
hipError_t launch_seg_views_finish(hipStream_t s, uint32_t n, const RegionRow *regions, const int *item_status, const DecodeRow *conv,
                                   const ViewRow *views, uint64_t max_npix, P *planes, int *status);
// The first 64 bytes of each of n restart indexes (index i at index + idx_offsets[i], a multiple of 16; idx_lens[i] bytes) to
// out + 64 i, zeros behind an index shorter than that: no byte outside [idx_offsets[i], idx_offsets[i] + idx_lens[i]) is read.
hipError_t launch_read_index_headers(hipStream_t s, const uint8_t *index, const uint64_t *idx_offsets, const uint64_t *idx_lens, uint32_t n,
                                     uint8_t *out);
// 16-bit streams of one shape through version-2 restart indexes (felics_decompress_batch_device_indexed16, felics.h "Restart index:
// 16-bit streams"; index i at index + idx_offsets[i], a multiple of 64, idx_lens[i] bytes): k_decode16_seg, one wave per (stream,
// plane, segment).  A launch is a PASS of the call's n * C * max(K, 1) items: items item0 .. item0 + nitems - 1, wave b on table b of
// `table` (decode16_table_bytes(nitems) bytes, launch_decode16's buffer and epoch rule: one fresh epoch per pass).  seg_status: a word
// per item of the call; *rows_loaded += the state rows copied.  The call's tail is launch_seg_finish.
hipError_t launch_decode16_seg(hipStream_t s, const uint8_t *streams, const uint64_t *offsets, const uint64_t *lens, const uint8_t *index,
                               const uint64_t *idx_offsets, const uint64_t *idx_lens, uint32_t W, uint32_t H, uint32_t color, uint32_t segment_pixels,
                               uint32_t K, uint32_t item0, uint32_t nitems, uint16_t *pixels, int32_t *planes, uint32_t *table, uint32_t epoch,
                               int *seg_status, unsigned long long *rows_loaded);
// Regions of such streams (felics_decompress_regions_device_indexed16, felics.h "Restart index: regions of 16-bit streams"):
// k_decode16_region, one wave per work item = (region, plane, needed segment) -- k_decode16_seg's walk with the region sink.  The
// tables are launch_decode8_regions' (RegionRow, RegionItem, REGION_HEADER_ONLY), with out_off in bytes (even) and plane_off in
// int32 samples of crop-sized planes.  A launch is a PASS: items item0 .. item0 + nitems - 1 of `items`, wave b on table b of `table`
// (launch_decode16_seg's buffer and epoch rule); item_status: a word per item of the call; *rows_loaded += the state rows copied.
// The call's tail, once behind the last pass, is launch_regions_finish.
hipError_t launch_decode16_regions(hipStream_t s, const uint8_t *streams, const uint64_t *offsets, const uint64_t *lens, const uint8_t *index,
                                   const uint64_t *idx_offsets, const uint64_t *idx_lens, uint32_t W, uint32_t H, uint32_t color,
                                   uint32_t segment_pixels, uint32_t K, const RegionRow *rows, const RegionItem *items, uint32_t item0, uint32_t nitems,
                                   uint8_t *pixels, int32_t *planes, uint32_t *table, uint32_t epoch, int *item_status,
                                   unsigned long long *rows_loaded);
// 16-bit streams of ANY shapes through version-2 indexes into views (felics_decompress_views_device_indexed16, felics.h "Restart
// index: 16-bit streams into views and mixed shapes"): k_decode16_seg_views, one wave per work item = (row, plane, segment) --
// k_decode16_seg's walk with the view sink, on launch_decode8_seg_views' tables (IndexViewRow, IndexViewItem; index + index_off a
// multiple of 64, plane_off in int32 samples; the index's length is idx_lens[row.stream]).  Gray samples go through the row's view, one
// aligned two-byte store each, any (even) strides; RGB rows write int32 planes at planes + plane_off, converted through the view by
// k_ycocg16_to_rgb<ConvStrided>.  One launch: `nitems` consecutive items of the work list whose rows all fit `lds` bytes of dynamic
// LDS (decode16_lds_bytes of the widest), wave b on table b of `table` (decode16_table_bytes(nitems) bytes, launch_decode16_seg's
// buffer and epoch rule: one fresh epoch per launch); item_status: a word per item of the launch; *rows_loaded += the state rows
// copied.  A stream pass's tail is launch_seg_views_finish.
hipError_t launch_decode16_seg_views(hipStream_t s, const uint8_t *streams, const uint64_t *offsets, const uint64_t *lens, const uint8_t *index,
                                     const uint64_t *idx_lens, const IndexViewRow *rows, const IndexViewItem *items, uint32_t nitems, uint32_t lds,
                                     int32_t *planes, uint32_t *table, uint32_t epoch, int *item_status, unsigned long long *rows_loaded);
// Regions of indexed streams of ANY shapes straight into views (felics_decompress_region_views_device_indexed and its 16-bit form,
// felics.h "Restart index: regions into views and mixed shapes"): one wave per work item = (region, plane, needed segment),
// k_decode8_region_views / k_decode16_region_views -- the region walk (it stops behind the region's last pixel) with a sink that writes
// a gray sample of the window through the region's view, one aligned store at view_sample_offset(.., col - x, y - y0, 0), and an RGB one
// to plane c of the region's crop-sized planes at planes + plane_off (converted through the view by the strided conversion:
// launch_seg_views_finish with a DecodeRow of W = w, H = h per region).  The tables: a RegionViewStream per stream of the call that
// passed the host's checks (what the host read out of its headers; the walk checks both again), a RegionRow per region (stream: the
// stream's number, which names its RegionViewStream and its offsets / lens; item0 / nitems for k_seg_status; out_off unused) with its
// ViewRow beside it, RegionItem as in the same-shape region calls (no REGION_HEADER_ONLY items: the header checks are final on the
// host, an empty region has no item).
struct RegionViewStream {
    uint32_t W, H, color;
    uint32_t segment_pixels, K;
    uint32_t pad;
    uint64_t index_off;  // byte offset of its index in `index` (index + index_off a multiple of 16; 16-bit: of 64)
};
// One launch: `nitems` < 2^31 consecutive items of the work list whose streams' rows all fit `lds` bytes of dynamic LDS; item_status: a
// word per item of the launch.  The 16-bit form: wave b on table b of `table`, one fresh epoch per launch, the index's length from
// idx_lens[stream], *rows_loaded += the state rows copied (as launch_decode16_seg_views).
hipError_t launch_decode8_region_views(hipStream_t s, const uint8_t *streams, const uint64_t *offsets, const uint64_t *lens, const uint8_t *index,
                                       const RegionViewStream *srows, const RegionRow *regions, const ViewRow *views, const RegionItem *items,
                                       uint32_t nitems, uint32_t lds, int16_t *planes, int *item_status);
hipError_t launch_decode16_region_views(hipStream_t s, const uint8_t *streams, const uint64_t *offsets, const uint64_t *lens, const uint8_t *index,
                                        const uint64_t *idx_lens, const RegionViewStream *srows, const RegionRow *regions, const ViewRow *views,
                                        const RegionItem *items, uint32_t nitems, uint32_t lds, int32_t *planes, uint32_t *table, uint32_t epoch,
                                        int *item_status, unsigned long long *rows_loaded);
// The same for 16-bit streams, gray or RGB (k_decode16_lanes): 64 streams per wave, lane = stream; needs W >= 8 and a table of
// decode16_lanes_table_bytes(n, W, H, color) bytes = n * planes * dec16l_rows(W * H, planes) * 64 (felics_lanetable.h: sized by the
// pixel count, 512 KB per plane of a 64 x 64 stream, the wave form's 8.4 MB from 32 771 pixels on), zero-initialised ONCE: rows carry
// the epoch they were written in; a launch uses epochs epoch0 .. epoch0 + 2, in 1 .. DEC16L_EPOCH_MAX and never reused on the same
// buffer.  RGB: `planes` takes the int32 planes (n * 3 * W * H), `pixels` the converted frames.
constexpr uint32_t DECODE16_LANES_NEVER = 0xFFFFFFFFu;  // a threshold no call reaches (the form then only when forced); not needed today
// measured (profiles/decode16_lanes.txt, 64 x 64 streams, both forms in one run): the wave form saturates at 1.3 - 2.0 GPix/s from
// ~1000 streams, a lane decodes 0.5 - 1.0 MPix/s whatever the batch; at 1 024 streams the lane form has half the wave form's rate
// on synth, natural and noise content alike, at 4 096 it is 1.8 - 2.0x faster on all three (16 384: 6.7 - 6.8x, 8.4 - 13.6 GPix/s)
constexpr uint32_t DECODE16_LANES_MIN_STREAMS = 4096;
// RGB16 (same file): the wave form's 0.38 - 0.54 GPix/s against 0.19 - 0.29 at 1 024 streams, 0.38 - 0.55 against 0.76 - 1.10 at 4 096 (2.0 - 2.1x)
constexpr uint32_t DECODE16_LANES_MIN_STREAMS_RGB = 4096;
// size_t decode16_lanes_table_bytes(uint32_t n, uint32_t W, uint32_t H, uint32_t color): felics_lanetable.h (the native check compiles it too)
hipError_t launch_decode16_lanes(hipStream_t s, const uint8_t *streams, const uint64_t *offsets, const uint64_t *lens, uint32_t n,
                                 uint32_t W, uint32_t H, uint32_t color, uint16_t *pixels, int32_t *planes, uint32_t *table,
                                 uint32_t epoch0, int *status);
// The headers of n streams in device memory (felics_read_headers_device, felics_decompress_images_device): a lane per stream,
// felics_read_header's checks in its order, every read inside [offsets[i], offsets[i] + lens[i]).  Fields are zero where
// status != FELICS_OK.  dstatus: status, or for a valid header the decode call's own rules -- w * h < 2^32
// (FELICS_E_INVALID_DIMENSIONS) and at least C * (64 + max(0, w * h - 2)) bits behind the header (FELICS_E_IO).
struct DecodeHeader {
    uint32_t W, H;
    uint8_t color, depth;
    int8_t status, dstatus;
};
hipError_t launch_read_headers(hipStream_t s, const uint8_t *streams, const uint64_t *offsets, const uint64_t *lens, uint32_t n,
                               DecodeHeader *out);
// ---- Mixed shapes in one decode call (felics_decompress_images_device).
// A stream decoded by a wave of its own: k_decode8 / k_decode16 take blockIdx.x, the RGB conversions blockIdx.y as the row (scalar loads).
struct DecodeRow {
    uint32_t stream;     // index into offsets / lens / status
    uint32_t W, H, color;
    uint64_t out_off;    // byte offset of the frame in the caller's pixels
    uint64_t plane_off;  // RGB: element offset of its Y / Co / Cg planes in the planes buffer
};
// k_decode8_lanes: a row per wave (every stream of a wave has one shape), a slot per lane
struct LaneWave {
    uint32_t W, H;
    uint32_t first, n;   // slots first .. first + n - 1 (n <= 64; the lanes past n stay idle)
};
struct LaneSlot {
    uint32_t stream;     // index into offsets / lens / status; the slot's index names its estimator table
    uint32_t table_row;  // k_decode16_lanes: first row of the slot's estimator tables in the launch's table (k_decode8_lanes: unused, 0)
    uint64_t out_off;    // element offset: gray, of the frame in the caller's pixels; RGB, of its planes in `planes`
};
// one launch per LDS class: lds = decode8_lds_bytes of the class's widest row; RGB rows through the int16 `planes`
hipError_t launch_decode8_rows(hipStream_t s, const uint8_t *streams, const uint64_t *offsets, const uint64_t *lens, const DecodeRow *rows,
                               uint32_t n, uint32_t lds, uint64_t max_npix, bool any_rgb, uint8_t *pixels, int16_t *planes, int *status);
// waves of one colour; RGB: conv = a DecodeRow per slot for the conversion; `table` zeroed, decode8_lanes_table_bytes(slots, color) bytes
hipError_t launch_decode8_lanes_waves(hipStream_t s, const uint8_t *streams, const uint64_t *offsets, const uint64_t *lens, const LaneWave *waves,
                                      uint32_t nwaves, const LaneSlot *slots, uint32_t color, const DecodeRow *conv, uint32_t nconv,
                                      uint64_t max_npix, uint8_t *pixels, int16_t *planes, uint32_t *table, int *status);
// 16-bit waves of one colour (k_decode16_lanes<.., LaneMixed>): slot j's tables start at row slots[j].table_row of `table` and take
// planes * dec16l_rows(W * H, planes) rows; out_off in samples (u16 of the caller's pixels / int32 of `planes`)
hipError_t launch_decode16_lanes_waves(hipStream_t s, const uint8_t *streams, const uint64_t *offsets, const uint64_t *lens, const LaneWave *waves,
                                       uint32_t nwaves, const LaneSlot *slots, uint32_t color, const DecodeRow *conv, uint32_t nconv,
                                       uint64_t max_npix, uint16_t *pixels, int32_t *planes, uint32_t *table, uint32_t epoch0, int *status);
// a pass of 16-bit rows: row j uses estimator table j
hipError_t launch_decode16_rows(hipStream_t s, const uint8_t *streams, const uint64_t *offsets, const uint64_t *lens, const DecodeRow *rows,
                                uint32_t n, uint32_t lds, uint64_t max_npix, bool any_rgb, uint16_t *pixels, int32_t *planes, uint32_t *table,
                                uint32_t epoch0, int *status);
// ---- Decoding into views (felics_decompress_views_device).  The tables above stay as they are; a launch whose streams write through
// views gets a PARALLEL table of ViewRow, one per DecodeRow (views[j] belongs to rows[j]) or per LaneSlot (views[j] to slots[j]):
//   gray  : data = the first sample's address, row_stride = the pitch (>= W samples; the other strides are unused) -- the pitched
//           policies DecPitched / LanePitched, for surfaces and crops written where they lie;
//   RGB   : the view's four fields as the caller gave them -- the conversion kernels' ConvStrided policy (any strides).
// pitched / strided say whether the launch needs those policies at all: without them it is the launch above, views unused, and the
// rows' and slots' out_off are absolute addresses (`pixels` = nullptr).
struct DecodeViews {
    const ViewRow *views = nullptr;
    bool pitched = false;   // a gray row / slot of the launch has a pitch other than its width
    bool strided = false;   // an RGB row of the launch is not the dense interleaved layout
};
hipError_t launch_decode8_rows_views(hipStream_t s, const uint8_t *streams, const uint64_t *offsets, const uint64_t *lens, const DecodeRow *rows,
                                     uint32_t n, uint32_t lds, uint64_t max_npix, bool any_rgb, int16_t *planes, int *status, const DecodeViews &dv);
hipError_t launch_decode16_rows_views(hipStream_t s, const uint8_t *streams, const uint64_t *offsets, const uint64_t *lens, const DecodeRow *rows,
                                      uint32_t n, uint32_t lds, uint64_t max_npix, bool any_rgb, int32_t *planes, uint32_t *table, uint32_t epoch0,
                                      int *status, const DecodeViews &dv);
// lane form: dv.views is per slot for the gray launch (pitched), cv.views per conversion row for the RGB one (strided)
hipError_t launch_decode8_lanes_waves_views(hipStream_t s, const uint8_t *streams, const uint64_t *offsets, const uint64_t *lens, const LaneWave *waves,
                                            uint32_t nwaves, const LaneSlot *slots, uint32_t color, const DecodeRow *conv, uint32_t nconv,
                                            uint64_t max_npix, int16_t *planes, uint32_t *table, int *status, const DecodeViews &dv,
                                            const DecodeViews &cv);
hipError_t launch_decode16_lanes_waves_views(hipStream_t s, const uint8_t *streams, const uint64_t *offsets, const uint64_t *lens, const LaneWave *waves,
                                             uint32_t nwaves, const LaneSlot *slots, uint32_t color, const DecodeRow *conv, uint32_t nconv,
                                             uint64_t max_npix, int32_t *planes, uint32_t *table, uint32_t epoch0, int *status,
                                             const DecodeViews &dv, const DecodeViews &cv);
// A dense frame (W * H * C samples of T at src) written through a view: the inverse of launch_gather_view, for a whole table in one
// launch per sample type.  Row j is skipped unless status[rows[j].stream] == FELICS_OK.
struct ScatterRow {
    uint32_t stream, W, H, C;
    const void *src;
    ViewRow v;
};
template <typename T>
hipError_t launch_scatter_views(hipStream_t s, const ScatterRow *rows, uint32_t n, uint32_t max_row_samples, uint32_t max_h, const int *status);

// ---- 16-bit samples (felics_wide.hip): contexts 0..131070 and 15 Rice parameters (traits.rs:35-43).
// The events of a batch are compacted into 64-bit records {context, Rice operand, sample index in its plane},
// ordered by (plane, context) with a stable radix sort (two 9-bit passes per plane; the records are written plane by
// plane) and every context's chain is replayed by one wave; lengths / pack are the kernels above on u16 / i32 planes.
constexpr uint32_t WIDE_MAX_PLANE_PIXELS = 1u << 29;  // the sample index in a record has 29 bits

void launch_rgb16_to_planes(hipStream_t s, const uint16_t *rgb, int32_t *planes, uint32_t npix, uint32_t nimg);
// mixed sub-batch: image i's pixels from table[3 i].image, its i32 planes to table[3 i + c].samples
void launch_rgb16_to_planes_mixed(hipStream_t s, const PlaneGeom *table, uint32_t max_npix, uint32_t nimg);
// mixed sub-batch of RGB16 views: image i read through rows[i] (strides in bytes, even), its i32 planes as launch_rgb16_to_planes_mixed
void launch_rgb16_view_to_planes(hipStream_t s, const PlaneGeom *table, const ViewRow *rows, uint32_t max_npix, uint32_t nimg);

struct WideSizes {
    uint32_t px_tiles, max_sort_tiles;
    size_t tile_cnt_bytes, meta_bytes, rec_bytes, hist_bytes, heads_bytes, digtot_bytes;
};
WideSizes wide_sizes(const Geometry &g);

// count -> scan -> emit: the records of all events, plane by plane in raster order; meta = totals and per-plane ranges
template <typename T>
void launch_wide_events(hipStream_t s, const T *planes, uint32_t *tile_cnt, uint32_t *meta, uint64_t *recs, const Geometry &g);
// stable sort by context inside every plane; the result is in recs_a again
void launch_wide_sort(hipStream_t s, uint64_t *recs_a, uint64_t *recs_b, const uint32_t *meta, uint32_t *hist, uint32_t *dig_tot,
                      const Geometry &g);
// chain heads and the replay of the estimator along every chain: k_map[plane * npix + i] = k.  counters = {heads, chains
// handed over}: two words, zero beforehand.  lane_limit != 0: four lanes per chain for its first lane_limit events
// (k_wide_chains_quad), the wave-per-chain kernel for the rest (long_heads: 8 bytes, long_state: 64 bytes per chain handed
// over, wide_long_capacity() of them); lane_limit == 0: the wave-per-chain kernel alone.
constexpr uint32_t WIDE_LANE_LIMIT_MIN = 2048, WIDE_LANE_LIMIT_MAX = 4096;
constexpr uint64_t WIDE_LANE_MIN_SAMPLES = 96u << 20;  // (measured: 8 4K planes 1.28 against 1.49 ms for the wave-wide form, 16: 2.74 against 2.31, 32: 5.40 against 3.60)
uint32_t wide_lane_limit(const Geometry &g);
size_t wide_long_capacity(const Geometry &g, uint32_t lane_limit);
void launch_wide_chains(hipStream_t s, const uint64_t *recs, const uint32_t *meta, uint64_t *heads, uint32_t *counters,
                        uint8_t *k_map, const Geometry &g, uint32_t lane_limit, uint64_t *long_heads, uint32_t *long_state);

}  // namespace felics
