// felics_index.hip -- the encoder's side of the restart index (felics.h): the index of every image of a pass, from
// what the 8-bit pipeline has computed anyway and would throw away (gfx950).
//
// At a tile boundary the decoder needs the estimator's state, the bit position and the 2 W samples in front of it:
//   * k_spine3 leaves the six counters at the start of every 16-event record (ChainSlice::state16), and runtab names the first
//     record of every context in every 4096-pixel tile -- so the state of context c before pixel p0 = T * 4096 is the state of
//     the first record of c in the first tile t >= T that has events of c (no event of c lies between), and if no tile has any
//     the state is never read again: zeros.  That is the index's canonical form (felics_index_build zeroes the same rows);
//   * the pack stage leaves every tile's bit offset in its plane (tile_bitoff; plane 0's first tile carries the 112 header bits)
//     and every plane's bits (plane_carry) and base in the stream (plane_base);
//   * the samples are still in memory: the caller's frames (gray), the lane's Y / Co / Cg planes (RGB).
// Two kernels per pass, both plain vector loads and stores, on the index zeroed beforehand (what they do not write is zero: the
// states of segment 0, the canonical zeros, windows in front of the plane, padding, reserved bytes).
// Two forms of each: the uniform ones for a pass of one shape (felics_compress_batch_device_indexed), and the mixed ones for a
// sub-batch of images of any shapes, layouts and segments (felics_compress_views_device_indexed), which take per plane what the
// uniform ones take per pass from a table row of their own (IndexGeom, beside PlaneGeom / PitchedGeom).
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/felics.h"
#include "felics_device.h"
#include "felics_index.h"
#include "felics_kernels.h"

namespace felics {

namespace {

constexpr uint32_t NO_TILE = 0xFFFFFFFFu;

// States.  One wave per chain (plane, context), a lane per checkpoint interval: lane j looks through the seg_tiles tiles between
// checkpoint j and j + 1 for the first one with events of the context -- every run-table entry is read once, by one lane --
// and an interval without any takes the find of the nearest interval behind it (a ballot and a shuffle inside the chunk of 64
// intervals, a carried find across chunks, which run from the plane's end down).  No thread scans to the end of the plane.
// Two kernels: the uniform pass's, and the mixed sub-batch's, written as the three steps below.

// The first tile of [t0, t1) with events of the chain whose run-table row is `run`, and the chain's first record in it.
// (eight entries asked for at a time: a load per entry that waits for the test of the one before it is a chain of memory
// latencies as long as the interval)
__device__ __forceinline__ void first_run(const uint32_t *run, uint32_t t0, uint32_t t1, uint32_t &hit_t, uint32_t &hit_r) {
    for (uint32_t t = t0; t < t1 && hit_t == NO_TILE; t += 8) {
        uint32_t v[8];
#pragma unroll
        for (uint32_t i = 0; i < 8; i++) v[i] = t + i < t1 ? run[t + i] : 0u;
#pragma unroll
        for (uint32_t i = 0; i < 8; i++)
            if (hit_t == NO_TILE && (v[i] >> 16)) {
                hit_t = t + i;
                hit_r = v[i] & 0xFFFFu;
            }
    }
}

// A chunk of 64 intervals: every lane's own find (hit_t, hit_r) becomes the find of the nearest interval at or behind it -- in the
// chunk, else the carried one -- and the chunk's first find is carried to the chunks in front of it.
__device__ __forceinline__ void nearest_find(uint32_t lane, uint32_t hit_t, uint32_t hit_r, uint32_t &carry_t, uint32_t &carry_r, uint32_t &t,
                                             uint32_t &r) {
    const uint64_t found = __ballot(hit_t != NO_TILE);
    const uint64_t ahead = found >> lane;  // this interval and the later ones of the chunk
    const int src = ahead ? (int)(lane + (uint32_t)__builtin_ctzll(ahead)) : (int)lane;
    t = (uint32_t)__shfl((int)hit_t, src), r = (uint32_t)__shfl((int)hit_r, src);
    if (!ahead) {
        t = carry_t;
        r = carry_r;
    }
    if (found) {
        const int first = __builtin_ctzll(found);
        carry_t = (uint32_t)__shfl((int)hit_t, first);
        carry_r = (uint32_t)__shfl((int)hit_r, first);
    }
}

// the counters as the format stores them, u16 little-endian (S0 | S1 << 16, ...), to context ctx's row of a checkpoint
__device__ __forceinline__ void put_state(uint8_t *cp, uint32_t ctx, const uint4 &st) {
    uint32_t *dst = reinterpret_cast<uint32_t *>(cp + CP_STATE_OFF + ctx * 12u);
    dst[0] = st.x;
    dst[1] = st.y;
    dst[2] = st.z;
}

// (The uniform kernel is written out as it was: with any of the three steps factored out of it the compiler allocates it 28 VGPRs
// instead of 26 -- profiles/tools/kernel_meta.py -- and its figures are to stay.  The mixed form is made of the steps.)
__global__ __launch_bounds__(64) void k_index_states(const uint32_t *__restrict__ runtab, const uint4 *__restrict__ state16, uint32_t cap,
                                                     IndexEmit e) {
    const uint32_t chain = blockIdx.x, plane = chain / e.nctx, ctx = chain % e.nctx;
    const uint32_t img = plane / e.planes_per_image, c = plane % e.planes_per_image;
    const uint32_t lane = lane_id();
    const uint32_t *run = runtab + (uint64_t)chain * e.tiles;
    uint8_t *cps = e.index + (uint64_t)img * e.index_bytes + INDEX_HEADER_BYTES + (uint64_t)c * e.K * e.cp_bytes;
    uint32_t carry_t = NO_TILE, carry_r = 0;  // the first tile with events behind the chunk at hand, and the context's first record in it
    for (int64_t base = (int64_t)((e.K - 1) / 64u) * 64; base >= 0; base -= 64) {
        const uint32_t j = (uint32_t)base + lane;
        uint32_t hit_t = NO_TILE, hit_r = 0;
        if (j < e.K) {
            const uint32_t t0 = j * e.seg_tiles, t1 = min(t0 + e.seg_tiles, e.tiles);  // (j * seg_tiles < tiles: K = ceil(tiles / seg_tiles))
            // (eight entries asked for at a time: a load per entry that waits for the test of the one before it is a chain of memory
            // latencies as long as the interval)
            for (uint32_t t = t0; t < t1 && hit_t == NO_TILE; t += 8) {
                uint32_t v[8];
#pragma unroll
                for (uint32_t i = 0; i < 8; i++) v[i] = t + i < t1 ? run[t + i] : 0u;
#pragma unroll
                for (uint32_t i = 0; i < 8; i++)
                    if (hit_t == NO_TILE && (v[i] >> 16)) {
                        hit_t = t + i;
                        hit_r = v[i] & 0xFFFFu;
                    }
            }
        }
        const uint64_t found = __ballot(hit_t != NO_TILE);
        const uint64_t ahead = found >> lane;  // this interval and the later ones of the chunk
        const int src = ahead ? (int)(lane + (uint32_t)__builtin_ctzll(ahead)) : (int)lane;
        uint32_t t = (uint32_t)__shfl((int)hit_t, src), r = (uint32_t)__shfl((int)hit_r, src);
        if (!ahead) {
            t = carry_t;
            r = carry_r;
        }
        // (segment 0 starts on a zeroed table; a record index the tile cannot hold would be a broken run table: left as zeros)
        if (j >= 1 && j < e.K && t != NO_TILE && r < cap / REC) {
            const uint4 st = state16[((uint64_t)plane * e.tiles + t) * cap / REC + r];
            uint32_t *dst = reinterpret_cast<uint32_t *>(cps + (uint64_t)j * e.cp_bytes + CP_STATE_OFF + ctx * 12u);
            dst[0] = st.x;  // S0 | S1 << 16: the counters as the format stores them, u16 little-endian
            dst[1] = st.y;
            dst[2] = st.z;
        }
        if (found) {
            const int first = __builtin_ctzll(found);
            carry_t = (uint32_t)__shfl((int)hit_t, first);
            carry_r = (uint32_t)__shfl((int)hit_r, first);
        }
    }
}

// The mixed form (a sub-batch of felics_compress_views_device_indexed): the same wave per chain.  The run-table row is as wide as
// the sub-batch's largest plane (row_tiles, which strides state16 as well); the plane's own tiles come from its PlaneGeom row -- the
// entries behind them are empty and belong to no interval -- and its index, K and seg_tiles from its IndexGeom row (wave-uniform:
// scalar loads).  A plane without an index, or with segment 0 alone (which starts on a zeroed table), leaves at once.
__global__ __launch_bounds__(64) void k_index_states_mixed(const uint32_t *__restrict__ runtab, const uint4 *__restrict__ state16, uint32_t cap,
                                                           const PlaneGeom *__restrict__ table, const IndexGeom *__restrict__ rows,
                                                           uint32_t row_tiles, uint32_t nctx, uint32_t planes_per_image) {
    const uint32_t chain = blockIdx.x, plane = (uint32_t)__builtin_amdgcn_readfirstlane((int)(chain / nctx)), ctx = chain % nctx;
    const IndexGeom ig = rows[plane];
    if (!ig.index || ig.K < 2) return;
    const uint32_t tiles = (table[plane].npix + SORT_TILE - 1) / SORT_TILE, c = plane % planes_per_image;
    const uint32_t lane = lane_id();
    const uint32_t *run = runtab + (uint64_t)chain * row_tiles;
    uint8_t *cps = ig.index + INDEX_HEADER_BYTES + (uint64_t)c * ig.K * ig.cp_bytes;
    uint32_t carry_t = NO_TILE, carry_r = 0;
    for (int64_t base = (int64_t)((ig.K - 1) / 64u) * 64; base >= 0; base -= 64) {
        const uint32_t j = (uint32_t)base + lane;
        uint32_t hit_t = NO_TILE, hit_r = 0;
        if (j < ig.K) {
            const uint32_t t0 = j * ig.seg_tiles, t1 = min(t0 + ig.seg_tiles, tiles);  // (the plane's OWN end: K = ceil(tiles / seg_tiles))
            first_run(run, t0, t1, hit_t, hit_r);
        }
        uint32_t t, r;
        nearest_find(lane, hit_t, hit_r, carry_t, carry_r, t, r);
        if (j >= 1 && j < ig.K && t != NO_TILE && r < cap / REC)
            put_state(cps + (uint64_t)j * ig.cp_bytes, ctx, state16[((uint64_t)plane * row_tiles + t) * cap / REC + r]);
    }
}

__device__ __forceinline__ void store64(uint8_t *p, uint64_t v) {  // (p is 8-byte aligned)
    reinterpret_cast<uint32_t *>(p)[0] = (uint32_t)v;
    reinterpret_cast<uint32_t *>(p)[1] = (uint32_t)(v >> 32);
}

// What thread 0 of the workgroups of checkpoint 0 adds to the windows: the plane's end, and in plane 0 the index's header.
__device__ __forceinline__ void index_plane_end(uint8_t *idx, uint32_t c, uint64_t end_bit) { store64(idx + IDX_PLANE_END + 8 * c, end_bit); }
__device__ __forceinline__ void index_header(uint8_t *idx, uint32_t color, uint32_t W, uint32_t H, uint32_t segment_pixels, uint32_t K) {
    uint32_t *h = reinterpret_cast<uint32_t *>(idx);
    h[0] = 0x58434C46u;  // "FLCX"
    h[1] = INDEX_VERSION | (color << 16) | ((uint32_t)FELICS_DEPTH_8 << 24);
    h[2] = W;
    h[3] = H;
    h[4] = segment_pixels;
    h[5] = K;
}

// Bit offsets, windows, headers.  One workgroup per (checkpoint, plane); T = u8 (gray frames) or i16 (Y / Co / Cg planes).
template <typename T>
__global__ __launch_bounds__(256) void k_index_windows(const T *__restrict__ planes, const uint64_t *__restrict__ tile_bitoff,
                                                       const uint64_t *__restrict__ plane_base, const uint64_t *__restrict__ plane_carry,
                                                       IndexEmit e) {
    const uint32_t j = blockIdx.x, plane = blockIdx.y;
    const uint32_t img = plane / e.planes_per_image, c = plane % e.planes_per_image;
    uint8_t *idx = e.index + (uint64_t)img * e.index_bytes;
    uint8_t *cp = idx + INDEX_HEADER_BYTES + ((uint64_t)c * e.K + j) * e.cp_bytes;
    // plane 0's first tile carries the stream header's bits, so tile_bitoff counts from the stream's first byte there; a later
    // plane's counts from the plane's start, plane_base bits into the stream
    const uint64_t base = plane_base[plane];
    if (threadIdx.x == 0) store64(cp, j ? base + tile_bitoff[(uint64_t)plane * e.tiles + (uint64_t)j * e.seg_tiles] : (c ? base : STREAM_HEADER_BITS));
    const uint64_t p0 = (uint64_t)j * e.seg_tiles * SORT_TILE, w2 = 2ull * e.W;
    const T *pl = planes + (uint64_t)plane * e.npix;
    T *win = reinterpret_cast<T *>(cp + e.win_off);
    for (uint64_t t = threadIdx.x; t < w2; t += 256)
        if (p0 + t >= w2) win[t] = pl[p0 + t - w2];  // samples p0 - 2 W .. p0 - 1; in front of the plane: the zeros already there
    if (j == 0 && threadIdx.x == 0) index_plane_end(idx, c, base + plane_carry[plane]);
    if (j == 0 && c == 0 && threadIdx.x == 0) index_header(idx, e.color, e.W, e.H, e.seg_tiles * SORT_TILE, e.K);
}

// The mixed form: one workgroup per (checkpoint, plane) up to the sub-batch's largest K; the plane's rows are wave-uniform (scalar
// loads) and a workgroup behind its plane's K, or of a plane without an index, leaves at once.  Sample q of the plane lies at
// samples + q / W * pitch + q % W: a pitched gray plane's rows `pitch` bytes apart (the PitchedGeom row; 64-bit addresses), every
// other plane dense (pitch = W: gray frames and the dense copies of gathered views where they lie, Y / Co / Cg in the lane's planes
// buffer, which plane_rows has put into `samples`).  q < npix: every load is a sample of the view.  Consecutive threads take
// consecutive samples of a row.
template <typename T>
__global__ __launch_bounds__(256) void k_index_windows_mixed(const PlaneGeom *__restrict__ table, const PitchedGeom *__restrict__ pitched,
                                                             const IndexGeom *__restrict__ rows, const uint64_t *__restrict__ tile_bitoff,
                                                             const uint64_t *__restrict__ plane_base, const uint64_t *__restrict__ plane_carry,
                                                             uint32_t row_tiles, uint32_t planes_per_image, uint32_t color) {
    const uint32_t j = blockIdx.x, plane = (uint32_t)__builtin_amdgcn_readfirstlane((int)blockIdx.y);
    const IndexGeom ig = rows[plane];
    if (!ig.index || j >= ig.K) return;
    const PlaneGeom pg = table[plane];
    const uint64_t pitch = pitched ? pitched[plane].pitch : (uint64_t)pg.W;
    const uint32_t c = plane % planes_per_image;
    uint8_t *idx = ig.index;
    uint8_t *cp = idx + INDEX_HEADER_BYTES + ((uint64_t)c * ig.K + j) * ig.cp_bytes;
    const uint64_t base = plane_base[plane];
    if (threadIdx.x == 0) store64(cp, j ? base + tile_bitoff[(uint64_t)plane * row_tiles + (uint64_t)j * ig.seg_tiles] : (c ? base : STREAM_HEADER_BITS));
    const uint64_t p0 = (uint64_t)j * ig.seg_tiles * SORT_TILE, w2 = 2ull * pg.W;
    const T *pl = reinterpret_cast<const T *>(pg.samples);
    T *win = reinterpret_cast<T *>(cp + ig.win_off);
    for (uint64_t t = threadIdx.x; t < w2; t += 256)
        if (p0 + t >= w2) {
            const uint32_t q = (uint32_t)(p0 + t - w2);  // (< npix < 2^32)
            win[t] = pl[(uint64_t)(q / pg.W) * pitch + q % pg.W];
        }
    if (j == 0 && threadIdx.x == 0) index_plane_end(idx, c, base + plane_carry[plane]);
    if (j == 0 && c == 0 && threadIdx.x == 0) index_header(idx, color, pg.W, pg.H, ig.seg_tiles * SORT_TILE, ig.K);
}

}  // namespace

void launch_index_emit(hipStream_t s, const void *planes, const uint32_t *runtab, const uint4 *state16, uint32_t cap, const uint64_t *tile_bitoff,
                       const uint64_t *plane_base, const uint64_t *plane_carry, const Geometry &g, uint8_t *index, uint32_t segment_pixels) {
    const IndexLayout L = index_layout(g.W, g.H, g.color, segment_pixels);
    if (L.K == 0 || g.nplanes == 0) return;
    const IndexEmit e{index, L.total, L.cp_bytes, L.win_off, g.W, g.H, g.npix, g.sort_tiles, g.nctx, g.planes_per_image, L.K, segment_pixels / SORT_TILE,
                      g.color};
    if (L.K > 1) hipLaunchKernelGGL(k_index_states, dim3(g.nplanes * g.nctx), dim3(64), 0, s, runtab, state16, cap, e);
    if (g.planes_per_image == 3)
        hipLaunchKernelGGL(k_index_windows<int16_t>, dim3(L.K, g.nplanes), dim3(256), 0, s, (const int16_t *)planes, tile_bitoff, plane_base, plane_carry, e);
    else
        hipLaunchKernelGGL(k_index_windows<uint8_t>, dim3(L.K, g.nplanes), dim3(256), 0, s, (const uint8_t *)planes, tile_bitoff, plane_base, plane_carry, e);
}

// The indexes of a mixed 8-bit sub-batch (Geometry::mixed): g's tile count is the row width of runtab, state16 and tile_bitoff, the
// plane rows name everything else.  max_K = the largest K of `rows` (0: no plane has an index).
void launch_index_emit_mixed(hipStream_t s, const uint32_t *runtab, const uint4 *state16, uint32_t cap, const uint64_t *tile_bitoff,
                             const uint64_t *plane_base, const uint64_t *plane_carry, const Geometry &g, const IndexGeom *rows, uint32_t max_K) {
    if (max_K == 0 || g.nplanes == 0) return;
    if (max_K > 1)
        hipLaunchKernelGGL(k_index_states_mixed, dim3(g.nplanes * g.nctx), dim3(64), 0, s, runtab, state16, cap, g.mixed, rows, g.sort_tiles, g.nctx,
                           g.planes_per_image);
    if (g.planes_per_image == 3)
        hipLaunchKernelGGL(k_index_windows_mixed<int16_t>, dim3(max_K, g.nplanes), dim3(256), 0, s, g.mixed, (const PitchedGeom *)nullptr, rows,
                           tile_bitoff, plane_base, plane_carry, g.sort_tiles, g.planes_per_image, g.color);
    else
        hipLaunchKernelGGL(k_index_windows_mixed<uint8_t>, dim3(max_K, g.nplanes), dim3(256), 0, s, g.mixed, g.pitched, rows, tile_bitoff, plane_base,
                           plane_carry, g.sort_tiles, g.planes_per_image, g.color);
}

}  // namespace felics
