// felics_index16.hip -- the encoder's side of the restart index of 16-bit streams (felics.h "Restart index: 16-bit streams", format
// version 2): the indexes of every image of a pass of run_wide, from what the pass leaves in the lane's workspace --
// the sorted event records and the chain heads, the pack tiles' bit offsets, the planes (gfx950).
//
// A checkpoint (plane c, segment j, p0 = j * segment_pixels) holds a state row for context x iff x's chain has two consecutive
// events a, b with pix_a < p0 <= pix_b: the fifteen counters as they stand before b.  Five kernels per pass:
//   k_wide_index_mark   a thread per sorted record: a record whose predecessor is of its chain and of an earlier segment sets the bit
//                       of its context in the bitmap of every checkpoint between the two (65 536 or 131 072 bits per checkpoint)
//   k_wide_index_rank   a workgroup per checkpoint: the exclusive prefix of the bitmap words' popcounts, and n_rows
//   k_wide_index_plan   a workgroup per image: rows_off of every checkpoint, chained from rows_base, and the index's total bytes
//   (the host reads the totals, places the indexes one behind the other and says which of them fit the caller's buffer)
//   k_wide_index_rows   a wave per chain in k_wide_chains' wave-wide form, every chain from zero and with no k: a lane whose event lies
//                       in a later segment than the event before it writes the counters before its event as the row of every checkpoint
//                       between the two, at the place the bitmap and its prefix name -- so the rows stand in context order whatever
//                       order the chains are walked in
//   k_wide_index_head   a thread per dword of header, directory and windows (everything in front of rows_base, padding included)
// Every byte of an index is written by exactly one thread, so the caller's buffer is not cleared first.
//
// The same five in TABLE-DRIVEN form (k_wide_index_*_t; felics_compress_views_device_indexed16): a sub-batch whose images differ in
// shape or segment.  What the uniform kernels take once per launch from Index16Emit -- K, segment_pixels, W, H, the layout, where the
// samples lie -- comes from an Index16Geom row per plane, indexed by plane the way the mixed encode kernels index PlaneGeom
// (wave-uniform: scalar loads); checkpoint (plane, j) of the workspace lies at row.cp0 + j.  The chain walk and the head of an index
// are device functions both forms call.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <type_traits>

#include "../../include/felics.h"
#include "felics_device.h"
#include "felics_index.h"
#include "felics_kernels.h"
#include "felics_widerec.h"

namespace felics {

namespace {

constexpr uint32_t I16_THREADS = 256;

// exclusive prefix of v over the I16_THREADS threads of a workgroup (wsum: 4 words of LDS); *total = sum
__device__ __forceinline__ uint32_t block_excl_scan256(uint32_t v, uint32_t *wsum, uint32_t *total) {
    const uint32_t inc = wave_incl_scan(v);
    const uint32_t wave = threadIdx.x >> 6;
    __syncthreads();
    if (lane_id() == 63) wsum[wave] = inc;
    __syncthreads();
    uint32_t off = 0, tot = 0;
    for (uint32_t w = 0; w < I16_THREADS / 64; w++) {
        if (w < wave) off += wsum[w];
        tot += wsum[w];
    }
    *total = tot;
    return off + inc - v;
}

// Mark.  Workgroups (x, y): plane y (strided), the plane's sorted records strided over x.  A record's chain predecessor is the record
// in front of it if that is of the same plane and context.
__global__ __launch_bounds__(I16_THREADS) void k_wide_index_mark(const uint64_t *__restrict__ recs, const uint32_t *__restrict__ meta,
                                                                 Index16Emit e) {
    for (uint32_t plane = blockIdx.y; plane < e.nplanes; plane += gridDim.y) {
        const uint32_t first = meta[WMETA_EV0 + plane], end = meta[WMETA_EV0 + plane + 1];
        uint32_t *maps = e.bitmap + (uint64_t)plane * e.K * e.wpc;
        for (uint64_t i = (uint64_t)first + 1u + blockIdx.x * I16_THREADS + threadIdx.x; i < end; i += (uint64_t)gridDim.x * I16_THREADS) {
            const uint64_t a = recs[i - 1], b = recs[i];
            const uint32_t ctx = rec_ctx(b);
            if (rec_ctx(a) != ctx || (ctx >> 5) >= e.wpc) continue;  // (a context the plane cannot have: never, and no address follows it)
            const uint32_t ja = rec_pix(a) / e.segment_pixels, jb = min(rec_pix(b) / e.segment_pixels, e.K - 1u);  // (pix < npix: jb < K anyway)
            for (uint32_t j = ja + 1u; j <= jb; j++) atomicOr(maps + (uint64_t)j * e.wpc + (ctx >> 5), 1u << (ctx & 31u));
        }
    }
}

// The table-driven form: the divisor, the clamp and the bitmaps' place are the plane's own.  The predecessor test is the same -- the
// record in front, inside the plane's range of meta, of the same context -- so the last chain of a plane and the first chain of the
// next one, which may be of one context, stay apart.
__global__ __launch_bounds__(I16_THREADS) void k_wide_index_mark_t(const uint64_t *__restrict__ recs, const uint32_t *__restrict__ meta,
                                                                   Index16TableEmit t) {
    for (uint32_t plane = blockIdx.y; plane < t.nplanes; plane += gridDim.y) {
        const Index16Geom *g = t.rows + plane;
        const uint32_t K = g->K, seg = g->segment_pixels;
        if (K < 2u) continue;  // no index asked for, or checkpoint 0 alone: no bit to set
        const uint32_t first = meta[WMETA_EV0 + plane], end = meta[WMETA_EV0 + plane + 1];
        uint32_t *maps = t.bitmap + (uint64_t)g->cp0 * t.wpc;
        for (uint64_t i = (uint64_t)first + 1u + blockIdx.x * I16_THREADS + threadIdx.x; i < end; i += (uint64_t)gridDim.x * I16_THREADS) {
            const uint64_t a = recs[i - 1], b = recs[i];
            const uint32_t ctx = rec_ctx(b);
            if (rec_ctx(a) != ctx || (ctx >> 5) >= t.wpc) continue;
            const uint32_t ja = rec_pix(a) / seg, jb = min(rec_pix(b) / seg, K - 1u);
            for (uint32_t j = ja + 1u; j <= jb; j++) atomicOr(maps + (uint64_t)j * t.wpc + (ctx >> 5), 1u << (ctx & 31u));
        }
    }
}

// One checkpoint's bitmap by its workgroup: the exclusive prefix of the words' popcounts, and n_rows.  A thread takes wpc / 256
// consecutive words.
__device__ __forceinline__ void index16_rank_checkpoint(const uint32_t *__restrict__ bitmap, uint32_t *__restrict__ prefix,
                                                        uint32_t *__restrict__ n_rows, uint32_t wpc, uint64_t cp, uint32_t *wsum) {
    const uint32_t per = wpc / I16_THREADS;  // 8 or 16
    const uint32_t *map = bitmap + cp * wpc + threadIdx.x * per;
    uint32_t *pre = prefix + cp * wpc + threadIdx.x * per;
    uint32_t w[16], n = 0;
#pragma unroll
    for (uint32_t i = 0; i < 16; i++) {
        w[i] = i < per ? map[i] : 0u;
        n += (uint32_t)__popc(w[i]);
    }
    uint32_t total;
    uint32_t at = block_excl_scan256(n, wsum, &total);
#pragma unroll
    for (uint32_t i = 0; i < 16; i++)
        if (i < per) {
            pre[i] = at;
            at += (uint32_t)__popc(w[i]);
        }
    if (threadIdx.x == 0) n_rows[cp] = total;
}

// Rank.  Workgroup (j, y): checkpoint j of plane y (strided).
__global__ __launch_bounds__(I16_THREADS) void k_wide_index_rank(Index16Emit e) {
    __shared__ uint32_t wsum[I16_THREADS / 64];
    const uint32_t j = blockIdx.x;
    for (uint32_t plane = blockIdx.y; plane < e.nplanes; plane += gridDim.y)
        index16_rank_checkpoint(e.bitmap, e.prefix, e.n_rows, e.wpc, (uint64_t)plane * e.K + j, wsum);
}

// The table-driven form needs no table: the sub-batch's checkpoints are 0 .. ncps - 1 of the workspace, strided over the workgroups.
__global__ __launch_bounds__(I16_THREADS) void k_wide_index_rank_t(Index16TableEmit t) {
    __shared__ uint32_t wsum[I16_THREADS / 64];
    for (uint64_t cp = blockIdx.x; cp < t.ncps; cp += gridDim.x) index16_rank_checkpoint(t.bitmap, t.prefix, t.n_rows, t.wpc, cp, wsum);
}

// Plan.  Workgroup i: the C K entries of image i in (plane, segment) order.  totals[2 i] = the index's bytes, [2 i + 1] = its rows.
// (one image by its workgroup: its E entries are n_rows[0 .. E - 1]; totals: the image's two words)
__device__ __forceinline__ void index16_plan_image(const uint32_t *__restrict__ n_rows, uint64_t *__restrict__ rows_off, uint32_t E,
                                                   uint64_t rows_base, uint64_t *__restrict__ totals, uint32_t *wsum) {
    uint64_t carry = 0;
    for (uint32_t base = 0; base < E; base += I16_THREADS) {
        const uint32_t i = base + threadIdx.x;
        const uint32_t v = i < E ? n_rows[i] : 0u;
        uint32_t total;
        const uint32_t at = block_excl_scan256(v, wsum, &total);
        if (i < E) rows_off[i] = rows_base + (uint64_t)INDEX16_ROW_BYTES * (carry + at);
        carry += total;
    }
    if (threadIdx.x == 0) {
        totals[0] = rows_base + (uint64_t)INDEX16_ROW_BYTES * carry;
        totals[1] = carry;
    }
}
__global__ __launch_bounds__(I16_THREADS) void k_wide_index_plan(Index16Emit e, uint64_t rows_base) {
    __shared__ uint32_t wsum[I16_THREADS / 64];
    const uint32_t img = blockIdx.x, E = e.planes_per_image * e.K;
    index16_plan_image(e.n_rows + (uint64_t)img * E, e.rows_off + (uint64_t)img * E, E, rows_base, e.totals + 2ull * img, wsum);
}
// The table-driven form: image i's entries are the C K checkpoints from its first plane's cp0 on (its planes follow each other in the
// table and have one K), chained from its own rows_base.  An image that asks for no index (K = 0) gets totals of zero.
__global__ __launch_bounds__(I16_THREADS) void k_wide_index_plan_t(Index16TableEmit t) {
    __shared__ uint32_t wsum[I16_THREADS / 64];
    for (uint32_t img = blockIdx.x; img < t.nimages; img += gridDim.x) {
        const Index16Geom *g = t.rows + (uint64_t)img * t.planes_per_image;
        const uint32_t K = g->K;
        if (K == 0) {
            if (threadIdx.x == 0) t.totals[2ull * img] = t.totals[2ull * img + 1u] = 0;
            continue;
        }
        index16_plan_image(t.n_rows + g->cp0, t.rows_off + g->cp0, t.planes_per_image * K, g->rows_base, t.totals + 2ull * img, wsum);
    }
}

__device__ __forceinline__ void store_row(uint8_t *dst, const uint32_t (&v)[16]) {  // (dst is 64-byte aligned)
    uint4 *d = reinterpret_cast<uint4 *>(dst);
#pragma unroll
    for (uint32_t q = 0; q < 4; q++) d[q] = make_uint4(v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]);
}

// Rows.  k_wide_chains' block step (felics_wide.hip: 64 events a step, fifteen prefix sums, the halvings found by ballot) in a copy of
// its own, so that kernel's code stays what it is; here no k is chosen or stored and every chain starts from zero, whichever kernel gave
// its events their k.  In the resolve loop the lanes an iteration serves (from `base` to the halving at f) have the counters before
// their event in S + P - len: S as it stands in THAT iteration (S alone may have wrapped mod 2^32; a halving turns it into
// ((S + P(f)) >> 1) - P(f)).  A served lane whose event is of a later segment than the event before it -- the lane before; for
// lane 0 the last event of the block before, carried over; a chain's first event has none -- writes them as the row of every checkpoint
// between the two.  Rows are rare beside events (some 20 per 1000 pixels at 64 segments per 4K frame): the stores are under a branch.
// index16_chain_rows is one chain by its wave, for both forms of the kernel: records j .. of context ctx up to plane_end.  The
// checkpoints of the chain's plane are cp0 .. cp0 + K - 1 of the workspace ws; index: the index of the plane's image.
struct Index16Ws {
    const uint32_t *bitmap, *prefix, *n_rows;
    const uint64_t *rows_off;
    uint32_t wpc;
};
__device__ __forceinline__ void index16_chain_rows(const uint64_t *__restrict__ recs, uint32_t j, uint32_t plane_end, uint32_t ctx,
                                                   uint8_t *index, uint64_t cp0, uint32_t K, uint32_t segment_pixels, const Index16Ws &ws) {
    const uint32_t lane = lane_id();
    const uint32_t word = ctx >> 5, below = (1u << (ctx & 31u)) - 1u;
    uint32_t S[WIDE_NK];
#pragma unroll
    for (int k = 0; k < WIDE_NK; k++) S[k] = 0u;
    const uint32_t last_rec = plane_end - 1u;
    uint32_t carry_seg = 0xFFFFFFFFu;  // segment of the chain's last event so far (none yet: no crossing)
    uint64_t cur = recs[min(j + lane, last_rec)];
    for (;;) {
        const bool valid = j + lane < plane_end && rec_ctx(cur) == ctx;
        const uint64_t vm = __ballot(valid);  // a prefix of the lanes
        const uint32_t nvalid = (uint32_t)__popcll(vm);
        if (nvalid == 0) break;
        const uint64_t nx = recs[min(j + 64u + lane, last_rec)];
        const uint32_t ev = valid ? rec_e(cur) : 0u;
        const uint32_t seg = rec_pix(cur) / segment_pixels;
        uint32_t seg_before = (uint32_t)__shfl_up((int)seg, 1);
        if (lane == 0) seg_before = min(carry_seg, seg);
        const bool cross = valid && seg_before < seg;
        uint32_t P[WIDE_NK];
#pragma unroll
        for (int k = 0; k < WIDE_NK; k++) P[k] = wave_incl_scan(valid ? (ev >> k) + 1u + (uint32_t)k : 0u);  // rice_coding.rs:40-46
        uint32_t base = 0;  // first event of the block not yet resolved
        while (true) {
            uint32_t after_min = 0xFFFFFFFFu;
#pragma unroll
            for (int k = 0; k < WIDE_NK; k++) after_min = min(after_min, S[k] + P[k]);
            const bool live = valid && lane >= base;
            const uint64_t hm = __ballot(live && after_min > WIDE_HALVE);
            const uint32_t f = hm ? (uint32_t)__builtin_ctzll(hm) : nvalid - 1u;  // last event served by these counters
            if (cross && live && lane <= f) {
                uint32_t row[16];
#pragma unroll
                for (int k = 0; k < WIDE_NK; k++) row[k] = S[k] + P[k] - ((ev >> k) + 1u + (uint32_t)k);
                row[INDEX16_ROW_CTX] = ctx;
                for (uint32_t jj = seg_before + 1u; jj <= seg && jj < K; jj++) {
                    const uint64_t cp = cp0 + jj;
                    const uint32_t rank = ws.prefix[cp * ws.wpc + word] + (uint32_t)__popc(ws.bitmap[cp * ws.wpc + word] & below);
                    if (rank < ws.n_rows[cp]) store_row(index + ws.rows_off[cp] + (uint64_t)INDEX16_ROW_BYTES * rank, row);
                }
            }
            if (!hm) {
#pragma unroll
                for (int k = 0; k < WIDE_NK; k++) S[k] += readlane(P[k], nvalid - 1u);
                break;
            }
#pragma unroll
            for (int k = 0; k < WIDE_NK; k++) {
                const uint32_t pf = readlane(P[k], f);
                S[k] = ((S[k] + pf) >> 1) - pf;
            }
            base = f + 1u;
            if (base >= nvalid) {  // the halving fell on the block's last event: carry the counters over as they are
#pragma unroll
                for (int k = 0; k < WIDE_NK; k++) S[k] += readlane(P[k], nvalid - 1u);
                break;
            }
        }
        if (nvalid < 64u) break;
        carry_seg = readlane(seg, 63u);
        j += 64u;
        cur = nx;
    }
}

__global__ __launch_bounds__(256) void k_wide_index_rows(const uint64_t *__restrict__ recs, const uint32_t *__restrict__ meta,
                                                         const uint64_t *__restrict__ heads, const uint32_t *__restrict__ nheads, Index16Emit e) {
    const uint32_t nchains = *nheads;
    const uint32_t wave0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6));
    const uint32_t nwaves = (gridDim.x * blockDim.x) >> 6;
    const Index16Ws ws{e.bitmap, e.prefix, e.n_rows, e.rows_off, e.wpc};
    for (uint32_t c = wave0; c < nchains; c += nwaves) {
        const uint64_t hd = heads[c];
        const uint32_t j = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)hd);
        const uint32_t plane = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(hd >> 32));
        const uint64_t at = e.index_off[plane / e.planes_per_image];  // where the image's index goes; ~0: it does not fit the caller's buffer
        if (at == ~0ull) continue;
        const uint32_t plane_end = meta[WMETA_EV0 + plane + 1];
        if (plane_end - j < 2u) continue;  // (a chain of one event crosses nothing)
        const uint32_t ctx = rec_ctx(recs[j]);
        if ((ctx >> 5) >= e.wpc) continue;  // (as in k_wide_index_mark)
        index16_chain_rows(recs, j, plane_end, ctx, e.index + at, (uint64_t)plane * e.K, e.K, e.segment_pixels, ws);
    }
}

// The table-driven form: the chain's plane names its row -- K, the segment, the plane's first checkpoint and its image.
__global__ __launch_bounds__(256) void k_wide_index_rows_t(const uint64_t *__restrict__ recs, const uint32_t *__restrict__ meta,
                                                           const uint64_t *__restrict__ heads, const uint32_t *__restrict__ nheads,
                                                           Index16TableEmit t) {
    const uint32_t nchains = *nheads;
    const uint32_t wave0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6));
    const uint32_t nwaves = (gridDim.x * blockDim.x) >> 6;
    const Index16Ws ws{t.bitmap, t.prefix, t.n_rows, t.rows_off, t.wpc};
    for (uint32_t c = wave0; c < nchains; c += nwaves) {
        const uint64_t hd = heads[c];
        const uint32_t j = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)hd);
        const uint32_t plane = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(hd >> 32));
        if (plane >= t.nplanes) continue;  // (never: no row, no address)
        const Index16Geom *g = t.rows + plane;
        const uint32_t K = g->K;
        if (K < 2u) continue;  // no index asked for (K = 0), or one without a row (K = 1)
        const uint64_t at = t.index_off[g->image];  // ~0: the index does not fit the caller's buffer
        if (at == ~0ull) continue;
        const uint32_t plane_end = meta[WMETA_EV0 + plane + 1];
        if (plane_end - j < 2u) continue;
        const uint32_t ctx = rec_ctx(recs[j]);
        if ((ctx >> 5) >= t.wpc) continue;
        index16_chain_rows(recs, j, plane_end, ctx, t.index + at, (uint64_t)g->cp0, K, g->segment_pixels, ws);
    }
}

// Header, directory, windows.  Workgroups (x, i): the dwords of image i's index in front of rows_base, strided over x.  T = u16 (gray
// frames) or i32 (Y / Co / Cg planes).  Bit offsets by version 1's rules (k_index_windows): plane 0's first pack tile carries the stream
// header's bits, so tile_bitoff counts from the stream's first byte there; a later plane's counts from the plane's start.
// (One image for both forms of the kernel.  h: what the image's head is written from -- plane0: its first plane in the sub-batch, which
// indexes plane_base / plane_carry and, times the sub-batch's pack_tiles, tile_bitoff; cp0: that plane's first checkpoint in the
// workspace; plane_of(c): the samples of its plane c.)
struct Index16Head {
    uint32_t *out;
    uint32_t C, K, W, H, segment_pixels, color, plane0;
    uint64_t cp0, total;
    uint64_t win_base, win_bytes, rows_base;
};
template <typename T, typename PlaneOf>
__device__ __forceinline__ void index16_head_image(const Index16Head &h, PlaneOf plane_of, const uint64_t *__restrict__ tile_bitoff,
                                                   const uint64_t *__restrict__ plane_base, const uint64_t *__restrict__ plane_carry,
                                                   uint32_t pack_tiles, const uint32_t *__restrict__ n_rows, const uint64_t *__restrict__ rows_off) {
    uint32_t *out = h.out;
    const uint32_t C = h.C, E = C * h.K, plane0 = h.plane0;
    const uint32_t dir_end = (INDEX_HEADER_BYTES + INDEX16_ENTRY_BYTES * E) / 4u;  // (E < 2^26: K <= 2^29 / 4096 per plane)
    const uint64_t win_end = h.win_base + (uint64_t)E * h.win_bytes, w2 = 2ull * h.W;
    const uint32_t seg_tiles = h.segment_pixels / PACK_TILE;
    static_assert(PACK_TILE == FELICS_INDEX_GRANULE, "a segment is a whole number of pack tiles");
    for (uint64_t d = (uint64_t)blockIdx.x * I16_THREADS + threadIdx.x; d < h.rows_base / 4u; d += (uint64_t)gridDim.x * I16_THREADS) {
        uint32_t v = 0;
        if (d < INDEX_HEADER_BYTES / 4u) {
            const uint32_t q = (uint32_t)d;
            if (q == 0) v = 0x58434C46u;  // "FLCX"
            else if (q == 1) v = INDEX16_VERSION | (h.color << 16) | ((uint32_t)FELICS_DEPTH_16 << 24);
            else if (q == 2) v = h.W;
            else if (q == 3) v = h.H;
            else if (q == 4) v = h.segment_pixels;
            else if (q == 5) v = h.K;
            else if (q < IDX16_TOTAL / 4u) {
                const uint32_t c = (q - IDX_PLANE_END / 4u) >> 1;
                const uint64_t end = c < C ? plane_base[plane0 + c] + plane_carry[plane0 + c] : 0ull;
                v = (uint32_t)(q & 1u ? end >> 32 : end);
            } else if (q < IDX16_RESERVED / 4u) {
                v = (uint32_t)(q & 1u ? h.total >> 32 : h.total);
            }
        } else if (d < dir_end) {
            const uint32_t q = (uint32_t)d - INDEX_HEADER_BYTES / 4u, en = q / (INDEX16_ENTRY_BYTES / 4u), f = q % (INDEX16_ENTRY_BYTES / 4u);
            const uint32_t c = en / h.K, j = en % h.K, plane = plane0 + c;
            if (f < 2u) {
                const uint64_t base = plane_base[plane];
                const uint64_t bit = j ? base + tile_bitoff[(uint64_t)plane * pack_tiles + (uint64_t)j * seg_tiles] : (c ? base : STREAM_HEADER_BITS);
                v = (uint32_t)(f ? bit >> 32 : bit);
            } else if (f < 4u) {
                const uint64_t ro = rows_off[h.cp0 + en];
                v = (uint32_t)(f & 1u ? ro >> 32 : ro);
            } else if (f == 4u) {
                v = n_rows[h.cp0 + en];
            }
        } else if (4u * d >= h.win_base && 4u * d < win_end) {
            const uint64_t off = 4u * d - h.win_base;
            const uint32_t en = (uint32_t)(off / h.win_bytes);
            const uint64_t r = off - (uint64_t)en * h.win_bytes;
            const uint32_t c = en / h.K, j = en % h.K;
            const T *pl = plane_of(c);
            const uint64_t p0 = (uint64_t)j * h.segment_pixels;
            // samples p0 - 2 W .. p0 - 1; in front of the plane, and behind the window's 2 W samples: zeros
            if constexpr (sizeof(T) == 2) {
                const uint64_t s = r / 2u;
                const uint32_t lo = s < w2 && p0 + s >= w2 ? (uint32_t)pl[p0 + s - w2] : 0u;
                const uint32_t hi = s + 1u < w2 && p0 + s + 1u >= w2 ? (uint32_t)pl[p0 + s + 1u - w2] : 0u;
                v = lo | (hi << 16);
            } else {
                const uint64_t s = r / 4u;
                v = s < w2 && p0 + s >= w2 ? (uint32_t)pl[p0 + s - w2] : 0u;
            }
        }
        out[d] = v;
    }
}
template <typename T>
__global__ __launch_bounds__(I16_THREADS) void k_wide_index_head(const T *__restrict__ planes, const uint64_t *__restrict__ tile_bitoff,
                                                                 const uint64_t *__restrict__ plane_base, const uint64_t *__restrict__ plane_carry,
                                                                 uint32_t pack_tiles, Index16Emit e, Index16Layout L) {
    for (uint32_t img = blockIdx.y; img < e.nimages; img += gridDim.y) {
        const uint64_t at = e.index_off[img];
        if (at == ~0ull) continue;
        const uint32_t C = e.planes_per_image, plane0 = img * C;
        const Index16Head h{reinterpret_cast<uint32_t *>(e.index + at), C, e.K, e.W, e.H, e.segment_pixels, e.color, plane0, (uint64_t)plane0 * e.K,
                            e.totals[2ull * img], L.win_base, L.win_bytes, L.rows_base};
        index16_head_image<T>(h, [&](uint32_t c) { return planes + (uint64_t)(plane0 + c) * e.npix; }, tile_bitoff, plane_base, plane_carry,
                              pack_tiles, e.n_rows, e.rows_off);
    }
}
// The table-driven form: W, H, K, the segment and the layout from the image's first row, every plane's samples from its own row (u16
// with row length W for gray, the i32 Y / Co / Cg plane for RGB).  pack_tiles: the sub-batch's padded tile count, tile_bitoff's stride.
template <typename T>
__global__ __launch_bounds__(I16_THREADS) void k_wide_index_head_t(const uint64_t *__restrict__ tile_bitoff, const uint64_t *__restrict__ plane_base,
                                                                   const uint64_t *__restrict__ plane_carry, uint32_t pack_tiles,
                                                                   Index16TableEmit t) {
    for (uint32_t img = blockIdx.y; img < t.nimages; img += gridDim.y) {
        const uint32_t C = t.planes_per_image, plane0 = img * C;
        const Index16Geom *g = t.rows + plane0;
        if (g->K == 0) continue;  // no index asked for
        const uint64_t at = t.index_off[img];
        if (at == ~0ull) continue;
        const Index16Head h{reinterpret_cast<uint32_t *>(t.index + at), C, g->K, g->W, g->H, g->segment_pixels, t.color, plane0, (uint64_t)g->cp0,
                            t.totals[2ull * img], g->win_base, g->win_bytes, g->rows_base};
        index16_head_image<T>(h, [&](uint32_t c) { return (const T *)g[c].samples; }, tile_bitoff, plane_base, plane_carry, pack_tiles, t.n_rows,
                              t.rows_off);
    }
}

}  // namespace

uint32_t index16_words_per_checkpoint(uint32_t color) { return (color ? INDEX16_CONTEXTS + 1u : 65536u) / 32u; }

void launch_index16_scan(hipStream_t s, const uint64_t *recs, const uint32_t *meta, const Geometry &g, const Index16Emit &e) {
    if (e.K == 0 || g.nplanes == 0) return;
    const Index16Layout L = index16_layout(g.W, g.H, g.color, e.segment_pixels);
    const uint32_t by = std::min(g.nplanes, 4096u);
    (void)hipMemsetAsync(e.bitmap, 0, (size_t)g.nplanes * e.K * e.wpc * 4u, s);
    if (e.K > 1) {
        const uint32_t bx = std::max(1u, std::min((g.npix + I16_THREADS * 8u - 1u) / (I16_THREADS * 8u), 64u));
        FELICS_LAUNCH(k_wide_index_mark, dim3(bx, by), dim3(I16_THREADS), s, recs, meta, e);
    }
    FELICS_LAUNCH(k_wide_index_rank, dim3(e.K, by), dim3(I16_THREADS), s, e);
    FELICS_LAUNCH(k_wide_index_plan, dim3(g.nimages), dim3(I16_THREADS), s, e, L.rows_base);
}

void launch_index16_write(hipStream_t s, const void *planes, const uint64_t *recs, const uint32_t *meta, const uint64_t *heads, const uint32_t *nheads,
                          const uint64_t *tile_bitoff, const uint64_t *plane_base, const uint64_t *plane_carry, const Geometry &g,
                          const Index16Emit &e) {
    if (e.K == 0 || g.nplanes == 0) return;
    const Index16Layout L = index16_layout(g.W, g.H, g.color, e.segment_pixels);
    // persistent, as k_wide_chains: 8 workgroups of 4 waves per CU share the chains
    if (e.K > 1) FELICS_LAUNCH(k_wide_index_rows, dim3(256u * 8u), dim3(256), s, recs, meta, heads, nheads, e);
    const uint32_t bx = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((L.rows_base / 4u + I16_THREADS - 1u) / I16_THREADS, 1024u));
    const uint32_t by = std::min(g.nimages, 4096u);
    if (g.planes_per_image == 3)
        FELICS_LAUNCH((k_wide_index_head<int32_t>), dim3(bx, by), dim3(I16_THREADS), s, (const int32_t *)planes, tile_bitoff, plane_base,
                      plane_carry, g.pack_tiles, e, L);
    else
        FELICS_LAUNCH((k_wide_index_head<uint16_t>), dim3(bx, by), dim3(I16_THREADS), s, (const uint16_t *)planes, tile_bitoff, plane_base,
                      plane_carry, g.pack_tiles, e, L);
}

void launch_index16_scan_table(hipStream_t s, const uint64_t *recs, const uint32_t *meta, const Index16TableEmit &t, uint32_t max_npix) {
    if (t.ncps == 0 || t.nplanes == 0) return;
    const uint32_t by = std::min(t.nplanes, 4096u);
    (void)hipMemsetAsync(t.bitmap, 0, (size_t)t.ncps * t.wpc * 4u, s);
    const uint32_t bx = std::max(1u, std::min((max_npix + I16_THREADS * 8u - 1u) / (I16_THREADS * 8u), 64u));
    FELICS_LAUNCH(k_wide_index_mark_t, dim3(bx, by), dim3(I16_THREADS), s, recs, meta, t);
    // (the checkpoints of a sub-batch can be many more than a grid should carry: 2048 workgroups stride over them)
    FELICS_LAUNCH(k_wide_index_rank_t, dim3((uint32_t)std::min<uint64_t>(t.ncps, 2048u)), dim3(I16_THREADS), s, t);
    FELICS_LAUNCH(k_wide_index_plan_t, dim3(std::min(t.nimages, 2048u)), dim3(I16_THREADS), s, t);
}

void launch_index16_write_table(hipStream_t s, const uint64_t *recs, const uint32_t *meta, const uint64_t *heads, const uint32_t *nheads,
                                const uint64_t *tile_bitoff, const uint64_t *plane_base, const uint64_t *plane_carry, uint32_t pack_tiles,
                                const Index16TableEmit &t, uint64_t max_rows_base) {
    if (t.ncps == 0 || t.nplanes == 0) return;
    FELICS_LAUNCH(k_wide_index_rows_t, dim3(256u * 8u), dim3(256), s, recs, meta, heads, nheads, t);  // (persistent, as k_wide_index_rows)
    const uint32_t bx = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((max_rows_base / 4u + I16_THREADS - 1u) / I16_THREADS, 1024u));
    const uint32_t by = std::min(t.nimages, 4096u);
    if (t.planes_per_image == 3)
        FELICS_LAUNCH((k_wide_index_head_t<int32_t>), dim3(bx, by), dim3(I16_THREADS), s, tile_bitoff, plane_base, plane_carry, pack_tiles, t);
    else
        FELICS_LAUNCH((k_wide_index_head_t<uint16_t>), dim3(bx, by), dim3(I16_THREADS), s, tile_bitoff, plane_base, plane_carry, pack_tiles, t);
}

}  // namespace felics
