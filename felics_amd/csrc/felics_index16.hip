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

// Rank.  Workgroup (j, y): checkpoint j of plane y (strided); a thread takes wpc / 256 consecutive words.
__global__ __launch_bounds__(I16_THREADS) void k_wide_index_rank(Index16Emit e) {
    __shared__ uint32_t wsum[I16_THREADS / 64];
    const uint32_t j = blockIdx.x, per = e.wpc / I16_THREADS;  // 8 or 16
    for (uint32_t plane = blockIdx.y; plane < e.nplanes; plane += gridDim.y) {
        const uint64_t cp = (uint64_t)plane * e.K + j;
        const uint32_t *map = e.bitmap + cp * e.wpc + threadIdx.x * per;
        uint32_t *pre = e.prefix + cp * e.wpc + threadIdx.x * per;
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
        if (threadIdx.x == 0) e.n_rows[cp] = total;
    }
}

// Plan.  Workgroup i: the C K entries of image i in (plane, segment) order.  totals[2 i] = the index's bytes, [2 i + 1] = its rows.
__global__ __launch_bounds__(I16_THREADS) void k_wide_index_plan(Index16Emit e, uint64_t rows_base) {
    __shared__ uint32_t wsum[I16_THREADS / 64];
    const uint32_t img = blockIdx.x, E = e.planes_per_image * e.K;
    const uint32_t *n_rows = e.n_rows + (uint64_t)img * E;
    uint64_t *rows_off = e.rows_off + (uint64_t)img * E;
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
        e.totals[2ull * img] = rows_base + (uint64_t)INDEX16_ROW_BYTES * carry;
        e.totals[2ull * img + 1u] = carry;
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
__global__ __launch_bounds__(256) void k_wide_index_rows(const uint64_t *__restrict__ recs, const uint32_t *__restrict__ meta,
                                                         const uint64_t *__restrict__ heads, const uint32_t *__restrict__ nheads, Index16Emit e) {
    const uint32_t lane = lane_id();
    const uint32_t nchains = *nheads;
    const uint32_t wave0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)((blockIdx.x * blockDim.x + threadIdx.x) >> 6));
    const uint32_t nwaves = (gridDim.x * blockDim.x) >> 6;
    for (uint32_t c = wave0; c < nchains; c += nwaves) {
        const uint64_t hd = heads[c];
        uint32_t j = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)hd);
        const uint32_t plane = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(hd >> 32));
        const uint64_t at = e.index_off[plane / e.planes_per_image];  // where the image's index goes; ~0: it does not fit the caller's buffer
        if (at == ~0ull) continue;
        const uint32_t plane_end = meta[WMETA_EV0 + plane + 1];
        if (plane_end - j < 2u) continue;  // (a chain of one event crosses nothing)
        const uint32_t ctx = rec_ctx(recs[j]);
        if ((ctx >> 5) >= e.wpc) continue;  // (as in k_wide_index_mark)
        uint8_t *const index = e.index + at;
        const uint64_t cp0 = (uint64_t)plane * e.K;
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
            const uint32_t seg = rec_pix(cur) / e.segment_pixels;
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
                    for (uint32_t jj = seg_before + 1u; jj <= seg && jj < e.K; jj++) {
                        const uint64_t cp = cp0 + jj;
                        const uint32_t rank = e.prefix[cp * e.wpc + word] + (uint32_t)__popc(e.bitmap[cp * e.wpc + word] & below);
                        if (rank < e.n_rows[cp]) store_row(index + e.rows_off[cp] + (uint64_t)INDEX16_ROW_BYTES * rank, row);
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
}

// Header, directory, windows.  Workgroups (x, i): the dwords of image i's index in front of rows_base, strided over x.  T = u16 (gray
// frames) or i32 (Y / Co / Cg planes).  Bit offsets by version 1's rules (k_index_windows): plane 0's first pack tile carries the stream
// header's bits, so tile_bitoff counts from the stream's first byte there; a later plane's counts from the plane's start.
template <typename T>
__device__ __forceinline__ void index16_head_image(const T *__restrict__ planes, const uint64_t *__restrict__ tile_bitoff,
                                                   const uint64_t *__restrict__ plane_base, const uint64_t *__restrict__ plane_carry,
                                                   uint32_t pack_tiles, const Index16Emit &e, const Index16Layout &L, uint32_t img) {
    const uint64_t at = e.index_off[img];
    if (at == ~0ull) return;
    uint32_t *out = reinterpret_cast<uint32_t *>(e.index + at);
    const uint32_t C = e.planes_per_image, E = C * e.K, plane0 = img * C;
    const uint32_t dir_end = (INDEX_HEADER_BYTES + INDEX16_ENTRY_BYTES * E) / 4u;  // (E < 2^26: K <= 2^29 / 4096 per plane)
    const uint64_t win_end = L.win_base + (uint64_t)E * L.win_bytes, w2 = 2ull * e.W;
    const uint32_t seg_tiles = e.segment_pixels / PACK_TILE;
    static_assert(PACK_TILE == FELICS_INDEX_GRANULE, "a segment is a whole number of pack tiles");
    for (uint64_t d = (uint64_t)blockIdx.x * I16_THREADS + threadIdx.x; d < L.rows_base / 4u; d += (uint64_t)gridDim.x * I16_THREADS) {
        uint32_t v = 0;
        if (d < INDEX_HEADER_BYTES / 4u) {
            const uint32_t q = (uint32_t)d;
            if (q == 0) v = 0x58434C46u;  // "FLCX"
            else if (q == 1) v = INDEX16_VERSION | (e.color << 16) | ((uint32_t)FELICS_DEPTH_16 << 24);
            else if (q == 2) v = e.W;
            else if (q == 3) v = e.H;
            else if (q == 4) v = e.segment_pixels;
            else if (q == 5) v = e.K;
            else if (q < IDX16_TOTAL / 4u) {
                const uint32_t c = (q - IDX_PLANE_END / 4u) >> 1;
                const uint64_t end = c < C ? plane_base[plane0 + c] + plane_carry[plane0 + c] : 0ull;
                v = (uint32_t)(q & 1u ? end >> 32 : end);
            } else if (q < IDX16_RESERVED / 4u) {
                const uint64_t total = e.totals[2ull * img];
                v = (uint32_t)(q & 1u ? total >> 32 : total);
            }
        } else if (d < dir_end) {
            const uint32_t q = (uint32_t)d - INDEX_HEADER_BYTES / 4u, en = q / (INDEX16_ENTRY_BYTES / 4u), f = q % (INDEX16_ENTRY_BYTES / 4u);
            const uint32_t c = en / e.K, j = en % e.K, plane = plane0 + c;
            if (f < 2u) {
                const uint64_t base = plane_base[plane];
                const uint64_t bit = j ? base + tile_bitoff[(uint64_t)plane * pack_tiles + (uint64_t)j * seg_tiles] : (c ? base : STREAM_HEADER_BITS);
                v = (uint32_t)(f ? bit >> 32 : bit);
            } else if (f < 4u) {
                const uint64_t ro = e.rows_off[(uint64_t)plane0 * e.K + en];
                v = (uint32_t)(f & 1u ? ro >> 32 : ro);
            } else if (f == 4u) {
                v = e.n_rows[(uint64_t)plane0 * e.K + en];
            }
        } else if (4u * d >= L.win_base && 4u * d < win_end) {
            const uint64_t off = 4u * d - L.win_base;
            const uint32_t en = (uint32_t)(off / L.win_bytes);
            const uint64_t r = off - (uint64_t)en * L.win_bytes;
            const uint32_t c = en / e.K, j = en % e.K;
            const T *pl = planes + (uint64_t)(plane0 + c) * e.npix;
            const uint64_t p0 = (uint64_t)j * e.segment_pixels;
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
    for (uint32_t img = blockIdx.y; img < e.nimages; img += gridDim.y)
        index16_head_image(planes, tile_bitoff, plane_base, plane_carry, pack_tiles, e, L, img);
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

}  // namespace felics
