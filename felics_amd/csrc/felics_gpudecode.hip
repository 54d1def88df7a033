// felics_gpudecode.hip -- GPU decoder for 8-bit streams (gfx950): decompress_channel of the reference
// (src/compression.rs:151-248, decode_intensity :48-61) for a whole batch of streams at once.
//
// Decoding is bit-serial per stream: the context of a pixel (its two neighbours, misc.rs:6-24) and the
// Rice parameter (the estimator's state, parameter_selection.rs:49-85) depend on everything decoded
// before it, and the planes of an RGB image share one bit stream (compression.rs:385-400: plane c + 1
// starts at the bit plane c ended on).  The only parallelism the format offers is ACROSS streams, so:
// one wave per stream, the estimator table (512 rows of six counters, 12 KiB) and the two image rows the
// neighbour rule looks at in LDS, the stream pulled in 256 bytes at a time with coalesced loads, finished
// rows stored coalesced.  A batch fills the chip from about a thousand streams up; a single stream runs at
// the speed of one wave's instruction stream: ~480 ns per pixel, whether that stream is vector code
// (round 2's first form: 112 MPix/s for 64 streams) or, as now, scalar code (134 MPix/s) -- a lone wave
// issues an instruction of either kind about every ten cycles and pays more for every taken branch.
//
// Valid streams decode to exactly the pixels the host decoder (felics_decode.cpp) produces.  Corrupt
// streams end with an error status (the code can differ from the host decoder's where both a range and a
// length check would fire), never with an out-of-bounds access: every read of the stream is bounded by its
// length and every pixel by the image size.
#include <hip/hip_runtime.h>
#include <type_traits>
#include <stdint.h>

#include "../../include/felics.h"
#include "felics_device.h"
#include "felics_index.h"
#include "felics_kernels.h"
#include "felics_lanewalk.h"

namespace felics {

// samples of an LDS row: whole 64-sample blocks (a block of the row above is read with one vector load)
__host__ __device__ static inline uint32_t decode8_row_stride(uint32_t W) { return (W + 63u) & ~63u; }

namespace {

__device__ __forceinline__ uint32_t uni(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }
__device__ __forceinline__ int unii(int v) { return __builtin_amdgcn_readfirstlane(v); }

// MSB-first bit reader over [base, base + len) in global memory (bitstream-io BitReader<_, BigEndian>).
// Everything about the position is wave-uniform and lives in scalar registers; the stream itself sits in two vector
// registers (lane j = dword j of a 256-byte chunk, big-endian order restored; the chunk after it already asked for),
// and the next dword is picked out of them with v_readlane: no LDS and no memory wait on the per-pixel path.
struct ScalarBits {
    const uint32_t *al;    // aligned-down dword pointer of the stream's first byte
    uint64_t total_dw;     // dwords from `al` that hold stream bytes
    uint64_t chunk0;       // dword index of cur's lane 0
    uint32_t cur, nxt;     // VECTOR: this chunk and the next one (zeros past the end)
    uint32_t cpos;         // next dword of `cur` to consume, 0..64
    uint64_t acc;          // unread bits, left-aligned
    uint32_t navail;       // valid bits in acc
    uint64_t end_bit;      // bits from `al` to the end of the stream

    // (whole aligned dwords: the first and the last one may hold up to three bytes that are not the stream's -- never
    // interpreted: `skew` bytes are dropped at the start, end_bit bounds the end -- and an aligned word that holds a stream
    // byte cannot leave the page that byte is in)
    __device__ __forceinline__ uint32_t fetch(uint64_t first) const {
        const uint64_t i = first + lane_id();
        return i < total_dw ? __builtin_bswap32(al[i]) : 0u;
    }
    __device__ __forceinline__ void init(const uint8_t *p, uint64_t n) {
        const uint32_t skew = (uint32_t)(reinterpret_cast<uintptr_t>(p) & 3u);
        al = reinterpret_cast<const uint32_t *>(p - skew);
        total_dw = (skew + n + 3u) >> 2;
        chunk0 = 0;
        cur = fetch(0);
        nxt = fetch(64);
        cpos = 0;
        acc = 0;
        navail = 0;
        end_bit = (skew + n) * 8u;
        refill();
        if (skew) {  // the first dword starts before the stream: drop those bytes
            acc <<= 8u * skew;
            navail -= 8u * skew;
        }
    }
    // the same, positioned `bit` bits behind p (bit <= 8 n: the caller's check, so the first chunk fetched holds a stream byte or lies
    // right behind the last one; like every fetch it is bounded by total_dw)
    __device__ __forceinline__ void init_at(const uint8_t *p, uint64_t n, uint64_t bit) {
        const uint32_t skew = (uint32_t)(reinterpret_cast<uintptr_t>(p) & 3u);
        al = reinterpret_cast<const uint32_t *>(p - skew);
        total_dw = (skew + n + 3u) >> 2;
        end_bit = (skew + n) * 8u;
        const uint64_t at = 8u * skew + bit, dw = at >> 5;
        chunk0 = dw & ~63ull;
        cur = fetch(chunk0);
        nxt = fetch(chunk0 + 64u);
        cpos = (uint32_t)(dw - chunk0);
        acc = 0;
        navail = 0;
        refill();
        acc <<= (uint32_t)(at & 31u);
        navail -= (uint32_t)(at & 31u);
    }
    // bits consumed so far, counted from p (the pointer init / init_at was given)
    __device__ __forceinline__ uint64_t pos(const uint8_t *p) const {
        return (chunk0 + cpos) * 32u - navail - 8u * (uint32_t)(reinterpret_cast<uintptr_t>(p) & 3u);
    }
    // at least 33 valid bits in acc afterwards (zeros past the end of the stream)
    __device__ __forceinline__ void refill() {
        if (navail <= 32u) {
            if (cpos == 64u) {
                cur = nxt;
                chunk0 += 64u;
                nxt = fetch(chunk0 + 64u);
                cpos = 0;
            }
            const uint32_t w = (uint32_t)__builtin_amdgcn_readlane((int)cur, (int)cpos);
            cpos++;
            acc |= (uint64_t)w << (32u - navail);
            navail += 32u;
        }
    }
    // the next n <= 32 bits; the caller has refilled (n <= navail)
    __device__ __forceinline__ uint32_t take(uint32_t n) {
        const uint32_t v = n ? (uint32_t)(acc >> (64u - n)) : 0u;
        acc <<= n;
        navail -= n;
        return v;
    }
    __device__ __forceinline__ uint32_t get(uint32_t n) {
        refill();
        return take(n);
    }
    // Bits past the end of the stream read as zeros, and whether any were handed out is worked out from the position when
    // somebody asks (at the end of every row, and wherever decoding stops): DecompressionError::IoError.  Nothing loops on
    // stream content without a bound: a run of ones ends at the first padding zero.
    __device__ __forceinline__ bool failed() const { return (chunk0 + cpos) * 32u - navail > end_bit; }
    // ones before the first zero, the zero consumed (read_unary0)
    __device__ __forceinline__ uint64_t unary0() {
        uint64_t q = 0;
        while (true) {
            refill();
            const uint32_t top = (uint32_t)(acc >> 32);
            const uint32_t ones = top == 0xFFFFFFFFu ? 32u : (uint32_t)__builtin_clz(~top);
            if (ones == 32u) {
                q += 32u;
                take(32u);
                if (failed()) return q;
                continue;
            }
            take(ones + 1u);
            return q + ones;
        }
    }
};

// Where a wave-per-stream kernel (k_decode8, k_decode16, the RGB conversions) finds its stream's shape and output: a geometry
// policy.  DecUniform: the same-shape call's arguments -- stream = row, W x H of `color`, frames and planes back to back, RGB iff
// there are planes.  DecMixed: row `row` of a DecodeRow table (the row index is wave-uniform: scalar loads).
struct DecUniform {
    uint32_t W, H, color;
};
struct DecMixed {
    const DecodeRow *rows;
};
// DecPitched (felics_decompress_views_device): a DecMixed table whose GRAY rows write where views[row] says -- data is the address
// of the row's first sample, row_stride the bytes between two of its rows (>= W samples).  RGB rows go to their planes as ever.
struct DecPitched : DecMixed {
    const ViewRow *views;
};
struct DecView {
    uint32_t img, W, H, color;  // img: the stream's index into offsets / lens / status
    uint64_t out_off, plane_off;
};
__device__ __forceinline__ DecView dec_view(const DecUniform &g, uint32_t row) { return DecView{row, g.W, g.H, g.color, 0, 0}; }
__device__ __forceinline__ DecView dec_view(const DecMixed &g, uint32_t row) {
    const DecodeRow r = g.rows[row];
    return DecView{r.stream, r.W, r.H, r.color, r.out_off, r.plane_off};
}
template <typename P>
__device__ __forceinline__ bool dec_rgb(const DecUniform &, const DecView &, const P *planes) { return planes != nullptr; }
template <typename P>
__device__ __forceinline__ bool dec_rgb(const DecMixed &, const DecView &v, const P *) { return v.color != 0; }
// the stream's frame (uniform: `per` samples of T per stream) and plane c of its planes
template <typename T>
__device__ __forceinline__ T *dec_frame(const DecUniform &, T *pixels, const DecView &v, uint64_t per) { return pixels + (uint64_t)v.img * per; }
template <typename T>
__device__ __forceinline__ T *dec_frame(const DecMixed &, T *pixels, const DecView &v, uint64_t) {
    // (as integers: in a views call `pixels` is null and out_off the frame's address, and null plus an offset is not a pointer; the
    // sum names device memory, which is said so that the stores stay global ones)
    using Global = __attribute__((address_space(1))) T;
    return (T *)reinterpret_cast<Global *>(reinterpret_cast<uintptr_t>(pixels) + v.out_off);
}
template <typename T>
__device__ __forceinline__ T *dec_frame(const DecPitched &g, T *, const DecView &, uint64_t) {
    return reinterpret_cast<T *>(const_cast<void *>(g.views[blockIdx.x].data));
}
template <typename T>
__device__ __forceinline__ T *dec_plane(const DecUniform &, T *planes, const DecView &v, uint32_t nplanes, uint32_t c, uint64_t npix) {
    return planes + ((uint64_t)v.img * nplanes + c) * npix;
}
template <typename T>
__device__ __forceinline__ T *dec_plane(const DecMixed &, T *planes, const DecView &v, uint32_t, uint32_t c, uint64_t npix) {
    return planes + v.plane_off + (uint64_t)c * npix;
}

}  // namespace

// One wave per stream.  status[i] = FELICS_OK or an error code.  Gray: u8 pixels straight to `pixels`;
// RGB: the three planes as int16 to `planes` (image i at i * 3 * npix), converted by k_ycocg8_to_rgb.
// G: DecUniform (the stream's header must be the one announced) or DecMixed (the row's shape: read from this stream's header by
// k_read_headers, so the comparison below holds).
// LDS (dynamic): table (256 or 512) x 6 u32 | rows 2 x rstride i16.
//
// The decode loop is one pixel after the other, and a lone wave retires a dependent vector instruction every ~10
// cycles: the per-pixel path is therefore written so that the compiler keeps it in SCALAR registers and instructions
// (every value that comes out of LDS or a vector register passes through readfirstlane / readlane, nothing depends on
// the lane id).  The vector side only moves data in bulk: the stream 256 bytes at a time, the row above 64 samples at
// a time (one register, read with v_readlane), the decoded row 64 samples at a time (collected with v_writelane,
// stored to LDS for the next row and to global memory coalesced).
template <typename G>
__global__ __launch_bounds__(64) void k_decode8(const uint8_t *__restrict__ streams, const uint64_t *__restrict__ offsets,
                                                const uint64_t *__restrict__ lens, G geo, uint8_t *__restrict__ pixels,
                                                int16_t *__restrict__ planes, int *__restrict__ status) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const DecView v = dec_view(geo, blockIdx.x);
    const uint32_t W = v.W, H = v.H, color = v.color;
    uint32_t *table = reinterpret_cast<uint32_t *>(smem);
    const uint32_t nctx = color ? nctx_of<int16_t>() : nctx_of<uint8_t>();  // gray: contexts 0..255, half the table
    int16_t *rows = reinterpret_cast<int16_t *>(smem + nctx * 6 * 4);
    const uint32_t rstride = decode8_row_stride(W);
    const uint32_t img = v.img, lane = lane_id();
    const uint8_t *s = streams + offsets[img];
    const uint64_t slen = lens[img];
    const uint64_t npix = (uint64_t)W * H;
    const uint32_t nplanes = color ? 3u : 1u;
    // header (format.rs:63-84) must be the one the caller announced
    int rc = FELICS_OK;
    if (slen < FELICS_HEADER_BYTES) {
        rc = FELICS_E_IO;
    } else {
        const uint32_t w = ((uint32_t)s[6] << 24) | ((uint32_t)s[7] << 16) | ((uint32_t)s[8] << 8) | s[9];
        const uint32_t h = ((uint32_t)s[10] << 24) | ((uint32_t)s[11] << 16) | ((uint32_t)s[12] << 8) | s[13];
        if (s[0] != 'F' || s[1] != 'L' || s[2] != 'C' || s[3] != 'S') rc = FELICS_E_INVALID_SIGNATURE;
        else if (s[4] > 1) rc = FELICS_E_INVALID_COLOR_TYPE;
        else if (s[5] > 1) rc = FELICS_E_INVALID_PIXEL_DEPTH;
        else if (s[4] != color || s[5] != 0 || w != W || h != H) rc = FELICS_E_INVALID_DIMENSIONS;
    }
    rc = unii(rc);
    if (rc != FELICS_OK) {
        if (lane == 0) status[img] = rc;
        return;
    }
    ScalarBits br;
    br.init(s + FELICS_HEADER_BYTES, slen - FELICS_HEADER_BYTES);
    for (uint32_t c = 0; c < nplanes && rc == FELICS_OK; c++) {
        const int32_t p0 = (int32_t)br.get(32), p1 = (int32_t)br.get(32);  // compression.rs:166-167
        if (br.failed()) {
            rc = FELICS_E_IO;
            break;
        }
        if (npix == 0) continue;
        for (uint32_t i = lane; i < nctx * 6; i += 64) table[i] = 0;  // KEstimator::new
        __builtin_amdgcn_wave_barrier();
        const bool rgb = dec_rgb(geo, v, planes);
        int16_t *outp = rgb ? dec_plane(geo, planes, v, nplanes, c, npix) : nullptr;
        uint8_t *outg = rgb ? nullptr : dec_frame(geo, pixels, v, npix);
        // DecPitched: the row's offset in the view, the pitch added in 64 bits once per row (the row above stays in LDS: the view is only written)
        uint64_t opitch = 0, orow = 0;
        if constexpr (std::is_same<G, DecPitched>::value) opitch = (uint64_t)geo.views[blockIdx.x].row_stride;
        const int lo_ok = color ? -255 : 0, hi_ok = 255;  // what a sample of this plane can be (Y 0..255, Co / Cg -255..255)
        // rows: cur = the row being decoded, prev = the one above; both in LDS, written 64 samples at a time
        uint32_t x = 0, y = 0;
        int16_t *cur = rows, *prev = rows + rstride;
        int upv = 0;   // VECTOR: prev[xb + lane] for the 64-sample block xb the walk stands in
        int rowv = 0;  // VECTOR: the samples of this block decoded so far
        int left = 0, left2 = 0;
        int first_col2 = 0;  // cur[0] as it was before this row: the sample two rows up (first-column rule)
        for (uint64_t i = 0; i < npix; i++) {
            const uint32_t xl = x & 63u;
            if (xl == 0) {
                if (y > 0) upv = (int)prev[x + lane];  // (rows are padded to whole blocks)
                // second neighbour of the row's first pixel (misc.rs:14-23): two rows up -- what cur[0] still holds --
                // or, in row 1, above-right
                if (x == 0 && y > 0) first_col2 = y >= 2 ? unii((int)cur[0]) : (W > 1 ? __builtin_amdgcn_readlane(upv, 1) : 0);
            }
            int pv;
            if (i < 2) {
                pv = i == 0 ? p0 : p1;
            } else {
                const int above = __builtin_amdgcn_readlane(upv, (int)xl);
                // misc.rs:6-24 with selects: interior = left and above; first row = the two to the left; first column =
                // above and first_col2
                const bool row0 = y == 0, col0 = x == 0 && !row0;
                const int v1 = col0 ? above : left;
                const int v2 = col0 ? first_col2 : (row0 ? left2 : above);
                const int hi = max(v1, v2), lo = min(v1, v2);
                const uint32_t ctx = (uint32_t)(hi - lo);  // <= 510 because every stored sample is in range
                br.refill();  // >= 33 bits: an in-range code has at most 11, the two flags of the other kind 2
                if (br.take(1)) {  // in range: phased-in code of p - L (phase_in_coding.rs:86-112)
                    const uint32_t n = ctx + 1;
                    const uint32_t m = 31u - (uint32_t)__builtin_clz(n);
                    const uint32_t right_p = (2u << m) - n, left_p = n - (1u << m);
                    uint32_t r = br.take(m);
                    const uint32_t longer = r >= right_p ? 1u : 0u;  // the code has one more bit
                    const uint32_t r2 = (r - right_p) * 2u + right_p + br.take(longer);
                    r = longer ? r2 : r;
                    uint32_t rot = r + left_p;  // rotate_left: (r + left_p) mod n, r < n
                    rot = rot >= n ? rot - n : rot;
                    pv = lo + (int)rot;
                } else {
                    const bool above_flag = br.take(1) != 0;
                    const uint64_t *row = reinterpret_cast<const uint64_t *>(table + ctx * 6);  // 24-byte rows: 8-byte aligned
                    const uint64_t r01 = row[0], r23 = row[1], r45 = row[2];                 // one LDS round trip for the row
                    uint32_t S[6] = {uni((uint32_t)r01), uni((uint32_t)(r01 >> 32)), uni((uint32_t)r23),
                                     uni((uint32_t)(r23 >> 32)), uni((uint32_t)r45), uni((uint32_t)(r45 >> 32))};
                    // get_k: smallest counter, ties to the largest k (parameter_selection.rs:71-85)
                    const uint32_t key = min(min(min((S[0] << 3) | 7u, (S[1] << 3) | 6u), min((S[2] << 3) | 5u, (S[3] << 3) | 4u)),
                                             min((S[4] << 3) | 3u, (S[5] << 3) | 2u));
                    const uint32_t k = 7u - (key & 7u);
                    const uint64_t q = br.unary0();
                    const uint64_t e64 = (q << k) + br.get(k);
                    if (e64 > 1024u) {  // no sample of an 8-bit plane is that far from its neighbours
                        rc = e64 > 0xFFFFFFFFull ? FELICS_E_VALUE_OVERFLOW : FELICS_E_INVALID_VALUE;
                        break;
                    }
                    const uint32_t e = (uint32_t)e64;
                    uint32_t mn = 0xFFFFFFFFu;
#pragma unroll
                    for (uint32_t kk = 0; kk < 6; kk++) {
                        S[kk] += (e >> kk) + 1u + kk;
                        mn = min(mn, S[kk]);
                    }
                    const uint32_t hsh = mn > 1024u ? 1u : 0u;
                    uint64_t *wrow = reinterpret_cast<uint64_t *>(table + ctx * 6);  // (every lane: same address, same value)
                    wrow[0] = (uint64_t)(S[0] >> hsh) | ((uint64_t)(S[1] >> hsh) << 32);
                    wrow[1] = (uint64_t)(S[2] >> hsh) | ((uint64_t)(S[3] >> hsh) << 32);
                    wrow[2] = (uint64_t)(S[4] >> hsh) | ((uint64_t)(S[5] >> hsh) << 32);
                    pv = above_flag ? hi + (int)e + 1 : lo - (int)e - 1;
                }
            }
            if (pv < lo_ok || pv > hi_ok) {  // try_into::<u8>() / the estimator's context bound would fail
                rc = FELICS_E_INVALID_VALUE;
                break;
            }
            rowv = lane == xl ? pv : rowv;  // (off the serial path: nothing reads rowv before the block is complete)
            left2 = left;
            left = pv;
            const bool row_end = x + 1 == W;
            if (xl == 63u || row_end) {  // a block of the row is complete: to LDS (the next row's `above`) and to the output
                const uint32_t xb = x & ~63u;
                if (xb + lane <= x) {
                    cur[xb + lane] = (int16_t)rowv;
                    if constexpr (std::is_same<G, DecPitched>::value) {
                        if (outg)
                            outg[orow + xb + lane] = (uint8_t)rowv;  // (xb + lane <= x < W: never the bytes between W and the pitch)
                        else
                            outp[(uint64_t)y * W + xb + lane] = (int16_t)rowv;
                    } else if (outg)
                        outg[(uint64_t)y * W + xb + lane] = (uint8_t)rowv;
                    else
                        outp[(uint64_t)y * W + xb + lane] = (int16_t)rowv;
                }
            }
            if (row_end) {
                if (br.failed()) {
                    rc = FELICS_E_IO;
                    break;
                }
                __builtin_amdgcn_wave_barrier();
                x = 0;
                y++;
                if constexpr (std::is_same<G, DecPitched>::value) orow += opitch;
                int16_t *t = cur;
                cur = prev;
                prev = t;
            } else {
                x++;
            }
        }
    }
    if (br.failed()) rc = FELICS_E_IO;  // (whatever else stopped the decoding: it was decoding padding)
    if (lane == 0) status[img] = rc;
}

// ------------------------------------------------------------------------------------------
// The restart index (felics.h, felics_index.h): ONE walk from a checkpoint, and the two kernels that are its sinks.
//
// decode8_from_checkpoint is k_decode8's walk, started in the middle of a plane: the LDS table comes out of the checkpoint's
// counters, the two LDS rows out of its window of 2 W samples, (x, y) from the segment's first pixel p0, the bit reader is positioned
// on its bit_offset.  Every check of felics.h is made here, in this order: the stream's header, the index header against it and
// against the launch's (segment_pixels, K: what the host sized the index by, so that no checkpoint is read outside index_stride), the
// segment's bit range, the window's samples, and at the end that the reader stands exactly on the next checkpoint.  The per-pixel
// path is k_decode8's (that kernel is left as it is: the unindexed call is what the indexed one is measured against).  A 64-sample
// block goes to the LDS row for every lane, because later rows read it, and to the sink from the segment's first pixel on -- the
// samples in front of p0 belong to other waves.  An empty image (K = 0) has no checkpoint: its pseudo segment reads the plane's two
// raw samples only.  LDS (dynamic): as k_decode8 (decode8_lds_bytes).
//
// What a caller of the walk decides is its Sink:
//   stop(pend)              the pixel behind the last one to decode, <= pend (the segment's end).  The end check is made only where
//                           stop is the segment's end: a walk that stops early has no checkpoint to stand on, only that the reader did
//                           not run off the stream;
//   store(col, y, at, v)    sample v of pixel at = y W + col, p0 <= at < stop, to the output.
// ------------------------------------------------------------------------------------------
namespace {

// The checks of a segment before a bit is decoded, for one (stream, index) pair: the stream's header (format.rs:63-84) must be the one
// the caller announced, the index header must fit both and the launch's (segment_pixels, K); then, if `bounds`, the bit range of
// segment (c, j).  FELICS_OK (L, and start / end if asked for, are set) or the code.  Plain per-thread code: the lane kernel
// evaluates it with a stream per lane, the wave kernels make the result uniform themselves.
__device__ __forceinline__ int indexed_segment_check(const uint8_t *s, uint64_t slen, const uint8_t *idx, uint32_t color, uint32_t W, uint32_t H,
                                                     uint32_t segment_pixels, uint32_t K, bool bounds, uint32_t c, uint32_t j, IndexLayout &L,
                                                     uint64_t &start, uint64_t &end) {
    if (slen < FELICS_HEADER_BYTES) return FELICS_E_IO;
    const uint32_t w = ((uint32_t)s[6] << 24) | ((uint32_t)s[7] << 16) | ((uint32_t)s[8] << 8) | s[9];
    const uint32_t h = ((uint32_t)s[10] << 24) | ((uint32_t)s[11] << 16) | ((uint32_t)s[12] << 8) | s[13];
    if (s[0] != 'F' || s[1] != 'L' || s[2] != 'C' || s[3] != 'S') return FELICS_E_INVALID_SIGNATURE;
    if (s[4] > 1) return FELICS_E_INVALID_COLOR_TYPE;
    if (s[5] > 1) return FELICS_E_INVALID_PIXEL_DEPTH;
    if (s[4] != color || s[5] != 0 || w != W || h != H) return FELICS_E_INVALID_DIMENSIONS;
    if (index_header_check(idx, color, W, H, slen, L) != FELICS_OK || idx_rd32(idx + IDX_SEGPIX) != segment_pixels || L.K != K)
        return FELICS_E_INVALID_INDEX;
    return bounds ? index_segment_bounds(idx, L, c, j, slen, start, end) : FELICS_OK;
}

// Segment (c, j) of stream s / index idx, decoded by the calling wave into `sink`; `smem` is the kernel's dynamic LDS.  Returns the
// segment's status, wave-uniform.  header_only: the checks of the two headers and nothing else (c and j are not looked at).
template <typename Sink>
__device__ __forceinline__ int decode8_from_checkpoint(uint8_t *smem, const uint8_t *s, uint64_t slen, const uint8_t *idx, const DecUniform &geo,
                                                       uint32_t segment_pixels, uint32_t K, uint32_t c, uint32_t j, bool header_only,
                                                       const Sink &sink) {
    const uint32_t W = geo.W, H = geo.H, color = geo.color;
    uint32_t *table = reinterpret_cast<uint32_t *>(smem);
    const uint32_t nctx = color ? nctx_of<int16_t>() : nctx_of<uint8_t>();
    int16_t *rows = reinterpret_cast<int16_t *>(smem + nctx * 6 * 4);
    const uint32_t rstride = decode8_row_stride(W);
    const uint32_t lane = lane_id();
    const uint64_t npix = (uint64_t)W * H;
    IndexLayout L;
    uint64_t start = 0, end = 0;
    int rc = unii(indexed_segment_check(s, slen, idx, color, W, H, segment_pixels, K, !header_only, c, j, L, start, end));
    if (rc != FELICS_OK || header_only) return rc;
    const uint64_t p0 = (uint64_t)j * segment_pixels, pend = min(npix, p0 + segment_pixels);  // this segment's pixels
    const uint64_t stop = sink.stop(pend);
    uint32_t x = 0, y = 0;
    int16_t *cur = rows, *prev = rows + rstride;
    if (K) {
        // the checkpoint: counters (u16 pairs -> u32 rows), then the window into the two rows -- with (x0, y0) = p0's place, window
        // sample t is pixel p0 - 2 W + t: row y0 from t = 2 W - x0 on (cur), row y0 - 1 from t = W - x0 on (prev), and in front of that
        // row y0 - 2, of which only (0, y0 - 2) is ever looked at, and only if x0 = 0 (the first-column rule: what cur[0] holds)
        const uint8_t *cp = idx + INDEX_HEADER_BYTES + ((uint64_t)c * K + j) * L.cp_bytes;
        const uint32_t *st = reinterpret_cast<const uint32_t *>(cp + CP_STATE_OFF);  // (index and checkpoints are 16-byte aligned)
        for (uint32_t i = lane; i < nctx * 3; i += 64) {
            const uint32_t w2 = st[i];
            table[2 * i] = w2 & 0xFFFFu;
            table[2 * i + 1] = w2 >> 16;
        }
        x = (uint32_t)(p0 % W);
        y = (uint32_t)(p0 / W);
        const uint8_t *win = cp + L.win_off;
        const int lo_w = color && c ? -255 : 0;
        bool bad = false;
        for (uint64_t t = lane; t < 2ull * W; t += 64) {
            if (p0 + t < 2ull * W) continue;  // in front of the plane: zeros, never looked at
            const int v = color ? (int)reinterpret_cast<const int16_t *>(win)[t] : (int)win[t];
            bad |= v < lo_w || v > 255;
            if (t >= 2ull * W - x) cur[t - (2ull * W - x)] = (int16_t)v;
            else if (t >= (uint64_t)W - x) prev[t - ((uint64_t)W - x)] = (int16_t)v;
            else if (t == 0 && x == 0) cur[0] = (int16_t)v;
        }
        if (__ballot(bad) != 0) return FELICS_E_INVALID_INDEX;
    }
    __builtin_amdgcn_wave_barrier();
    ScalarBits br;
    br.init_at(s, slen, start);
    int32_t raw0 = 0, raw1 = 0;
    if (j == 0) {  // the plane's two raw samples (compression.rs:166-167) stand in front of its first segment only
        raw0 = (int32_t)br.get(32);
        raw1 = (int32_t)br.get(32);
        if (br.failed()) rc = FELICS_E_IO;
    }
    if (rc == FELICS_OK && stop > p0) {
        const int lo_ok = color ? -255 : 0, hi_ok = 255;  // what a sample of this plane can be (Y 0..255, Co / Cg -255..255)
        const uint32_t xl0 = x & 63u;
        int upv = 0;   // VECTOR: prev[xb + lane] for the 64-sample block xb the walk stands in
        int rowv = 0;  // VECTOR: the samples of this block decoded so far
        if (xl0) {     // a start inside a block: the block's samples in front of it are the window's
            if (y > 0) upv = (int)prev[(x & ~63u) + lane];
            rowv = (int)cur[(x & ~63u) + lane];
        }
        int left = x >= 1 ? unii((int)cur[x - 1]) : 0, left2 = x >= 2 ? unii((int)cur[x - 2]) : 0;
        int first_col2 = 0;  // cur[0] as it was before this row: the sample two rows up (first-column rule)
        for (uint64_t i = p0; i < stop; i++) {
            const uint32_t xl = x & 63u;
            if (xl == 0) {
                if (y > 0) upv = (int)prev[x + lane];  // (rows are padded to whole blocks)
                if (x == 0 && y > 0) first_col2 = y >= 2 ? unii((int)cur[0]) : (W > 1 ? __builtin_amdgcn_readlane(upv, 1) : 0);
            }
            int pv;
            if (i < 2) {
                pv = i == 0 ? raw0 : raw1;
            } else {
                const int above = __builtin_amdgcn_readlane(upv, (int)xl);
                const bool row0 = y == 0, col0 = x == 0 && !row0;  // misc.rs:6-24 with selects
                const int v1 = col0 ? above : left;
                const int v2 = col0 ? first_col2 : (row0 ? left2 : above);
                const int hi = max(v1, v2), lo = min(v1, v2);
                const uint32_t ctx = (uint32_t)(hi - lo);  // <= 510 because every stored sample is in range
                br.refill();  // >= 33 bits: an in-range code has at most 11, the two flags of the other kind 2
                if (br.take(1)) {  // in range: phased-in code of p - L (phase_in_coding.rs:86-112)
                    const uint32_t n = ctx + 1;
                    const uint32_t m = 31u - (uint32_t)__builtin_clz(n);
                    const uint32_t right_p = (2u << m) - n, left_p = n - (1u << m);
                    uint32_t r = br.take(m);
                    const uint32_t longer = r >= right_p ? 1u : 0u;  // the code has one more bit
                    const uint32_t r2 = (r - right_p) * 2u + right_p + br.take(longer);
                    r = longer ? r2 : r;
                    uint32_t rot = r + left_p;  // rotate_left: (r + left_p) mod n, r < n
                    rot = rot >= n ? rot - n : rot;
                    pv = lo + (int)rot;
                } else {
                    const bool above_flag = br.take(1) != 0;
                    const uint64_t *row = reinterpret_cast<const uint64_t *>(table + ctx * 6);  // 24-byte rows: 8-byte aligned
                    const uint64_t r01 = row[0], r23 = row[1], r45 = row[2];                 // one LDS round trip for the row
                    uint32_t S[6] = {uni((uint32_t)r01), uni((uint32_t)(r01 >> 32)), uni((uint32_t)r23),
                                     uni((uint32_t)(r23 >> 32)), uni((uint32_t)r45), uni((uint32_t)(r45 >> 32))};
                    // get_k: smallest counter, ties to the largest k (parameter_selection.rs:71-85)
                    const uint32_t key = min(min(min((S[0] << 3) | 7u, (S[1] << 3) | 6u), min((S[2] << 3) | 5u, (S[3] << 3) | 4u)),
                                             min((S[4] << 3) | 3u, (S[5] << 3) | 2u));
                    const uint32_t k = 7u - (key & 7u);
                    const uint64_t q = br.unary0();
                    const uint64_t e64 = (q << k) + br.get(k);
                    if (e64 > 1024u) {  // no sample of an 8-bit plane is that far from its neighbours
                        rc = e64 > 0xFFFFFFFFull ? FELICS_E_VALUE_OVERFLOW : FELICS_E_INVALID_VALUE;
                        break;
                    }
                    const uint32_t e = (uint32_t)e64;
                    uint32_t mn = 0xFFFFFFFFu;
#pragma unroll
                    for (uint32_t kk = 0; kk < 6; kk++) {
                        S[kk] += (e >> kk) + 1u + kk;
                        mn = min(mn, S[kk]);
                    }
                    const uint32_t hsh = mn > 1024u ? 1u : 0u;
                    uint64_t *wrow = reinterpret_cast<uint64_t *>(table + ctx * 6);  // (every lane: same address, same value)
                    wrow[0] = (uint64_t)(S[0] >> hsh) | ((uint64_t)(S[1] >> hsh) << 32);
                    wrow[1] = (uint64_t)(S[2] >> hsh) | ((uint64_t)(S[3] >> hsh) << 32);
                    wrow[2] = (uint64_t)(S[4] >> hsh) | ((uint64_t)(S[5] >> hsh) << 32);
                    pv = above_flag ? hi + (int)e + 1 : lo - (int)e - 1;
                }
            }
            if (pv < lo_ok || pv > hi_ok) {  // try_into::<u8>() / the estimator's context bound would fail
                rc = FELICS_E_INVALID_VALUE;
                break;
            }
            rowv = lane == xl ? pv : rowv;
            left2 = left;
            left = pv;
            const bool row_end = x + 1 == W;
            if (xl == 63u || row_end || i + 1 == stop) {  // a block of the row is complete, or the walk is
                const uint32_t xb = x & ~63u;
                if (xb + lane <= x) {
                    cur[xb + lane] = (int16_t)rowv;  // (lanes in front of a mid-block start store back what they loaded)
                    const uint64_t at = (uint64_t)y * W + xb + lane;  // < stop: xb + lane <= x
                    if (at >= p0) sink.store(xb + lane, y, at, rowv);  // the samples in front of p0 are the segment's before this one
                }
            }
            if (row_end) {
                if (br.failed()) {
                    rc = FELICS_E_IO;
                    break;
                }
                __builtin_amdgcn_wave_barrier();
                x = 0;
                y++;
                int16_t *t = cur;
                cur = prev;
                prev = t;
            } else {
                x++;
            }
        }
    }
    if (br.failed()) rc = FELICS_E_IO;  // (whatever else stopped the decoding: it was decoding padding)
    else if (rc == FELICS_OK && stop == pend && br.pos(s) != end) rc = FELICS_E_INVALID_INDEX;  // the end check: exactly on the next checkpoint
    return rc;
}

// The three sinks of both depths' walks from a checkpoint.  T is the pixel type (uint8_t, uint16_t), P the type of an RGB plane's
// sample (int16_t, int32_t): the 8-bit kernels take <uint8_t, int16_t>, the 16-bit ones <uint16_t, int32_t>.

// The whole segment into the stream's frame (gray) or plane c of its planes: pixel `at` to out[at].  The walk hands it
// p0 <= at < pend only, so a wave writes its own segment's samples and no other.
template <typename T, typename P>
struct SegmentSink {
    T *outg;  // gray: the stream's frame; else null
    P *outp;  // RGB: plane c of the stream's planes
    __device__ __forceinline__ uint64_t stop(uint64_t pend) const { return pend; }
    __device__ __forceinline__ void store(uint32_t, uint32_t, uint64_t at, int v) const {
        if (outg) outg[at] = (T)v;
        else outp[at] = (P)v;
    }
};

// The segment's part of a region into the region's dense crop (gray, or plane c of the crop-sized planes): the walk ends
// behind the region's last pixel, and a sample is written only if its (column, row) lies inside the region -- column in [x, x + w),
// row in [y, y + h) (row < y + h holds for every at < stop) -- to (row - y) * w + (column - x), an offset below w * h.  reg and W
// are wave-uniform (scalar loads of the kernel); the store's predicate is the only divergence, once per 64-sample block.
template <typename T, typename P>
struct RegionSink {
    RegionRow reg;  // (inside the image, both sides non-zero: the host's checks)
    uint32_t W;
    T *outg;
    P *outp;
    __device__ __forceinline__ uint64_t stop(uint64_t pend) const { return min(pend, (uint64_t)(reg.y + reg.h - 1) * W + reg.x + reg.w); }
    __device__ __forceinline__ void store(uint32_t col, uint32_t y, uint64_t, int v) const {
        if (col >= reg.x && col - reg.x < reg.w && y >= reg.y && y - reg.y < reg.h) {
            const uint64_t to = (uint64_t)(y - reg.y) * reg.w + (col - reg.x);
            if (outg) outg[to] = (T)v;
            else outp[to] = (P)v;
        }
    }
};

// The whole segment into a view (felics_decompress_views_device_indexed, _indexed16): a gray sample as ONE aligned store of a T at the
// place the view's strides give pixel (col, y) -- whatever lies between the samples is never stored to, and any strides do, negative
// ones and pixel strides other than sizeof(T) included (16-bit: address and strides are even, felics_view_writable); an RGB sample to
// plane c of the row's planes as the segment sink does (the conversion writes the view).  The walk hands it p0 <= at < pend only,
// and (col, y) is a pixel of the image the view was checked against.
template <typename T, typename P>
struct ViewSink {
    uint8_t *data;  // gray: the view's first sample; else null
    int64_t row_stride, pixel_stride;
    P *outp;        // RGB: plane c of the row's planes
    __device__ __forceinline__ uint64_t stop(uint64_t pend) const { return pend; }
    __device__ __forceinline__ void store(uint32_t col, uint32_t y, uint64_t at, int v) const {
        if (data) *reinterpret_cast<T *>(data + view_sample_offset(row_stride, pixel_stride, 0, col, y, 0)) = (T)v;
        else outp[at] = (P)v;
    }
};

// A region's part of a segment straight into the region's view (felics_decompress_region_views_device_indexed and its 16-bit form):
// the walk ends where RegionSink's does, and a sample is written only if its (column, row) lies inside the window -- gray as ONE
// aligned store of a T at the place the view's strides give window sample (col - x, y - y0), as ViewSink stores a frame's; RGB to
// plane c of the region's crop-sized planes at (y - y0) * w + (col - x), as RegionSink does (the strided conversion writes the view).
// One address rule serves both: the plane is handed over as the dense view it is (row stride w * sizeof(P), pixel stride sizeof(P)),
// so the sink keeps one base and one pair of strides in scalar registers, not two targets.  Region, strides and W are wave-uniform
// (scalar loads off blockIdx.x); the store's predicate is the only divergence.
template <typename T, typename P>
struct RegionViewSink {
    RegionSink<T, P> crop;  // the window and W (its two targets stay null)
    uint8_t *base;          // gray: the view's first sample; RGB: plane c of the region's planes
    int64_t row_stride, pixel_stride;
    uint32_t rgb;
    __device__ __forceinline__ uint64_t stop(uint64_t pend) const { return crop.stop(pend); }
    __device__ __forceinline__ void store(uint32_t col, uint32_t y, uint64_t, int v) const {
        const RegionRow &reg = crop.reg;
        if (col >= reg.x && col - reg.x < reg.w && y >= reg.y && y - reg.y < reg.h) {
            uint8_t *to = base + view_sample_offset(row_stride, pixel_stride, 0, col - reg.x, y - reg.y, 0);
            if (rgb) *reinterpret_cast<P *>(to) = (P)v;
            else *reinterpret_cast<T *>(to) = (T)v;
        }
    }
    // region reg of a stream of rows of W samples (rgb: colour) into view, or into plane c of its planes at `planes`
    __device__ __forceinline__ static RegionViewSink make(const RegionRow &reg, uint32_t W, uint32_t rgb, uint32_t c, const ViewRow &view,
                                                          P *planes) {
        if (rgb)
            return RegionViewSink{{reg, W, nullptr, nullptr}, reinterpret_cast<uint8_t *>(planes + reg.plane_off + (uint64_t)c * reg.w * reg.h),
                                  (int64_t)reg.w * (int64_t)sizeof(P), (int64_t)sizeof(P), rgb};
        return RegionViewSink{{reg, W, nullptr, nullptr}, reinterpret_cast<uint8_t *>(const_cast<void *>(view.data)), view.row_stride,
                              view.pixel_stride, rgb};
    }
};

}  // namespace

// One wave per SEGMENT of a plane of a stream (felics_decompress_batch_device_indexed).  Block b is segment (img, c, j) =
// (b / (C Keff), b / Keff % C, b % Keff), Keff = max(K, 1).  seg_status[b] = FELICS_OK or the code; k_seg_status picks a stream's first.
__global__ __launch_bounds__(64) void k_decode8_seg(const uint8_t *__restrict__ streams, const uint64_t *__restrict__ offsets,
                                                    const uint64_t *__restrict__ lens, const uint8_t *__restrict__ index, uint64_t index_stride,
                                                    DecUniform geo, uint32_t segment_pixels, uint32_t K, uint8_t *__restrict__ pixels,
                                                    int16_t *__restrict__ planes, int *__restrict__ seg_status) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const uint32_t nplanes = geo.color ? 3u : 1u, keff = max(K, 1u);
    const uint32_t img = blockIdx.x / (nplanes * keff), c = blockIdx.x / keff % nplanes, j = blockIdx.x % keff;
    const uint64_t npix = (uint64_t)geo.W * geo.H;
    const SegmentSink<uint8_t, int16_t> sink{geo.color ? nullptr : pixels + (uint64_t)img * npix, geo.color ? planes + ((uint64_t)img * nplanes + c) * npix : nullptr};
    const int rc = decode8_from_checkpoint(smem, streams + offsets[img], lens[img], index + (uint64_t)img * index_stride, geo, segment_pixels, K, c,
                                           j, false, sink);
    if (lane_id() == 0) seg_status[blockIdx.x] = rc;
}

// One wave per WORK ITEM = (region, plane, needed segment) of felics_decompress_regions_device_indexed (felics.h "Restart index:
// regions"; host model: felics_decompress_region_indexed).  The host names needed segments only (j < K, p0 < stop); an item with
// seg = REGION_HEADER_ONLY ends after the header checks.  item_status[b] = FELICS_OK or the code; k_seg_status picks a region's first.
__global__ __launch_bounds__(64) void k_decode8_region(const uint8_t *__restrict__ streams, const uint64_t *__restrict__ offsets,
                                                       const uint64_t *__restrict__ lens, const uint8_t *__restrict__ index, uint64_t index_stride,
                                                       DecUniform geo, uint32_t segment_pixels, uint32_t K, const RegionRow *__restrict__ regions,
                                                       const RegionItem *__restrict__ items, uint8_t *__restrict__ pixels,
                                                       int16_t *__restrict__ planes, int *__restrict__ item_status) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const RegionItem item = items[blockIdx.x];
    const RegionRow reg = regions[item.region];
    const uint32_t img = reg.stream, c = item.plane;
    const RegionSink<uint8_t, int16_t> sink{reg, geo.W, geo.color ? nullptr : pixels + reg.out_off,
                                            geo.color ? planes + reg.plane_off + (uint64_t)c * reg.w * reg.h : nullptr};
    const int rc = decode8_from_checkpoint(smem, streams + offsets[img], lens[img], index + (uint64_t)img * index_stride, geo, segment_pixels, K, c,
                                           item.seg, item.seg == REGION_HEADER_ONLY, sink);
    if (lane_id() == 0) item_status[blockIdx.x] = rc;
}

// status[r] = the code of row r's first failing word in (plane, segment) order; one wave per row.  A row's words are
// regions[r]'s items (item0, nitems), or, without a region table, the `per` segment words of stream r.
__global__ __launch_bounds__(64) void k_seg_status(const int *__restrict__ words, const RegionRow *__restrict__ regions, uint32_t per,
                                                   int *__restrict__ status) {
    __shared__ uint32_t first;
    if (threadIdx.x == 0) first = 0xFFFFFFFFu;
    __syncthreads();
    const uint64_t word0 = regions ? regions[blockIdx.x].item0 : (uint64_t)blockIdx.x * per;
    const uint32_t count = regions ? regions[blockIdx.x].nitems : per;
    const int *mine = words + word0;
    for (uint32_t k = threadIdx.x; k < count; k += 64)
        if (mine[k] != FELICS_OK) {
            atomicMin(&first, k);
            break;
        }
    __syncthreads();
    if (threadIdx.x == 0) status[blockIdx.x] = first == 0xFFFFFFFFu ? FELICS_OK : mine[first];
}

// One wave per WORK ITEM = (row, plane, segment) of felics_decompress_views_device_indexed (felics_kernels.h; host model:
// felics_decompress_indexed_view).  Item and row are wave-uniform (blockIdx.x: scalar loads); the walk's geometry, segment_pixels and
// K are the row's, so the streams of a launch need not share a shape -- only the launch's dynamic LDS, which holds its widest row.
// item_status[b] = FELICS_OK or the code; k_seg_status picks a row's first.
__global__ __launch_bounds__(64) void k_decode8_seg_views(const uint8_t *__restrict__ streams, const uint64_t *__restrict__ offsets,
                                                          const uint64_t *__restrict__ lens, const uint8_t *__restrict__ index,
                                                          const IndexViewRow *__restrict__ rows, const IndexViewItem *__restrict__ items,
                                                          int16_t *__restrict__ planes, int *__restrict__ item_status) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const IndexViewItem item = items[blockIdx.x];
    const IndexViewRow r = rows[item.row];
    const DecUniform geo{r.W, r.H, r.color};
    const uint32_t c = item.plane;
    const ViewSink<uint8_t, int16_t> sink{r.color ? nullptr : reinterpret_cast<uint8_t *>(const_cast<void *>(r.view.data)), r.view.row_stride,
                                          r.view.pixel_stride, r.color ? planes + r.plane_off + (uint64_t)c * r.W * r.H : nullptr};
    const int rc = decode8_from_checkpoint(smem, streams + offsets[r.stream], lens[r.stream], index + r.index_off, geo, r.segment_pixels, r.K, c,
                                           item.seg, false, sink);
    if (lane_id() == 0) item_status[blockIdx.x] = rc;
}

// One wave per WORK ITEM = (region, plane, needed segment) of felics_decompress_region_views_device_indexed (felics_kernels.h; host
// model: felics_decompress_region_indexed_view).  Item, region, view and stream row are wave-uniform (blockIdx.x: scalar loads); the
// region names its stream, whose row carries the walk's geometry, segment_pixels and K, so the streams of a launch need not share a
// shape -- only the launch's dynamic LDS, which holds its widest row.  The host names needed segments only (j < K, p0 < stop).
// item_status[b] = FELICS_OK or the code; k_seg_status picks a region's first.
__global__ __launch_bounds__(64) void k_decode8_region_views(const uint8_t *__restrict__ streams, const uint64_t *__restrict__ offsets,
                                                             const uint64_t *__restrict__ lens, const uint8_t *__restrict__ index,
                                                             const RegionViewStream *__restrict__ srows, const RegionRow *__restrict__ regions,
                                                             const ViewRow *__restrict__ views, const RegionItem *__restrict__ items,
                                                             int16_t *__restrict__ planes, int *__restrict__ item_status) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const RegionItem item = items[blockIdx.x];
    const RegionRow reg = regions[item.region];
    const ViewRow view = views[item.region];
    const RegionViewStream r = srows[reg.stream];
    const DecUniform geo{r.W, r.H, r.color};
    const uint32_t c = item.plane;
    const auto sink = RegionViewSink<uint8_t, int16_t>::make(reg, r.W, r.color, c, view, planes);
    const int rc = decode8_from_checkpoint(smem, streams + offsets[reg.stream], lens[reg.stream], index + r.index_off, geo, r.segment_pixels, r.K, c,
                                           item.seg, false, sink);
    if (lane_id() == 0) item_status[blockIdx.x] = rc;
}

// The first 64 bytes of every index of felics_decompress_views_device_indexed for the host's checks: four lanes per index, a
// 16-byte word each (the indexes are 16-byte aligned), bytes where an index ends inside the word, zeros behind its end.
__global__ __launch_bounds__(256) void k_read_index_headers(const uint8_t *__restrict__ index, const uint64_t *__restrict__ idx_offsets,
                                                            const uint64_t *__restrict__ idx_lens, uint32_t n, uint8_t *__restrict__ out) {
    const uint64_t t = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const uint64_t i = t / 4;
    const uint32_t q = (uint32_t)(t % 4) * 16u;
    if (i >= n) return;
    const uint8_t *src = index + idx_offsets[i] + q;
    const uint64_t len = idx_lens[i];
    uint4 w = make_uint4(0, 0, 0, 0);
    if (len >= q + 16u) {
        w = *reinterpret_cast<const uint4 *>(src);
    } else if (len > q) {
        uint8_t b[16] = {0};
        for (uint32_t k = 0; k < (uint32_t)(len - q); k++) b[k] = src[k];
        w = make_uint4(idx_rd32(b), idx_rd32(b + 4), idx_rd32(b + 8), idx_rd32(b + 12));
    }
    *reinterpret_cast<uint4 *>(out + i * INDEX_HEADER_BYTES + q) = w;
}

// ------------------------------------------------------------------------------------------
// Sixty-four streams per wave, LANE = stream (8-bit gray, batches of hundreds of streams and more).
//
// The streams of a call have one shape, so all of them are at the same pixel at the same time: the walk over (x, y) and the
// neighbour rule's case analysis are wave-uniform, and only what depends on a stream's content differs between the lanes --
// the bit reader (a 64-bit window, the position and one prefetched dword per lane), the two neighbours, the estimator row.
// Per pixel every lane executes both kinds of code under its own flag; a wave decodes 64 pixels in about the time
// k_decode8 decodes one, at the price of memory operations that are gathers (64 addresses per instruction):
//   * the stream: one dword per lane every ~8 pixels, asked for a whole dword ahead;
//   * the row above: read back from the stream's own OUTPUT image, four samples per lane at a time (a CU sees its own
//     stores; 64 rows do not fit in LDS: 3840 x 64 bytes);
//   * the estimator table: 256 contexts x six 16-bit counters = 3 KB per stream (a counter of an 8-bit gray plane stays
//     below 2^16: the smallest grows by >= 6 per event, the largest by <= 255, so a halving period adds at most 44 000 on
//     top of the halved rest).  The first DEC8L_HOT contexts of every stream live in LDS, one dword per lane and pair of
//     counters (lane-interleaved: no bank conflict whatever the contexts), the others in a zeroed table in HBM: smooth and
//     natural content keeps to the LDS rows, noise pays an L2 round trip per event.
// Error behaviour as in k_decode8: every read of a stream is bounded by its length, a lane that has failed keeps walking
// (on zeros, its samples clamped into range so that contexts stay inside the table) and reports its first error.
// Needs W >= 8 (the read-back of the row above looks four samples ahead of a row's end).
//
// What ONE lane does -- LaneReader, the groups of four samples, the pixel step, the estimators, the walk over a plane and the walk over a
// segment -- is felics_lanewalk.h, compiled by the three lane kernels here and by the host check lanewalk_check.cpp.  A kernel keeps
// what needs the wave or the grid: the lane's view, the checks, the set-up of reader and estimator, the status.
// ------------------------------------------------------------------------------------------

namespace {

// The lane form's geometry policy.  LaneUniform: the same-shape call's arguments -- lane j of wave b is stream 64 b + j, outputs
// back to back.  LaneMixed: the wave's row (W, H, its slots: scalar loads) and the lane's slot (stream, output).
struct LaneUniform {
    uint32_t n, W, H;
};
struct LaneMixed {
    const LaneWave *waves;
    const LaneSlot *slots;
};
// LanePitched (felics_decompress_views_device, gray only): a LaneMixed launch whose lanes write where views[slot] says -- data is the
// address of the lane's first sample, row_stride the bytes between two of its rows (>= W samples).  The 64 lanes of a wave have 64
// bases and pitches (per-lane data, as LaneSlot is); (x, y) stays wave-uniform: a wave's views have one shape.
struct LanePitched : LaneMixed {
    const ViewRow *views;
};
struct LaneView {
    uint32_t W, H, img, slot;  // img: index into offsets / lens / status; slot: the estimator table
    uint64_t out_off;
};
// false: this lane has no stream
__device__ __forceinline__ bool lane_view(const LaneUniform &g, uint32_t lane, LaneView &v) {
    v = LaneView{g.W, g.H, blockIdx.x * 64 + lane, blockIdx.x * 64 + lane, 0};
    return v.img < g.n;
}
__device__ __forceinline__ bool lane_view(const LaneMixed &g, uint32_t lane, LaneView &v) {
    const LaneWave w = g.waves[blockIdx.x];
    v.W = w.W;
    v.H = w.H;
    if (lane >= w.n) return false;
    v.slot = w.first + lane;
    const LaneSlot s = g.slots[v.slot];
    v.img = s.stream;
    v.out_off = s.out_off;
    return true;
}
template <typename ST>
__device__ __forceinline__ ST *lane_plane(const LaneUniform &, void *out_base, const LaneView &v, uint32_t np, uint32_t plane, uint64_t npix) {
    return reinterpret_cast<ST *>(out_base) + ((uint64_t)v.img * np + plane) * npix;
}
template <typename ST>
__device__ __forceinline__ ST *lane_plane(const LaneMixed &, void *out_base, const LaneView &v, uint32_t, uint32_t plane, uint64_t npix) {
    return reinterpret_cast<ST *>(out_base) + v.out_off + (uint64_t)plane * npix;
}

// LanePitched: this lane's view -- its first sample, and the samples between two of its rows (the walk leaves [0, W) of no row)
template <typename ST>
__device__ __forceinline__ ST *lane_pitched(const LanePitched &g, const LaneView &v, int64_t &pitch) {
    const ViewRow vr = g.views[v.slot];
    pitch = vr.row_stride / (int64_t)sizeof(ST);
    return reinterpret_cast<ST *>(const_cast<void *>(vr.data));
}
// The header (format.rs:63-84) of a whole-stream lane must be the one the caller announced: FELICS_OK, or the code with which the
// lane leaves before it decodes anything
__device__ __forceinline__ int lane_header_check(const uint8_t *s, uint64_t slen, uint32_t color, uint32_t depth, uint32_t W, uint32_t H) {
    if (slen < FELICS_HEADER_BYTES) return FELICS_E_IO;
    const uint32_t w = ((uint32_t)s[6] << 24) | ((uint32_t)s[7] << 16) | ((uint32_t)s[8] << 8) | s[9];
    const uint32_t h = ((uint32_t)s[10] << 24) | ((uint32_t)s[11] << 16) | ((uint32_t)s[12] << 8) | s[13];
    if (s[0] != 'F' || s[1] != 'L' || s[2] != 'C' || s[3] != 'S') return FELICS_E_INVALID_SIGNATURE;
    if (s[4] > 1) return FELICS_E_INVALID_COLOR_TYPE;
    if (s[5] > 1) return FELICS_E_INVALID_PIXEL_DEPTH;
    if (s[4] != color || s[5] != depth || w != W || h != H) return FELICS_E_INVALID_DIMENSIONS;
    return FELICS_OK;
}

}  // namespace

// RGB = false: gray8 streams, u8 frames straight to `out_base`.  RGB = true: the three planes of an RGB8 stream, one after the other from
// the same bit reader (compression.rs:385-400), as int16 planes (image i at i * 3 * npix; k_ycocg8_to_rgb converts them): samples
// -255 .. 255, contexts 0 .. 510, a zeroed table of its own per plane.  A counter still fits 16 bits: the Rice operand is at most 1024
// (larger is the corrupt-stream exit), so counter 0 gains at most 1025 per event while counter 5 gains at least 38, i.e. at most 27.7 K
// before the smallest counter passes 1024 and the row is halved -- below 56 K with the halved rest on top.
// G: LaneUniform or LaneMixed (the streams of a wave have one shape either way).
template <bool RGB, typename G>
__global__ __launch_bounds__(64) void k_decode8_lanes(const uint8_t *__restrict__ streams, const uint64_t *__restrict__ offsets,
                                                      const uint64_t *__restrict__ lens, G geo, void *out_base, uint32_t *table,
                                                      int *__restrict__ status) {
    using ST = typename std::conditional<RGB, int16_t, uint8_t>::type;
    constexpr uint32_t NP = RGB ? 3u : 1u;
    constexpr uint32_t TABLE_DW = RGB ? DEC8L_TABLE_DW_RGB : DEC8L_TABLE_DW;  // per plane
    constexpr bool PITCHED = std::is_same<G, LanePitched>::value;
    static_assert(!PITCHED || !RGB, "RGB lanes write planes; their views are the conversion kernel's");
    __shared__ uint32_t hot[DEC8L_HOT * 3 * 64];  // [context][pair of counters][lane]
    const uint32_t lane = lane_id();
    LaneView v;
    if (!lane_view(geo, lane, v)) return;
    const uint32_t img = v.img, W = v.W, H = v.H;
    const uint8_t *s = streams + offsets[img];
    const uint64_t slen = lens[img];
    const uint64_t npix = (uint64_t)W * H;
    int rc = lane_header_check(s, slen, RGB ? 1 : 0, 0, W, H);
    if (rc != FELICS_OK) {  // nothing of this stream is decoded (its lane leaves; the others go on)
        status[img] = rc;
        return;
    }
    LaneReader br;
    br.init(s + FELICS_HEADER_BYTES, slen - FELICS_HEADER_BYTES);
    Lane8Step<RGB> step{{hot + lane, nullptr}, 0};
    for (uint32_t plane = 0; plane < NP; plane++) {
        for (uint32_t i = 0; i < DEC8L_HOT * 3; i++) step.est.myhot[i * 64] = 0;  // KEstimator::new (the HBM rows arrive zeroed); a lane's own column
        const int32_t p0 = (int32_t)br.get(32), p1 = (int32_t)br.get(32);  // compression.rs:166-167
        if (br.failed() && rc == FELICS_OK) rc = FELICS_E_IO;
        if (npix == 0) continue;
        step.est.tab = table + ((uint64_t)v.slot * NP + plane) * TABLE_DW;
        ST *out = lane_plane<ST>(geo, out_base, v, NP, plane, npix);
        int64_t pitch = 0;
        if constexpr (PITCHED) out = lane_pitched<ST>(geo, v, pitch);
        lane_walk_plane<ST, PITCHED>(br, step, out, pitch, W, H, p0, p1, rc);
    }
    if (br.failed() && rc == FELICS_OK) rc = FELICS_E_IO;  // (whatever else: it was decoding padding)
    status[img] = rc;
}

// ------------------------------------------------------------------------------------------
// Sixty-four SEGMENTS per wave, LANE = stream (felics_decompress_batch_device_indexed on large batches).
//
// Segment j of 64 streams of one shape starts at the same pixel p0, so at the same (x, y): 64 such segments share a wave exactly as 64
// streams share one in k_decode8_lanes, with (x, y) wave-uniform.  Wave wave0 + blockIdx.x is (group g of 64 consecutive streams,
// plane c, segment j) = (w / (C K), w / K % C, w % K); lane l is stream 64 g + l (the launch covers whole groups only).  The
// per-pixel path is k_decode8_lanes's (lane8_pixel, felics_lanewalk.h); what differs is k_decode8_seg's business:
//   * every lane makes k_decode8_seg's checks, in its order: the stream's header, the index header against it and the launch's
//     (segment_pixels, K: no checkpoint is read outside index_stride), the segment's bit range, the window's samples (a u8 sample is
//     in range whatever it holds: only the int16 windows are looked through).  A lane that fails one writes its code and leaves;
//   * the reader is a LaneReader positioned on the checkpoint's bit_offset (init_at); segment 0 reads the plane's two raw samples;
//   * the estimator is LOADED, not zeroed: the checkpoint's u16 state[nctx][6] is three dwords per context in the lane table's
//     pairing, so the first DEC8L_HOT contexts are a dword copy into the lane's LDS column and the others a dword copy into the item's
//     rows of `table` (TABLE_DW dwords per item of the launch, nothing to zero) -- the wave copies one lane's rows after the other,
//     coalesced.  d_index is only read.  The 16-bit bound of k_decode8_lanes holds for every checkpoint felics_index_build or the
//     encoder writes: its counters are a snapshot of an estimator that obeys the bound at every pixel.  A forged checkpoint can hold
//     up to 65 535 per counter; a pair's low counter can then carry into the high one -- wrong values of k for a segment whose index
//     is wrong anyway (the end check is what judges it), and no address depends on a counter;
//   * the walk from p0 to pend is lane8_walk_segment (felics_lanewalk.h): which samples of the row above come from the window and
//     which from the lane's own output, and which samples of a group are this segment's to store, is said and checked there;
//   * at the end FELICS_E_IO if the reader ran off the stream, else the end check: the bit position equals the next checkpoint's
//     bit_offset (plane_end_bit[c] behind the last), else FELICS_E_INVALID_INDEX.
// seg_status[(img * C + c) * K + j] = FELICS_OK or the code, as k_decode8_seg writes it: k_seg_status picks a stream's first.
// A lane that fails mid-walk keeps walking on zeros, its samples clamped (the lane form's rule), inside its own segment and rows.
// Needs W >= 8 and K >= 1.
// ------------------------------------------------------------------------------------------
template <bool RGB>
__global__ __launch_bounds__(64) void k_decode8_seg_lanes(const uint8_t *__restrict__ streams, const uint64_t *__restrict__ offsets,
                                                          const uint64_t *__restrict__ lens, const uint8_t *__restrict__ index,
                                                          uint64_t index_stride, uint32_t W, uint32_t H, uint32_t segment_pixels, uint32_t K,
                                                          uint32_t wave0, void *out_base, uint32_t *table, int *seg_status) {
    using ST = typename std::conditional<RGB, int16_t, uint8_t>::type;
    constexpr uint32_t NP = RGB ? 3u : 1u;
    constexpr uint32_t NCTX = RGB ? 512u : 256u;                                // rows of a checkpoint's state (IndexLayout::nctx)
    constexpr uint32_t TABLE_DW = RGB ? DEC8L_TABLE_DW_RGB : DEC8L_TABLE_DW;  // per item
    static_assert(TABLE_DW == NCTX * 3, "a checkpoint's state is the lane table's rows");
    __shared__ uint32_t hot[DEC8L_HOT * 3 * 64];  // [context][pair of counters][lane]
    const uint32_t lane = lane_id();
    const uint32_t wv = wave0 + blockIdx.x;
    const uint32_t g = wv / (NP * K), c = wv / K % NP, j = wv % K;
    const uint32_t img = g * 64 + lane;
    const uint8_t *s = streams + offsets[img];
    const uint64_t slen = lens[img];
    const uint8_t *idx = index + (uint64_t)img * index_stride;
    const uint64_t npix = (uint64_t)W * H;
    // the wave kernels' checks, a stream per lane
    uint64_t start = 0, end = 0;
    IndexLayout L;
    int rc = indexed_segment_check(s, slen, idx, RGB ? 1u : 0u, W, H, segment_pixels, K, true, c, j, L, start, end);
    // (a lane that passed has the launch's layout: shape, colour and segment_pixels are what the layout is made of)
    const IndexLayout LL = index_layout(W, H, RGB ? 1u : 0u, segment_pixels);
    const uint64_t cp_off = INDEX_HEADER_BYTES + ((uint64_t)c * K + j) * LL.cp_bytes;
    const uint64_t p0 = (uint64_t)j * segment_pixels, pend = min(npix, p0 + segment_pixels);  // this segment's pixels
    // The wave's part of the set-up, one lane's checkpoint after the other (only lanes whose checks passed: their checkpoints lie
    // inside index_stride): the cold rows of the state into the item's table rows, and the int16 window looked through.
    const uint64_t okmask = __ballot(rc == FELICS_OK);
    uint64_t badmask = 0;
    uint32_t *wtab = table + (uint64_t)blockIdx.x * 64u * TABLE_DW;
    for (uint32_t l = 0; l < 64; l++) {
        if (!((okmask >> l) & 1u)) continue;
        const uint8_t *cpl = index + (uint64_t)(g * 64 + l) * index_stride + cp_off;
        // (index, index_stride and cp_bytes are multiples of 16, the state starts 8 bytes in: 8-byte loads)
        const uint2 *src = reinterpret_cast<const uint2 *>(cpl + CP_STATE_OFF);
        uint2 *dst = reinterpret_cast<uint2 *>(wtab + (uint64_t)l * TABLE_DW);
        for (uint32_t i = DEC8L_HOT * 3 / 2 + lane; i < TABLE_DW / 2; i += 64) dst[i] = src[i];
        if (RGB) {
            const uint32_t *wd = reinterpret_cast<const uint32_t *>(cpl + LL.win_off);  // samples 2 t | 2 t + 1
            const int lo_w = c ? -255 : 0;
            bool bad = false;
            for (uint32_t t = lane; t < W; t += 64) {
                const uint32_t v2 = wd[t];
                const int a = (int)(int16_t)(v2 & 0xFFFFu), b = (int)(int16_t)(v2 >> 16);
                if (p0 + 2ull * t >= 2ull * W) bad |= a < lo_w || a > 255;  // (in front of the plane: zeros, never looked at)
                if (p0 + 2ull * t + 1 >= 2ull * W) bad |= b < lo_w || b > 255;
            }
            if (__ballot(bad) != 0) badmask |= 1ull << l;
        }
    }
    __threadfence_block();  // a lane reads rows that other lanes of its wave stored
    __builtin_amdgcn_wave_barrier();
    if (rc == FELICS_OK && ((badmask >> lane) & 1u)) rc = FELICS_E_INVALID_INDEX;
    int *my_status = seg_status + ((uint64_t)img * NP + c) * K + j;
    if (rc != FELICS_OK) {  // nothing of this segment is decoded (its lane leaves; the others go on)
        *my_status = rc;
        return;
    }
    const uint8_t *cp = idx + cp_off;
    const ST *win = reinterpret_cast<const ST *>(cp + LL.win_off);  // sample t is pixel p0 - 2 W + t
    const Lane8Estimator est{hot + lane, wtab + (uint64_t)lane * TABLE_DW};
    {
        const uint2 *st = reinterpret_cast<const uint2 *>(cp + CP_STATE_OFF);
        for (uint32_t i = 0; i < DEC8L_HOT * 3 / 2; i++) {  // the checkpoint's hot rows: a lane's own column
            const uint2 v2 = st[i];
            est.myhot[(2 * i) * 64] = v2.x;
            est.myhot[(2 * i + 1) * 64] = v2.y;
        }
    }
    ST *out = reinterpret_cast<ST *>(out_base) + ((uint64_t)img * NP + c) * npix;
    LaneReader br;
    br.init_at(s, slen, start);
    int32_t raw0 = 0, raw1 = 0;
    if (j == 0) {  // the plane's two raw samples (compression.rs:166-167) stand in front of its first segment only
        raw0 = (int32_t)br.get(32);
        raw1 = (int32_t)br.get(32);
        if (br.failed()) rc = FELICS_E_IO;
    }
    uint32_t out_of_range;
    if constexpr (!RGB) {
        out_of_range = lane8_walk_segment<RGB>(br, est, out, win, W, p0, pend, raw0, raw1, rc);
    } else {
        // The RGB kernel keeps the walk and the pixel step as its own text: through the shared functions the same statements came back
        // from the compiler about 1 % slower on this instantiation, twice in two runs (profiles/lane_fold.txt), while the gray one
        // gained.  It is lane8_walk_segment over lane8_pixel, statement for statement; the host check runs those, not this copy.
        constexpr int LO_OK = -255, HI_OK = 255;
        uint32_t *const myhot = est.myhot, *const tab = est.tab;
        // pixel q of the plane as this lane may read it: its own output from p0 on, the window in front (p0 - 2 W <= q: the callers' business)
        auto rd = [&](uint64_t q) -> int { return q >= p0 ? (int)out[q] : (int)win[2ull * W - (p0 - q)]; };
        // (x, y) and everything derived from them alone is wave-uniform
        uint32_t x = (uint32_t)(p0 % W), y = (uint32_t)(p0 / W);
        // row y - 1 from column xg (a multiple of four below W) on: four samples, or the row's last one to three
        auto load_up = [&](uint32_t xg) {
            Four<ST> f;
            const uint64_t q0 = (uint64_t)(y - 1) * W + xg;
            const uint32_t cnt = min(4u, W - xg);
            if (cnt == 4u && q0 >= p0) {
                f.load(out + q0);
            } else if (cnt == 4u && q0 + 4u <= p0) {
                f.load(win + (2ull * W - (p0 - q0)));
            } else {
                f.clear();
                for (uint32_t k = 0; k < cnt; k++) f.set(k, rd(q0 + k));
            }
            return f;
        };
        int left = x >= 1 ? (int)win[2ull * W - 1] : 0, left2 = x >= 2 ? (int)win[2ull * W - 2] : 0;
        Four<ST> up4, up4_next, out4;
        up4.clear();
        up4_next.clear();
        out4.clear();
        if (x != 0 && y > 0) {  // a start inside a row: the groups of the row above that the row's start would have asked for
            if ((x & 3u) == 0) {
                up4_next = load_up(x);  // (moved into up4 by the first pixel)
            } else {
                up4 = load_up(x & ~3u);
                if ((x & ~3u) + 4 < W) up4_next = load_up((x & ~3u) + 4);
            }
        }
        uint32_t gfirst = x & 3u;   // first sample of the current group that is this segment's to store
        out_of_range = 0;  // nonzero if a sample was outside LO_OK .. HI_OK
        int first_col2 = 0;
        for (uint64_t i = p0; i < pend; i++) {
            const uint32_t xs = x & 3u;
            if (x == 0 && y > 0) {
                up4 = load_up(0);  // row above, samples 0 .. 3 (later groups are asked for four samples ahead); W >= 8
                up4_next = load_up(4);
                // second neighbour of a row's first pixel (misc.rs:14-23): two rows up, or above-right in row 1
                first_col2 = y >= 2 ? rd((uint64_t)(y - 2) * W) : up4.get(1);
            } else if (xs == 0 && y > 0) {
                up4 = up4_next;
                if (x + 4 < W) up4_next = load_up(x + 4);
            }
            int pv;
            if (i < 2) {
                pv = i == 0 ? raw0 : raw1;
            } else {
                const int above = up4.get(xs);
                const bool row0 = y == 0, col0 = x == 0 && !row0;
                const int v1 = col0 ? above : left;
                const int v2 = col0 ? first_col2 : (row0 ? left2 : above);
                const int hi = max(v1, v2), lo = min(v1, v2);
                const uint32_t ctx = (uint32_t)(hi - lo);  // <= 255 (510): every sample kept is in range, every window sample checked
                const bool is_hot = ctx < DEC8L_HOT;
                const uint32_t hrow = min(ctx, DEC8L_HOT - 1u) * 3u * 64u;
                uint32_t w01 = myhot[hrow], w23 = myhot[hrow + 64], w45 = myhot[hrow + 128];
                br.refill();  // >= 33 valid bits: both kinds of code are read off the top 32 of them, then consumed in one go
                const uint32_t top = (uint32_t)(br.acc >> 32);
                const bool in_range = (top >> 31) != 0;
                // -- in range: `1`, then the phased-in code of p - L in m or m + 1 bits (phase_in_coding.rs:86-112)
                const uint32_t nn = ctx + 1;
                const uint32_t m = 31u - (uint32_t)__builtin_clz(nn);
                const uint32_t right_p = (2u << m) - nn, left_p = nn - (1u << m);
                const uint32_t t1 = top << 1;
                uint32_t r = (t1 >> 1) >> (31u - m);               // the m bits behind the flag
                const uint32_t extra = (t1 >> (31u - m)) & 1u;      // the bit behind them
                const uint32_t longer = r >= right_p ? 1u : 0u;     // the code has one more bit
                r = longer ? (r - right_p) * 2u + right_p + extra : r;
                uint32_t rot = r + left_p;                          // rotate_left: (r + left_p) mod n, r < n
                rot = rot >= nn ? rot - nn : rot;
                const int pv_in = lo + (int)rot;
                const uint32_t bits_in = 1u + m + longer;
                // -- out of range: `0`, above / below flag, q ones, `0`, k bits -- off the same 32 bits when it fits in them
                const bool above_flag = ((top >> 30) & 1u) != 0;
                if (!in_range && !is_hot) {  // (noise: a cold context's row comes from the item's table in HBM)
                    w01 = tab[ctx * 3 + 0];
                    w23 = tab[ctx * 3 + 1];
                    w45 = tab[ctx * 3 + 2];
                }
                uint32_t S[6] = {w01 & 0xFFFFu, w01 >> 16, w23 & 0xFFFFu, w23 >> 16, w45 & 0xFFFFu, w45 >> 16};
                // get_k: smallest counter, ties to the largest k (parameter_selection.rs:71-85)
                const uint32_t key = min(min(min((S[0] << 3) | 7u, (S[1] << 3) | 6u), min((S[2] << 3) | 5u, (S[3] << 3) | 4u)),
                                         min((S[4] << 3) | 3u, (S[5] << 3) | 2u));
                const uint32_t k = 7u - (key & 7u);
                const uint32_t t2 = top << 2;                                  // 30 bits of the stream, two zeros behind them
                const uint32_t ones = (uint32_t)__builtin_clz(~t2);            // (<= 30: ~t2 ends in ones)
                const bool fits = ones + 1u + k <= 30u;                        // unary part, its zero and the k bits lie inside the 30
                uint32_t e = (ones << k) + (((t2 << (ones & 31u)) << 1 >> 1) >> (31u - k));  // k bits behind the zero (k <= 5)
                uint32_t nbits = in_range ? bits_in : 3u + ones + k;
                if (!in_range && !fits) {
                    // a long code (or the end of the stream): the general reader, bit field by bit field
                    br.take(2);
                    const uint64_t q = br.unary0();
                    const uint64_t e64 = (q << k) + br.get(k);
                    e = (uint32_t)e64;
                    if (e64 > 1024u) {  // no sample of an 8-bit plane is that far from its neighbours
                        if (rc == FELICS_OK) rc = e64 > 0xFFFFFFFFull ? FELICS_E_VALUE_OVERFLOW : FELICS_E_INVALID_VALUE;
                        e = 0;
                    }
                    nbits = 0;
                }
                br.acc <<= nbits;  // (nbits <= 32 < the valid bits)
                br.navail -= nbits;
                if (!in_range) {
                    // update (parameter_selection.rs:49-68): add the six Rice lengths, halve when the smallest passes 1024
                    uint32_t mn = 0xFFFFFFFFu;
    #pragma unroll
                    for (uint32_t kk = 0; kk < 6; kk++) {
                        S[kk] += (e >> kk) + 1u + kk;
                        mn = min(mn, S[kk]);
                    }
                    const uint32_t hsh = mn > 1024u ? 1u : 0u;
                    w01 = (S[0] >> hsh) | ((S[1] >> hsh) << 16);
                    w23 = (S[2] >> hsh) | ((S[3] >> hsh) << 16);
                    w45 = (S[4] >> hsh) | ((S[5] >> hsh) << 16);
                    if (is_hot) {
                        myhot[hrow] = w01;
                        myhot[hrow + 64] = w23;
                        myhot[hrow + 128] = w45;
                    } else {
                        tab[ctx * 3 + 0] = w01;
                        tab[ctx * 3 + 1] = w23;
                        tab[ctx * 3 + 2] = w45;
                    }
                }
                pv = in_range ? pv_in : (above_flag ? hi + (int)e + 1 : lo - (int)e - 1);
            }
            // out of LO_OK .. HI_OK: remembered and reported at the end of the row; the sample is cut into the range so that a failed
            // lane's contexts stay inside the table
            if (RGB) {
                out_of_range |= (uint32_t)(pv - LO_OK) > (uint32_t)(HI_OK - LO_OK) ? 1u : 0u;
                pv = min(max(pv, LO_OK), HI_OK);
            } else {
                out_of_range |= (uint32_t)pv;
                pv &= 255;
            }
            out4.set(xs, pv);
            left2 = left;
            left = pv;
            const bool row_end = x + 1 == W;
            if (xs == 3u || row_end || i + 1 == pend) {  // a group is complete, or the row is, or the segment
                ST *grp = out + (i - xs);                 // the group's first sample; samples gfirst .. xs of it are this segment's
                if (xs == 3u && gfirst == 0) {
                    out4.store(grp);  // four samples: one (unaligned) store to the lane's plane
                } else {
                    for (uint32_t k = gfirst; k <= xs; k++) grp[k] = (ST)out4.get(k);
                }
                out4.clear();
                gfirst = 0;
            }
            if (row_end) {
                if (rc == FELICS_OK) rc = br.failed() ? FELICS_E_IO : ((RGB ? out_of_range != 0 : out_of_range > 255u) ? FELICS_E_INVALID_VALUE : FELICS_OK);
                x = 0;
                y++;
            } else {
                x++;
            }
        }
    }
    if (br.failed()) rc = FELICS_E_IO;  // (whatever else stopped the decoding: it was decoding padding)
    else if (rc == FELICS_OK && lane8_bad<RGB>(out_of_range)) rc = FELICS_E_INVALID_VALUE;
    else if (rc == FELICS_OK && br.bit_pos(s) != end) rc = FELICS_E_INVALID_INDEX;  // the end check: exactly on the next checkpoint
    *my_status = rc;
}

// The conversions' geometry: ConvUniform -- npix of every stream, stream = blockIdx.y, planes and frames back to back; DecMixed --
// row blockIdx.y (a gray row has nothing to convert).  False: nothing to do for this row.
struct ConvUniform {
    uint32_t npix;
};
// ConvStrided (felics_decompress_views_device): a DecMixed table whose RGB rows are written through views[row], any strides.
struct ConvStrided : DecMixed {
    const ViewRow *views;
};
template <typename P, typename T>
struct ConvView {
    uint32_t img, npix;
    const P *pl;
    T *dst;
};
template <typename P, typename T>
__device__ __forceinline__ bool conv_view(const ConvUniform &g, const P *planes, T *pixels, ConvView<P, T> &c) {
    c.img = blockIdx.y;
    c.npix = g.npix;
    c.pl = planes + (uint64_t)c.img * 3 * c.npix;
    c.dst = pixels + (uint64_t)c.img * 3 * c.npix;
    return true;
}
template <typename P, typename T>
__device__ __forceinline__ bool conv_view(const DecMixed &g, const P *planes, T *pixels, ConvView<P, T> &c) {
    const DecodeRow r = g.rows[blockIdx.y];
    c.img = r.stream;
    c.npix = r.W * r.H;
    c.pl = planes + r.plane_off;
    c.dst = reinterpret_cast<T *>(reinterpret_cast<uint8_t *>(pixels) + r.out_off);
    return r.color != 0;
}

// ConvRegion (felics_decompress_regions_device_indexed and its 16-bit form): row base + blockIdx.y of a RegionRow table -- crop-sized planes, the crop
// dense at its out_off; status is per region.
struct ConvRegion {
    const RegionRow *rows;
    uint32_t base;
};
template <typename P, typename T>
__device__ __forceinline__ bool conv_view(const ConvRegion &g, const P *planes, T *pixels, ConvView<P, T> &c) {
    const RegionRow r = g.rows[g.base + blockIdx.y];
    c.img = g.base + blockIdx.y;
    c.npix = r.w * r.h;
    c.pl = planes + r.plane_off;
    c.dst = reinterpret_cast<T *>(reinterpret_cast<uint8_t *>(pixels) + r.out_off);
    return true;
}

// ycocg_to_rgb (color_transform.rs:20-26) on the decoded planes, range-checked like try_into::<u8>()
template <typename G>
__global__ __launch_bounds__(256) void k_ycocg8_to_rgb(const int16_t *__restrict__ planes, uint8_t *__restrict__ pixels,
                                                       G geo, int *__restrict__ status) {
    ConvView<int16_t, uint8_t> cv;
    if (!conv_view(geo, planes, pixels, cv)) return;
    const uint32_t img = cv.img, npix = cv.npix;
    if (status[img] != FELICS_OK) return;
    const int16_t *pl = cv.pl;
    uint8_t *dst = cv.dst;
    bool bad = false;
    if constexpr (std::is_same<G, ConvStrided>::value) {
        // Sample by sample through the view's strides: three one-byte stores per pixel (what the dense loop below issues as well), so
        // whatever lies between the samples -- an alpha byte, the rest of a pitch, another cell, another plane -- is never stored to.
        const ViewRow vr = geo.views[blockIdx.y];
        const uint32_t W = geo.rows[blockIdx.y].W;
        uint8_t *base = reinterpret_cast<uint8_t *>(const_cast<void *>(vr.data));
        for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < npix; i += gridDim.x * blockDim.x) {
            const int yv = pl[i], co = pl[(uint64_t)npix + i], cg = pl[2ull * npix + i];
            const int t = yv - cg / 2;
            const int g = cg + t, b = t - co / 2, r = b + co;
            if ((r | g | b) < 0 || r > 255 || g > 255 || b > 255) bad = true;
            const uint32_t y = i / W, x = i - y * W;
            uint8_t *p = base + (int64_t)y * vr.row_stride + (int64_t)x * vr.pixel_stride;
            p[0] = (uint8_t)r;
            p[vr.channel_stride] = (uint8_t)g;
            p[2 * vr.channel_stride] = (uint8_t)b;
        }
    } else {
        for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < npix; i += gridDim.x * blockDim.x) {
            const int yv = pl[i], co = pl[(uint64_t)npix + i], cg = pl[2ull * npix + i];
            const int t = yv - cg / 2;  // `/` truncates toward zero like Rust's
            const int g = cg + t, b = t - co / 2, r = b + co;
            if ((r | g | b) < 0 || r > 255 || g > 255 || b > 255) bad = true;
            dst[(uint64_t)i * 3] = (uint8_t)r;
            dst[(uint64_t)i * 3 + 1] = (uint8_t)g;
            dst[(uint64_t)i * 3 + 2] = (uint8_t)b;
        }
    }
    if (bad) atomicCAS(&status[img], FELICS_OK, FELICS_E_INVALID_VALUE);
}

// ------------------------------------------------------------------------------------------
// 16-bit streams (traits.rs:35-43: fifteen Rice parameters, contexts 0 .. 131 070).
//
// The same walk, one wave per stream, with the estimator table where it fits: in HBM, 131 071 rows of sixteen words per
// stream (fifteen counters + the EPOCH the row was last written in: a row of another epoch reads as zeros, so the table
// is never cleared between planes, streams or calls), behind a direct-mapped write-back cache of DEC16_SLOTS rows in LDS
// (a plane uses a few thousand contexts, a few dozen of them for most of its events).  A row lives one counter per lane
// (lanes 0 .. 14): get_k and the update's minimum are DPP reductions over one row of sixteen lanes, everything else about
// a pixel is scalar code as in k_decode8.  Gray: u16 pixels straight out; RGB: Y / Co / Cg as int32 planes + k_ycocg16_to_rgb.
// ------------------------------------------------------------------------------------------

constexpr uint32_t DEC16_SLOTS = 512;                 // cached rows: 32 KB of LDS
constexpr uint32_t DEC16_ROW = 16;                    // words per row (15 counters, epoch)
constexpr uint32_t DEC16_CONTEXTS = 2u * 65535u + 1u;  // MAX_CONTEXT + 1 (traits.rs:38)

// minimum over lanes 0 .. 15 (one DPP row), left in lane 15, returned wave-uniform
__device__ __forceinline__ uint32_t row16_min(uint32_t v) {
    v = min(v, (uint32_t)__builtin_amdgcn_update_dpp((int)0xFFFFFFFFu, (int)v, 0x111, 0xF, 0xF, false));  // row_shr:1
    v = min(v, (uint32_t)__builtin_amdgcn_update_dpp((int)0xFFFFFFFFu, (int)v, 0x112, 0xF, 0xF, false));  // row_shr:2
    v = min(v, (uint32_t)__builtin_amdgcn_update_dpp((int)0xFFFFFFFFu, (int)v, 0x114, 0xF, 0xF, false));  // row_shr:4
    v = min(v, (uint32_t)__builtin_amdgcn_update_dpp((int)0xFFFFFFFFu, (int)v, 0x118, 0xF, 0xF, false));  // row_shr:8
    return (uint32_t)__builtin_amdgcn_readlane((int)v, 15);
}

// G: DecUniform or DecMixed as for k_decode8; the estimator table is the row's (blockIdx.x) either way.
template <typename G>
__global__ __launch_bounds__(64) void k_decode16(const uint8_t *__restrict__ streams, const uint64_t *__restrict__ offsets,
                                                 const uint64_t *__restrict__ lens, G geo, uint16_t *__restrict__ pixels,
                                                 int32_t *__restrict__ planes, uint32_t *__restrict__ gtable, uint32_t epoch0,
                                                 int *__restrict__ status) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const DecView v = dec_view(geo, blockIdx.x);
    const uint32_t W = v.W, H = v.H, color = v.color;
    uint32_t *crow = reinterpret_cast<uint32_t *>(smem);                       // [DEC16_SLOTS][DEC16_ROW] cached rows
    uint32_t *ctag = crow + DEC16_SLOTS * DEC16_ROW;                            // [DEC16_SLOTS] context held (or ~0)
    int32_t *rows = reinterpret_cast<int32_t *>(ctag + DEC16_SLOTS);
    const uint32_t rstride = decode8_row_stride(W);
    const uint32_t img = v.img, lane = lane_id();
    const uint8_t *s = streams + offsets[img];
    const uint64_t slen = lens[img];
    const uint64_t npix = (uint64_t)W * H;
    const uint32_t nplanes = color ? 3u : 1u;
    uint32_t *table = gtable + (uint64_t)blockIdx.x * DEC16_CONTEXTS * DEC16_ROW;
    int rc = FELICS_OK;
    if (slen < FELICS_HEADER_BYTES) {
        rc = FELICS_E_IO;
    } else {
        const uint32_t w = ((uint32_t)s[6] << 24) | ((uint32_t)s[7] << 16) | ((uint32_t)s[8] << 8) | s[9];
        const uint32_t h = ((uint32_t)s[10] << 24) | ((uint32_t)s[11] << 16) | ((uint32_t)s[12] << 8) | s[13];
        if (s[0] != 'F' || s[1] != 'L' || s[2] != 'C' || s[3] != 'S') rc = FELICS_E_INVALID_SIGNATURE;
        else if (s[4] > 1) rc = FELICS_E_INVALID_COLOR_TYPE;
        else if (s[5] > 1) rc = FELICS_E_INVALID_PIXEL_DEPTH;
        else if (s[4] != color || s[5] != 1 || w != W || h != H) rc = FELICS_E_INVALID_DIMENSIONS;
    }
    rc = unii(rc);
    if (rc != FELICS_OK) {
        if (lane == 0) status[img] = rc;
        return;
    }
    ScalarBits br;
    br.init(s + FELICS_HEADER_BYTES, slen - FELICS_HEADER_BYTES);
    for (uint32_t c = 0; c < nplanes && rc == FELICS_OK; c++) {
        const int32_t p0 = (int32_t)br.get(32), p1 = (int32_t)br.get(32);  // compression.rs:166-167
        if (br.failed()) {
            rc = FELICS_E_IO;
            break;
        }
        if (npix == 0) continue;
        const uint32_t epoch = epoch0 + c;  // KEstimator::new: rows of other epochs read as zeros
        for (uint32_t i = lane; i < DEC16_SLOTS; i += 64) ctag[i] = 0xFFFFFFFFu;  // (nothing to write back: the last plane's rows are dead)
        __builtin_amdgcn_wave_barrier();
        const bool rgb = dec_rgb(geo, v, planes);
        int32_t *outp = rgb ? dec_plane(geo, planes, v, nplanes, c, npix) : nullptr;
        uint16_t *outg = rgb ? nullptr : dec_frame(geo, pixels, v, npix);
        uint64_t opitch = 0, orow = 0;  // DecPitched, in samples (strides are even at depth 16)
        if constexpr (std::is_same<G, DecPitched>::value) opitch = (uint64_t)geo.views[blockIdx.x].row_stride / 2u;
        const int lo_ok = (color && c > 0) ? -65535 : 0, hi_ok = 65535;  // Y 0..65535, Co / Cg -65535..65535
        uint32_t x = 0, y = 0;
        int32_t *cur = rows, *prev = rows + rstride;
        int upv = 0;   // VECTOR: prev[xb + lane] for the 64-sample block xb the walk stands in
        int rowv = 0;  // VECTOR: the samples of this block decoded so far
        int left = 0, left2 = 0;
        int first_col2 = 0;
        for (uint64_t i = 0; i < npix; i++) {
            const uint32_t xl = x & 63u;
            if (xl == 0) {
                if (y > 0) upv = (int)prev[x + lane];
                if (x == 0 && y > 0) first_col2 = y >= 2 ? unii((int)cur[0]) : (W > 1 ? __builtin_amdgcn_readlane(upv, 1) : 0);
            }
            int pv;
            if (i < 2) {
                pv = i == 0 ? p0 : p1;
            } else {
                const int above = __builtin_amdgcn_readlane(upv, (int)xl);
                const bool row0 = y == 0, col0 = x == 0 && !row0;
                const int v1 = col0 ? above : left;
                const int v2 = col0 ? first_col2 : (row0 ? left2 : above);
                const int hi = max(v1, v2), lo = min(v1, v2);
                const uint32_t ctx = (uint32_t)(hi - lo);  // <= 131 070 because every stored sample is in range
                br.refill();  // >= 33 bits: an in-range code has at most 18, the two flags of the other kind 2
                if (br.take(1)) {  // in range: phased-in code of p - L (phase_in_coding.rs:86-112)
                    const uint32_t n = ctx + 1;
                    const uint32_t m = 31u - (uint32_t)__builtin_clz(n);
                    const uint32_t right_p = (2u << m) - n, left_p = n - (1u << m);
                    uint32_t r = br.take(m);
                    const uint32_t longer = r >= right_p ? 1u : 0u;
                    const uint32_t r2 = (r - right_p) * 2u + right_p + br.take(longer);
                    r = longer ? r2 : r;
                    uint32_t rot = r + left_p;
                    rot = rot >= n ? rot - n : rot;
                    pv = lo + (int)rot;
                } else {
                    const bool above_flag = br.take(1) != 0;
                    // the context's row: lane k < 15 holds counter k
                    const uint32_t slot = ctx & (DEC16_SLOTS - 1u);
                    const uint32_t held = uni(ctag[slot]);
                    uint32_t S;
                    if (held == ctx) {
                        S = crow[slot * DEC16_ROW + (lane & 15u)];
                    } else {
                        if (held != 0xFFFFFFFFu && lane < DEC16_ROW)  // write the row this slot held back (its epoch word with it)
                            table[(uint64_t)held * DEC16_ROW + lane] = crow[slot * DEC16_ROW + lane];
                        // (read from L2, not from this CU's L1: the row may be one this wave wrote back a while ago; that store
                        // has been acknowledged by now -- every load's wait covers the stores before it)
                        uint32_t g = lane < DEC16_ROW ? __hip_atomic_load(&table[(uint64_t)ctx * DEC16_ROW + lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
                        const uint32_t row_epoch = (uint32_t)__builtin_amdgcn_readlane((int)g, 15);
                        g = row_epoch == epoch ? g : 0u;  // a row of another plane / call: fresh
                        S = (uint32_t)__shfl((int)g, (int)(lane & 15u));  // every row of sixteen lanes holds the counters
                        if (lane == 0) ctag[slot] = ctx;
                    }
                    // get_k: smallest counter, ties to the largest k (parameter_selection.rs:71-85)
                    const uint32_t l15 = lane & 15u;
                    const uint32_t key = l15 < 15u ? (S << 4) | (15u - l15) : 0xFFFFFFFFu;
                    const uint32_t k = 15u - (row16_min(key) & 15u);
                    const uint64_t q = br.unary0();
                    const uint64_t e64 = (q << k) + br.get(k);
                    if (e64 > 262144u) {  // no sample of a 16-bit plane is that far from its neighbours
                        rc = e64 > 0xFFFFFFFFull ? FELICS_E_VALUE_OVERFLOW : FELICS_E_INVALID_VALUE;
                        break;
                    }
                    const uint32_t e = (uint32_t)e64;
                    uint32_t S2 = S + (e >> l15) + 1u + l15;                       // update (rice_coding.rs:56-58 lengths)
                    const uint32_t mn = row16_min(l15 < 15u ? S2 : 0xFFFFFFFFu);
                    S2 = mn > 1024u ? S2 >> 1 : S2;                                // x /= 2 on every counter
                    if (lane < DEC16_ROW) crow[slot * DEC16_ROW + lane] = lane < 15u ? S2 : epoch;
                    pv = above_flag ? hi + (int)e + 1 : lo - (int)e - 1;
                }
            }
            if (pv < lo_ok || pv > hi_ok) {
                rc = FELICS_E_INVALID_VALUE;
                break;
            }
            rowv = lane == xl ? pv : rowv;
            left2 = left;
            left = pv;
            const bool row_end = x + 1 == W;
            if (xl == 63u || row_end) {
                const uint32_t xb = x & ~63u;
                if (xb + lane <= x) {
                    cur[xb + lane] = rowv;
                    if constexpr (std::is_same<G, DecPitched>::value) {
                        if (outg)
                            outg[orow + xb + lane] = (uint16_t)rowv;  // (xb + lane <= x < W)
                        else
                            outp[(uint64_t)y * W + xb + lane] = rowv;
                    } else if (outg)
                        outg[(uint64_t)y * W + xb + lane] = (uint16_t)rowv;
                    else
                        outp[(uint64_t)y * W + xb + lane] = rowv;
                }
            }
            if (row_end) {
                if (br.failed()) {
                    rc = FELICS_E_IO;
                    break;
                }
                __builtin_amdgcn_wave_barrier();
                x = 0;
                y++;
                if constexpr (std::is_same<G, DecPitched>::value) orow += opitch;
                int32_t *t = cur;
                cur = prev;
                prev = t;
            } else {
                x++;
            }
        }
    }
    if (br.failed()) rc = FELICS_E_IO;
    if (lane == 0) status[img] = rc;
}

// ycocg_to_rgb (color_transform.rs:20-26) on the decoded 16-bit planes, range-checked like try_into::<u16>()
template <typename G>
__global__ __launch_bounds__(256) void k_ycocg16_to_rgb(const int32_t *__restrict__ planes, uint16_t *__restrict__ pixels,
                                                        G geo, int *__restrict__ status) {
    ConvView<int32_t, uint16_t> cv;
    if (!conv_view(geo, planes, pixels, cv)) return;
    const uint32_t img = cv.img, npix = cv.npix;
    if (status[img] != FELICS_OK) return;
    const int32_t *pl = cv.pl;
    uint16_t *dst = cv.dst;
    bool bad = false;
    if constexpr (std::is_same<G, ConvStrided>::value) {
        // (as k_ycocg8_to_rgb: one two-byte store per sample; addresses and strides are even)
        const ViewRow vr = geo.views[blockIdx.y];
        const uint32_t W = geo.rows[blockIdx.y].W;
        uint8_t *base = reinterpret_cast<uint8_t *>(const_cast<void *>(vr.data));
        for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < npix; i += gridDim.x * blockDim.x) {
            const int yv = pl[i], co = pl[(uint64_t)npix + i], cg = pl[2ull * npix + i];
            const int t = yv - cg / 2;
            const int g = cg + t, b = t - co / 2, r = b + co;
            if ((r | g | b) < 0 || r > 65535 || g > 65535 || b > 65535) bad = true;
            const uint32_t y = i / W, x = i - y * W;
            uint8_t *p = base + (int64_t)y * vr.row_stride + (int64_t)x * vr.pixel_stride;
            *reinterpret_cast<uint16_t *>(p) = (uint16_t)r;
            *reinterpret_cast<uint16_t *>(p + vr.channel_stride) = (uint16_t)g;
            *reinterpret_cast<uint16_t *>(p + 2 * vr.channel_stride) = (uint16_t)b;
        }
    } else {
        for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < npix; i += gridDim.x * blockDim.x) {
            const int yv = pl[i], co = pl[(uint64_t)npix + i], cg = pl[2ull * npix + i];
            const int t = yv - cg / 2;  // `/` truncates toward zero like Rust's
            const int g = cg + t, b = t - co / 2, r = b + co;
            if ((r | g | b) < 0 || r > 65535 || g > 65535 || b > 65535) bad = true;
            dst[(uint64_t)i * 3] = (uint16_t)r;
            dst[(uint64_t)i * 3 + 1] = (uint16_t)g;
            dst[(uint64_t)i * 3 + 2] = (uint16_t)b;
        }
    }
    if (bad) atomicCAS(&status[img], FELICS_OK, FELICS_E_INVALID_VALUE);
}

// ------------------------------------------------------------------------------------------
// 16-bit streams through a restart index (format version 2: felics.h "Restart index: 16-bit streams", felics_index.h): one wave per
// (stream, plane, segment), the walk of decode8_from_checkpoint with k_decode16's per-pixel path.  Host model:
// felics_decompress_indexed16, with the same checks in the same order.  The sink is decode8_from_checkpoint's:
//   stop(pend), store(col, y, at, v).
// ------------------------------------------------------------------------------------------
namespace {

// Segment (c, j) of stream s / index idx (idx_len bytes, 64-byte aligned), decoded by the calling wave into `sink`; `smem` is the
// kernel's dynamic LDS (decode16_lds_bytes(W)), `table` the wave's own dense estimator table (DEC16_CONTEXTS rows; rows of another
// epoch read as zeros).  Returns the segment's status, wave-uniform; *loaded = the state rows it copied.  header_only: the checks of
// the two headers and nothing else (c and j are not looked at, no table row is touched).
template <typename Sink>
__device__ __forceinline__ int decode16_from_checkpoint(uint8_t *smem, const uint8_t *s, uint64_t slen, const uint8_t *idx, uint64_t idx_len,
                                                        const DecUniform &geo, uint32_t segment_pixels, uint32_t K, uint32_t c, uint32_t j,
                                                        bool header_only, uint32_t *table, uint32_t epoch, const Sink &sink, uint32_t *loaded) {
    const uint32_t W = geo.W, H = geo.H, color = geo.color;
    uint32_t *crow = reinterpret_cast<uint32_t *>(smem);  // [DEC16_SLOTS][DEC16_ROW] cached rows
    uint32_t *ctag = crow + DEC16_SLOTS * DEC16_ROW;      // [DEC16_SLOTS] context held (or ~0)
    int32_t *rows = reinterpret_cast<int32_t *>(ctag + DEC16_SLOTS);
    const uint32_t rstride = decode8_row_stride(W);
    const uint32_t lane = lane_id();
    const uint64_t npix = (uint64_t)W * H;
    *loaded = 0;
    // 1. the checks: the stream's header must be the one announced, the index header must fit it, the launch and the index's length;
    //    then this segment's directory entry
    Index16Layout L;
    uint64_t start = 0, end = 0, rows_off = 0;
    uint32_t n_rows = 0;
    int rc = FELICS_OK;
    if (slen < FELICS_HEADER_BYTES) {
        rc = FELICS_E_IO;
    } else {
        const uint32_t w = ((uint32_t)s[6] << 24) | ((uint32_t)s[7] << 16) | ((uint32_t)s[8] << 8) | s[9];
        const uint32_t h = ((uint32_t)s[10] << 24) | ((uint32_t)s[11] << 16) | ((uint32_t)s[12] << 8) | s[13];
        if (s[0] != 'F' || s[1] != 'L' || s[2] != 'C' || s[3] != 'S') rc = FELICS_E_INVALID_SIGNATURE;
        else if (s[4] > 1) rc = FELICS_E_INVALID_COLOR_TYPE;
        else if (s[5] > 1) rc = FELICS_E_INVALID_PIXEL_DEPTH;
        else if (s[4] != color || s[5] != 1 || w != W || h != H) rc = FELICS_E_INVALID_DIMENSIONS;
        else if (idx_len < INDEX_HEADER_BYTES || index16_header_check(idx, color, W, H, slen, idx_len, L) != FELICS_OK ||
                 idx_rd32(idx + IDX_SEGPIX) != segment_pixels || L.K != K)
            rc = FELICS_E_INVALID_INDEX;
        else if (!header_only) rc = index16_segment_bounds(idx, L, c, j, slen, idx_len, start, end, rows_off, n_rows);
    }
    rc = unii(rc);
    if (rc != FELICS_OK || header_only) return rc;
    start = ((uint64_t)uni((uint32_t)(start >> 32)) << 32) | uni((uint32_t)start);
    end = ((uint64_t)uni((uint32_t)(end >> 32)) << 32) | uni((uint32_t)end);
    rows_off = ((uint64_t)uni((uint32_t)(rows_off >> 32)) << 32) | uni((uint32_t)rows_off);
    n_rows = uni(n_rows);
    const uint64_t p0 = (uint64_t)j * segment_pixels, pend = min(npix, p0 + segment_pixels);  // this segment's pixels
    const uint64_t stop = sink.stop(pend);
    // 2. the estimator table: the checkpoint's rows into the wave's table, four rows per iteration at sixteen lanes per row.  A row
    //    is one coalesced 64-byte load; its last word is the context, checked (range, strictly ascending) before it indexes anything
    //    and replaced by the epoch in the store.  [rows_off, rows_off + 64 n_rows) lies inside the index: index16_segment_bounds.
    //    The wave reads these rows back later with k_decode16's agent-scope loads: the situation of that kernel's write-back path
    //    (a row this wave stored a while ago, read from L2; every load's wait covers the stores before it), and the same argument.
    {
        const uint32_t *src = reinterpret_cast<const uint32_t *>(idx + rows_off);
        const uint32_t limit = index16_contexts(color, c), l15 = lane & 15u, grp = lane >> 4;
        int64_t carry = -1;  // the context of the row in front of this iteration's first
        for (uint32_t r0 = 0; r0 < n_rows; r0 += 4) {
            const uint32_t r = r0 + grp;
            const bool have = r < n_rows;
            const uint32_t wv = have ? src[(uint64_t)r * DEC16_ROW + l15] : 0u;
            const uint32_t ctx = (uint32_t)__shfl((int)wv, (int)((lane & 48u) | 15u));
            const uint32_t before = (uint32_t)__shfl((int)wv, (int)(((lane & 48u) - 16u + 15u) & 63u));  // (group 0: not used)
            const int64_t prev = grp ? (int64_t)before : carry;
            const bool ok = ctx < limit && (int64_t)ctx > prev;
            if (__ballot(have && !ok) != 0) return FELICS_E_INVALID_INDEX;
            if (have) table[(uint64_t)ctx * DEC16_ROW + l15] = l15 == 15u ? epoch : wv;
            carry = (int64_t)(uint32_t)__builtin_amdgcn_readlane((int)ctx, 63);  // (a last iteration's missing rows: it is the last)
        }
        for (uint32_t i = lane; i < DEC16_SLOTS; i += 64) ctag[i] = 0xFFFFFFFFu;  // the LDS cache starts empty
        *loaded = n_rows;
    }
    // 3. the window into the two LDS rows (decode8_from_checkpoint's placement): with (x0, y0) = p0's place, window sample t is pixel
    //    p0 - 2 W + t: row y0 from t = 2 W - x0 on (cur), row y0 - 1 from t = W - x0 on (prev), and of row y0 - 2 only (0, y0 - 2), if
    //    x0 = 0 (the first-column rule: what cur[0] holds)
    uint32_t x = 0, y = 0;
    int32_t *cur = rows, *prev = rows + rstride;
    const int lo_ok = (color && c > 0) ? -65535 : 0, hi_ok = 65535;  // Y 0..65535, Co / Cg -65535..65535
    if (K) {
        x = (uint32_t)(p0 % W);
        y = (uint32_t)(p0 / W);
        const uint8_t *win = idx + L.win_base + ((uint64_t)c * K + j) * L.win_bytes;  // (16-byte aligned, inside the index: total >= rows_base)
        bool bad = false;
        for (uint64_t t = lane; t < 2ull * W; t += 64) {
            if (p0 + t < 2ull * W) continue;  // in front of the plane: zeros, never looked at
            const int v = color ? reinterpret_cast<const int32_t *>(win)[t] : (int)reinterpret_cast<const uint16_t *>(win)[t];
            bad |= v < lo_ok || v > hi_ok;
            if (t >= 2ull * W - x) cur[t - (2ull * W - x)] = v;
            else if (t >= (uint64_t)W - x) prev[t - ((uint64_t)W - x)] = v;
            else if (t == 0 && x == 0) cur[0] = v;
        }
        if (__ballot(bad) != 0) return FELICS_E_INVALID_INDEX;
    }
    __builtin_amdgcn_wave_barrier();
    // 4. the bit reader at the checkpoint's position (<= 8 slen: the bounds check); every fetch is bounded by the stream's length
    ScalarBits br;
    br.init_at(s, slen, start);
    int32_t raw0 = 0, raw1 = 0;
    if (j == 0) {  // the plane's two raw samples (compression.rs:166-167) stand in front of its first segment only
        raw0 = (int32_t)br.get(32);
        raw1 = (int32_t)br.get(32);
        if (br.failed()) rc = FELICS_E_IO;
    }
    // 5. the walk: k_decode16's pixel, decode8_from_checkpoint's block handling
    if (rc == FELICS_OK && stop > p0) {
        const uint32_t xl0 = x & 63u;
        int upv = 0;   // VECTOR: prev[xb + lane] for the 64-sample block xb the walk stands in
        int rowv = 0;  // VECTOR: the samples of this block decoded so far
        if (xl0) {     // a start inside a block: the block's samples in front of it are the window's
            if (y > 0) upv = (int)prev[(x & ~63u) + lane];
            rowv = (int)cur[(x & ~63u) + lane];
        }
        int left = x >= 1 ? unii((int)cur[x - 1]) : 0, left2 = x >= 2 ? unii((int)cur[x - 2]) : 0;
        int first_col2 = 0;
        for (uint64_t i = p0; i < stop; i++) {
            const uint32_t xl = x & 63u;
            if (xl == 0) {
                if (y > 0) upv = (int)prev[x + lane];
                if (x == 0 && y > 0) first_col2 = y >= 2 ? unii((int)cur[0]) : (W > 1 ? __builtin_amdgcn_readlane(upv, 1) : 0);
            }
            int pv;
            if (i < 2) {
                pv = i == 0 ? raw0 : raw1;
            } else {
                const int above = __builtin_amdgcn_readlane(upv, (int)xl);
                const bool row0 = y == 0, col0 = x == 0 && !row0;
                const int v1 = col0 ? above : left;
                const int v2 = col0 ? first_col2 : (row0 ? left2 : above);
                const int hi = max(v1, v2), lo = min(v1, v2);
                const uint32_t ctx = (uint32_t)(hi - lo);  // <= 131 070 because every stored sample is in range
                br.refill();
                if (br.take(1)) {  // in range: phased-in code of p - L (phase_in_coding.rs:86-112)
                    const uint32_t n = ctx + 1;
                    const uint32_t m = 31u - (uint32_t)__builtin_clz(n);
                    const uint32_t right_p = (2u << m) - n, left_p = n - (1u << m);
                    uint32_t r = br.take(m);
                    const uint32_t longer = r >= right_p ? 1u : 0u;
                    const uint32_t r2 = (r - right_p) * 2u + right_p + br.take(longer);
                    r = longer ? r2 : r;
                    uint32_t rot = r + left_p;
                    rot = rot >= n ? rot - n : rot;
                    pv = lo + (int)rot;
                } else {
                    const bool above_flag = br.take(1) != 0;
                    const uint32_t slot = ctx & (DEC16_SLOTS - 1u);
                    const uint32_t held = uni(ctag[slot]);
                    uint32_t S;
                    if (held == ctx) {
                        S = crow[slot * DEC16_ROW + (lane & 15u)];
                    } else {
                        if (held != 0xFFFFFFFFu && lane < DEC16_ROW)  // write the row this slot held back (its epoch word with it)
                            table[(uint64_t)held * DEC16_ROW + lane] = crow[slot * DEC16_ROW + lane];
                        uint32_t g = lane < DEC16_ROW ? __hip_atomic_load(&table[(uint64_t)ctx * DEC16_ROW + lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
                        const uint32_t row_epoch = (uint32_t)__builtin_amdgcn_readlane((int)g, 15);
                        g = row_epoch == epoch ? g : 0u;  // neither loaded nor written by this segment: fresh
                        S = (uint32_t)__shfl((int)g, (int)(lane & 15u));
                        if (lane == 0) ctag[slot] = ctx;
                    }
                    const uint32_t l15 = lane & 15u;
                    const uint32_t key = l15 < 15u ? (S << 4) | (15u - l15) : 0xFFFFFFFFu;
                    const uint32_t k = 15u - (row16_min(key) & 15u);
                    const uint64_t q = br.unary0();
                    const uint64_t e64 = (q << k) + br.get(k);
                    if (e64 > 262144u) {  // no sample of a 16-bit plane is that far from its neighbours
                        rc = e64 > 0xFFFFFFFFull ? FELICS_E_VALUE_OVERFLOW : FELICS_E_INVALID_VALUE;
                        break;
                    }
                    const uint32_t e = (uint32_t)e64;
                    uint32_t S2 = S + (e >> l15) + 1u + l15;
                    const uint32_t mn = row16_min(l15 < 15u ? S2 : 0xFFFFFFFFu);
                    S2 = mn > 1024u ? S2 >> 1 : S2;
                    if (lane < DEC16_ROW) crow[slot * DEC16_ROW + lane] = lane < 15u ? S2 : epoch;
                    pv = above_flag ? hi + (int)e + 1 : lo - (int)e - 1;
                }
            }
            if (pv < lo_ok || pv > hi_ok) {
                rc = FELICS_E_INVALID_VALUE;
                break;
            }
            rowv = lane == xl ? pv : rowv;
            left2 = left;
            left = pv;
            const bool row_end = x + 1 == W;
            if (xl == 63u || row_end || i + 1 == stop) {  // a block of the row is complete, or the walk is
                const uint32_t xb = x & ~63u;
                if (xb + lane <= x) {
                    cur[xb + lane] = rowv;  // (lanes in front of a mid-block start store back what they loaded)
                    const uint64_t at = (uint64_t)y * W + xb + lane;  // < stop: xb + lane <= x
                    if (at >= p0) sink.store(xb + lane, y, at, rowv);  // the samples in front of p0 are the segment's before this one
                }
            }
            if (row_end) {
                if (br.failed()) {
                    rc = FELICS_E_IO;
                    break;
                }
                __builtin_amdgcn_wave_barrier();
                x = 0;
                y++;
                int32_t *t = cur;
                cur = prev;
                prev = t;
            } else {
                x++;
            }
        }
    }
    // 6. the end check: exactly on the next checkpoint
    if (br.failed()) rc = FELICS_E_IO;  // (whatever else stopped the decoding: it was decoding padding)
    else if (rc == FELICS_OK && stop == pend && br.pos(s) != end) rc = FELICS_E_INVALID_INDEX;
    return rc;
}

}  // namespace

// One wave per SEGMENT of a plane of a 16-bit stream (felics_decompress_batch_device_indexed16), a pass of consecutive items at a
// time: block b is item item0 + b = (img, c, j) = (item / (C Keff), item / Keff % C, item % Keff), Keff = max(K, 1), and owns table b
// of the pass's tables.  seg_status[item] = FELICS_OK or the code; k_seg_status picks a stream's first.  rows_loaded: += the state
// rows the wave copied.
__global__ __launch_bounds__(64) void k_decode16_seg(const uint8_t *__restrict__ streams, const uint64_t *__restrict__ offsets,
                                                     const uint64_t *__restrict__ lens, const uint8_t *__restrict__ index,
                                                     const uint64_t *__restrict__ idx_offsets, const uint64_t *__restrict__ idx_lens, DecUniform geo,
                                                     uint32_t segment_pixels, uint32_t K, uint32_t item0, uint16_t *__restrict__ pixels,
                                                     int32_t *__restrict__ planes, uint32_t *__restrict__ gtable, uint32_t epoch,
                                                     int *__restrict__ seg_status, unsigned long long *__restrict__ rows_loaded) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const uint32_t nplanes = geo.color ? 3u : 1u, keff = max(K, 1u);
    const uint32_t item = item0 + blockIdx.x;
    const uint32_t img = item / (nplanes * keff), c = item / keff % nplanes, j = item % keff;
    const uint64_t npix = (uint64_t)geo.W * geo.H;
    const SegmentSink<uint16_t, int32_t> sink{geo.color ? nullptr : pixels + (uint64_t)img * npix, geo.color ? planes + ((uint64_t)img * nplanes + c) * npix : nullptr};
    uint32_t *table = gtable + (uint64_t)blockIdx.x * DEC16_CONTEXTS * DEC16_ROW;
    uint32_t loaded = 0;
    const int rc = decode16_from_checkpoint(smem, streams + offsets[img], lens[img], index + idx_offsets[img], idx_lens[img], geo, segment_pixels, K,
                                            c, j, false, table, epoch, sink, &loaded);
    if (lane_id() == 0) {
        seg_status[item] = rc;
        if (loaded) atomicAdd(rows_loaded, (unsigned long long)loaded);
    }
}

// One wave per WORK ITEM = (region, plane, needed segment) of felics_decompress_regions_device_indexed16 (felics.h "Restart index:
// regions of 16-bit streams"; host model: felics_decompress_region_indexed16), a pass of consecutive items at a time: block b is item
// item0 + b and owns table b of the pass's tables, exactly as in k_decode16_seg.  The host names needed segments only (j < K,
// p0 < stop); an item with seg = REGION_HEADER_ONLY ends after the header checks.  item_status[item] = FELICS_OK or the code;
// k_seg_status picks a region's first.  Gray crops lie at pixels + out_off (bytes, even), RGB planes at planes + plane_off.
__global__ __launch_bounds__(64) void k_decode16_region(const uint8_t *__restrict__ streams, const uint64_t *__restrict__ offsets,
                                                        const uint64_t *__restrict__ lens, const uint8_t *__restrict__ index,
                                                        const uint64_t *__restrict__ idx_offsets, const uint64_t *__restrict__ idx_lens,
                                                        DecUniform geo, uint32_t segment_pixels, uint32_t K, const RegionRow *__restrict__ regions,
                                                        const RegionItem *__restrict__ items, uint32_t item0, uint8_t *__restrict__ pixels,
                                                        int32_t *__restrict__ planes, uint32_t *__restrict__ gtable, uint32_t epoch,
                                                        int *__restrict__ item_status, unsigned long long *__restrict__ rows_loaded) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const RegionItem item = items[item0 + blockIdx.x];
    const RegionRow reg = regions[item.region];
    const uint32_t img = reg.stream, c = item.plane;
    const RegionSink<uint16_t, int32_t> sink{reg, geo.W, geo.color ? nullptr : reinterpret_cast<uint16_t *>(pixels + reg.out_off),
                                              geo.color ? planes + reg.plane_off + (uint64_t)c * reg.w * reg.h : nullptr};
    uint32_t *table = gtable + (uint64_t)blockIdx.x * DEC16_CONTEXTS * DEC16_ROW;
    uint32_t loaded = 0;
    const int rc = decode16_from_checkpoint(smem, streams + offsets[img], lens[img], index + idx_offsets[img], idx_lens[img], geo, segment_pixels, K,
                                            c, item.seg, item.seg == REGION_HEADER_ONLY, table, epoch, sink, &loaded);
    if (lane_id() == 0) {
        item_status[item0 + blockIdx.x] = rc;
        if (loaded) atomicAdd(rows_loaded, (unsigned long long)loaded);
    }
}

// One wave per WORK ITEM = (row, plane, segment) of felics_decompress_views_device_indexed16 (felics_kernels.h; host model:
// felics_decompress_indexed16_view): k_decode8_seg_views for version-2 indexes.  The tables are that kernel's own (IndexViewRow,
// IndexViewItem: every field fits; plane_off counts int32 samples); the one thing a version-2 walk needs beside them, the index's
// length, is read from idx_lens[row.stream], which the call has on the device anyway.  Item and row are wave-uniform (blockIdx.x:
// scalar loads); geometry, segment_pixels and K are the row's.  Block b of a launch works on items[b] with table b of the launch's
// tables and the launch's epoch, as in k_decode16_seg; item_status[b] = FELICS_OK or the code (k_seg_status picks a row's first);
// rows_loaded: += the state rows the wave copied.
__global__ __launch_bounds__(64) void k_decode16_seg_views(const uint8_t *__restrict__ streams, const uint64_t *__restrict__ offsets,
                                                           const uint64_t *__restrict__ lens, const uint8_t *__restrict__ index,
                                                           const uint64_t *__restrict__ idx_lens, const IndexViewRow *__restrict__ rows,
                                                           const IndexViewItem *__restrict__ items, int32_t *__restrict__ planes,
                                                           uint32_t *__restrict__ gtable, uint32_t epoch, int *__restrict__ item_status,
                                                           unsigned long long *__restrict__ rows_loaded) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const IndexViewItem item = items[blockIdx.x];
    const IndexViewRow r = rows[item.row];
    const DecUniform geo{r.W, r.H, r.color};
    const uint32_t c = item.plane;
    const ViewSink<uint16_t, int32_t> sink{r.color ? nullptr : reinterpret_cast<uint8_t *>(const_cast<void *>(r.view.data)), r.view.row_stride,
                                           r.view.pixel_stride, r.color ? planes + r.plane_off + (uint64_t)c * r.W * r.H : nullptr};
    uint32_t *table = gtable + (uint64_t)blockIdx.x * DEC16_CONTEXTS * DEC16_ROW;
    uint32_t loaded = 0;
    const int rc = decode16_from_checkpoint(smem, streams + offsets[r.stream], lens[r.stream], index + r.index_off, idx_lens[r.stream], geo,
                                            r.segment_pixels, r.K, c, item.seg, false, table, epoch, sink, &loaded);
    if (lane_id() == 0) {
        item_status[blockIdx.x] = rc;
        if (loaded) atomicAdd(rows_loaded, (unsigned long long)loaded);
    }
}

// One wave per WORK ITEM = (region, plane, needed segment) of felics_decompress_region_views_device_indexed16 (host model:
// felics_decompress_region_indexed16_view): k_decode8_region_views for version-2 indexes, on that kernel's tables (plane_off counts
// int32 samples); the index's length is idx_lens[region.stream].  Block b of a launch works on items[b] with table b of the launch's
// tables and the launch's epoch, as in k_decode16_seg_views; item_status[b] = FELICS_OK or the code (k_seg_status picks a region's
// first); rows_loaded: += the state rows the wave copied.
__global__ __launch_bounds__(64) void k_decode16_region_views(const uint8_t *__restrict__ streams, const uint64_t *__restrict__ offsets,
                                                              const uint64_t *__restrict__ lens, const uint8_t *__restrict__ index,
                                                              const uint64_t *__restrict__ idx_lens, const RegionViewStream *__restrict__ srows,
                                                              const RegionRow *__restrict__ regions, const ViewRow *__restrict__ views,
                                                              const RegionItem *__restrict__ items, int32_t *__restrict__ planes,
                                                              uint32_t *__restrict__ gtable, uint32_t epoch, int *__restrict__ item_status,
                                                              unsigned long long *__restrict__ rows_loaded) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const RegionItem item = items[blockIdx.x];
    const RegionRow reg = regions[item.region];
    const ViewRow view = views[item.region];
    const RegionViewStream r = srows[reg.stream];
    const DecUniform geo{r.W, r.H, r.color};
    const uint32_t c = item.plane;
    const auto sink = RegionViewSink<uint16_t, int32_t>::make(reg, r.W, r.color, c, view, planes);
    uint32_t *table = gtable + (uint64_t)blockIdx.x * DEC16_CONTEXTS * DEC16_ROW;
    uint32_t loaded = 0;
    const int rc = decode16_from_checkpoint(smem, streams + offsets[reg.stream], lens[reg.stream], index + r.index_off, idx_lens[reg.stream], geo,
                                            r.segment_pixels, r.K, c, item.seg, false, table, epoch, sink, &loaded);
    if (lane_id() == 0) {
        item_status[blockIdx.x] = rc;
        if (loaded) atomicAdd(rows_loaded, (unsigned long long)loaded);
    }
}

// ------------------------------------------------------------------------------------------
// 16-bit streams, sixty-four of one shape per wave, LANE = stream: the walk of k_decode8_lanes with the arithmetic of k_decode16.
//
// (x, y) is wave-uniform, the bit reader is a LaneReader, the row above is read back from the lane's own output four samples at a
// time and a load ahead.  Per pixel every lane works out the in-range code off the top 32 bits of its window (an in-range code has
// at most 18 bits); the lanes whose pixel is out of range then take the estimator path together: the context's row (fifteen 32-bit
// counters in named registers -- counter 0 can gain 131 071 per event while the smallest gains one, so several million accumulate
// between two halvings; `(S << 4) | rank` still fits 32 bits: below 2^28), get_k with ties to the largest k, the Rice code off the
// same 32 bits when its unary part, the zero and the k bits lie inside them and through LaneReader::unary0 (bounded by the stream's
// length) when they do not -- a valid stream holds unary runs of tens of thousands of bits --, the update, the halving.
//
// The estimator table is the lane's own, sized by what the stream can use (felics_lanetable.h: rows = 2 x (pixels - 2) rounded up to
// a power of two, hashed and open-addressed; from 65 536 rows on the dense table of k_decode16), one per plane, in HBM: rows of 64
// bytes read and written with 16-byte accesses, the tag word = (epoch << 17) | context.  A row of another epoch is empty, so nothing
// is zeroed per call.  A search is bounded by the row count; a table found full is FELICS_E_IO for that lane (the sizing rule does
// not let it happen), not a loop.
//
// Visibility: PLAIN loads and stores, as k_decode8_lanes has them, not the agent-scope loads of k_decode16.  A row is written and
// read by one lane of one wave only, in program order and through that CU's write-through L1 -- the same path by which the lane
// reads the row above back from its own output --, so there is no other CU's store to miss within a launch; rows left by earlier
// launches (other epochs) were made visible by the kernel boundary.  The L1 then serves a smooth plane's few hot rows.
//
// Error behaviour as in k_decode8_lanes: every read of a stream is bounded by its length; a lane that has failed keeps walking with
// its samples clamped into the plane's range, so its contexts stay below 131 071, its rows inside its own table (a row index is
// always below the row count) and its stores inside its own frame (x < W, y < H); it reports its first error.
// Needs W >= 8 (the read-back of the row above looks four samples ahead of a row's end).
// ------------------------------------------------------------------------------------------

namespace {

// first row of a lane's tables in the launch's table buffer
__device__ __forceinline__ uint64_t lane_table_row(const LaneUniform &, const LaneView &v, uint32_t np, uint32_t rows) {
    return (uint64_t)v.slot * np * rows;
}
__device__ __forceinline__ uint64_t lane_table_row(const LaneMixed &g, const LaneView &v, uint32_t, uint32_t) { return g.slots[v.slot].table_row; }

}  // namespace

// RGB = false: gray16 streams, u16 frames straight to `out_base`.  RGB = true: Y / Co / Cg off the same reader as int32 planes
// (k_ycocg16_to_rgb converts them).  `table`: decode16_lanes_table_bytes of the launch's streams; epoch0 .. epoch0 + 2 are this
// launch's (one per plane).  G: LaneUniform or LaneMixed.
template <bool RGB, typename G>
__global__ __launch_bounds__(64) void k_decode16_lanes(const uint8_t *__restrict__ streams, const uint64_t *__restrict__ offsets,
                                                       const uint64_t *__restrict__ lens, G geo, void *out_base, uint4 *table,
                                                       uint32_t epoch0, int *__restrict__ status) {
    using ST = typename std::conditional<RGB, int32_t, uint16_t>::type;
    constexpr uint32_t NP = RGB ? 3u : 1u;
    constexpr bool PITCHED = std::is_same<G, LanePitched>::value;
    static_assert(!PITCHED || !RGB, "RGB lanes write planes; their views are the conversion kernel's");
    const uint32_t lane = lane_id();
    LaneView v;
    if (!lane_view(geo, lane, v)) return;
    const uint32_t img = v.img, W = v.W, H = v.H;
    const uint8_t *s = streams + offsets[img];
    const uint64_t slen = lens[img];
    const uint64_t npix = (uint64_t)W * H;
    int rc = lane_header_check(s, slen, RGB ? 1 : 0, 1, W, H);
    if (rc != FELICS_OK) {  // nothing of this stream is decoded (its lane leaves; the others go on)
        status[img] = rc;
        return;
    }
    LaneReader br;
    br.init(s + FELICS_HEADER_BYTES, slen - FELICS_HEADER_BYTES);
    const uint32_t rows = dec16l_rows(npix, NP);  // (wave-uniform)
    LaneQuad *tab0 = reinterpret_cast<LaneQuad *>(table) + lane_table_row(geo, v, NP, rows) * 4u;
    for (uint32_t plane = 0; plane < NP; plane++) {
        const int32_t p0 = (int32_t)br.get(32), p1 = (int32_t)br.get(32);  // compression.rs:166-167
        if (br.failed() && rc == FELICS_OK) rc = FELICS_E_IO;
        if (npix == 0) continue;
        // KEstimator::new: the plane's own table and epoch (rows of other epochs are empty); Y 0..65535, Co / Cg -65535..65535
        Lane16Step step{tab0 + (uint64_t)plane * rows * 4u, rows, epoch0 + plane, (RGB && plane > 0) ? -65535 : 0, 65535, 0};
        ST *out = lane_plane<ST>(geo, out_base, v, NP, plane, npix);
        int64_t pitch = 0;
        if constexpr (PITCHED) out = lane_pitched<ST>(geo, v, pitch);
        lane_walk_plane<ST, PITCHED>(br, step, out, pitch, W, H, p0, p1, rc);
    }
    if (br.failed() && rc == FELICS_OK) rc = FELICS_E_IO;  // (whatever else: it was decoding padding)
    status[img] = rc;
}

uint32_t decode16_lds_bytes(uint32_t W) {
    return DEC16_SLOTS * DEC16_ROW * 4 + DEC16_SLOTS * 4 + 2u * decode8_row_stride(W) * 4u;
}
size_t decode16_table_bytes(uint32_t n) { return (size_t)n * DEC16_CONTEXTS * DEC16_ROW * 4; }

namespace {

// LDS above 64 KiB: raise the kernel's limit (a launch of `lds` bytes of dynamic LDS follows)
template <typename Kernel>
hipError_t raise_lds(Kernel kernel, uint32_t lds) {
    if (lds <= 64u * 1024u) return hipSuccess;
    return hipFuncSetAttribute(reinterpret_cast<const void *>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)DECODE_LDS_LIMIT);
}

// A grid's second dimension holds at most 65 535 rows: every launch that puts a stream, a row or a region there is cut into runs of
// at most this many (the one rule; launch_conv_uniform, launch_conv_rows, launch_conv_views, the region conversions, launch_scatter_views).
constexpr uint32_t GRID_ROWS = 65535u;

// the conversion of n same-shape RGB streams: the kernels take the stream from blockIdx.y, so a run starts at its own planes, frames
// and status words
template <typename P, typename T>
void launch_conv_uniform(hipStream_t s, uint32_t n, uint32_t W, uint32_t H, P *planes, T *pixels, int *status) {
    const uint64_t npix = (uint64_t)W * H;
    const uint32_t bx = (uint32_t)std::min<uint64_t>((npix + 255) / 256, 1024u);
    if (!bx) return;
    for (uint32_t i0 = 0; i0 < n; i0 += GRID_ROWS) {
        const dim3 grid(bx, std::min(n - i0, GRID_ROWS));
        P *const pl = planes + (uint64_t)i0 * 3u * npix;
        T *const px = pixels + (uint64_t)i0 * 3u * npix;
        if constexpr (sizeof(T) == 1) hipLaunchKernelGGL(k_ycocg8_to_rgb<ConvUniform>, grid, dim3(256), 0, s, pl, px, ConvUniform{(uint32_t)npix}, status + i0);
        else hipLaunchKernelGGL(k_ycocg16_to_rgb<ConvUniform>, grid, dim3(256), 0, s, pl, px, ConvUniform{(uint32_t)npix}, status + i0);
    }
}

}  // namespace

hipError_t launch_decode16(hipStream_t s, const uint8_t *streams, const uint64_t *offsets, const uint64_t *lens, uint32_t n,
                           uint32_t W, uint32_t H, uint32_t color, uint16_t *pixels, int32_t *planes, uint32_t *table,
                           uint32_t epoch0, int *status) {
    if (n == 0) return hipSuccess;
    const uint32_t lds = decode16_lds_bytes(W);
    const hipError_t e = raise_lds(&k_decode16<DecUniform>, lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_decode16<DecUniform>, dim3(n), dim3(64), lds, s, streams, offsets, lens, DecUniform{W, H, color}, pixels, planes,
                       table, epoch0, status);
    if (color) launch_conv_uniform(s, n, W, H, planes, pixels, status);
    return hipGetLastError();
}

namespace {

// The lane launchers' pattern, a wave per workgroup: gray streams by `gray` straight into `pixels`; RGB streams by `rgb` into `planes`,
// then the conversion conv().  tail: the kernel's arguments behind its output (table, [epoch0,] status).
template <typename KG, typename GG, typename KR, typename GR, typename Conv, typename... Tail>
hipError_t launch_lanes(hipStream_t s, const uint8_t *streams, const uint64_t *offsets, const uint64_t *lens, uint32_t nwaves, uint32_t color,
                        KG gray, const GG &ggeo, void *pixels, KR rgb, const GR &rgeo, void *planes, Conv conv, Tail... tail) {
    if (nwaves == 0) return hipSuccess;
    if (!color) {
        hipLaunchKernelGGL(gray, dim3(nwaves), dim3(64), 0, s, streams, offsets, lens, ggeo, pixels, tail...);
        return hipGetLastError();
    }
    hipLaunchKernelGGL(rgb, dim3(nwaves), dim3(64), 0, s, streams, offsets, lens, rgeo, planes, tail...);
    conv();
    return hipGetLastError();
}

}  // namespace

hipError_t launch_decode16_lanes(hipStream_t s, const uint8_t *streams, const uint64_t *offsets, const uint64_t *lens, uint32_t n,
                                 uint32_t W, uint32_t H, uint32_t color, uint16_t *pixels, int32_t *planes, uint32_t *table,
                                 uint32_t epoch0, int *status) {
    const LaneUniform g{n, W, H};
    return launch_lanes(s, streams, offsets, lens, (n + 63) / 64, color, k_decode16_lanes<false, LaneUniform>, g, pixels,
                        k_decode16_lanes<true, LaneUniform>, g, planes, [&] { launch_conv_uniform(s, n, W, H, planes, pixels, status); },
                        reinterpret_cast<uint4 *>(table), epoch0, status);
}

size_t decode8_lanes_table_bytes(uint32_t n, uint32_t color) { return (size_t)n * (color ? 3u * DEC8L_TABLE_DW_RGB : DEC8L_TABLE_DW) * 4; }

// lane = stream (gray8 or RGB8, W >= 8); `table` = decode8_lanes_table_bytes(n, color) bytes, all zero; RGB: `planes` takes the int16
// planes (n * 3 * W * H), `pixels` the converted frames
hipError_t launch_decode8_lanes(hipStream_t s, const uint8_t *streams, const uint64_t *offsets, const uint64_t *lens, uint32_t n,
                                uint32_t W, uint32_t H, uint32_t color, uint8_t *pixels, int16_t *planes, uint32_t *table, int *status) {
    const LaneUniform g{n, W, H};
    return launch_lanes(s, streams, offsets, lens, (n + 63) / 64, color, k_decode8_lanes<false, LaneUniform>, g, pixels,
                        k_decode8_lanes<true, LaneUniform>, g, planes, [&] { launch_conv_uniform(s, n, W, H, planes, pixels, status); }, table,
                        status);
}

namespace {

// read_header (format.rs:63-84) as felics_read_header does it: each field read only if the stream holds it; then, for a valid
// header, the decode call's own rules: w * h < 2^32 (compression.rs:86), and at least C * (64 + max(0, w * h - 2)) bits behind the
// header (two raw 32-bit samples per plane, then at least one flag bit per pixel, padded to a byte)
__global__ __launch_bounds__(256) void k_read_headers(const uint8_t *__restrict__ streams, const uint64_t *__restrict__ offsets,
                                                      const uint64_t *__restrict__ lens, uint32_t n, DecodeHeader *__restrict__ out) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint8_t *s = streams + offsets[i];
    const uint64_t len = lens[i];
    DecodeHeader h = {0, 0, 0, 0, FELICS_OK, FELICS_OK};
    if (len < 4) h.status = FELICS_E_IO;
    else if (s[0] != 'F' || s[1] != 'L' || s[2] != 'C' || s[3] != 'S') h.status = FELICS_E_INVALID_SIGNATURE;
    else if (len < 5) h.status = FELICS_E_IO;
    else if (s[4] > 1) h.status = FELICS_E_INVALID_COLOR_TYPE;
    else if (len < 6) h.status = FELICS_E_IO;
    else if (s[5] > 1) h.status = FELICS_E_INVALID_PIXEL_DEPTH;
    else if (len < FELICS_HEADER_BYTES) h.status = FELICS_E_IO;
    h.dstatus = h.status;
    if (h.status == FELICS_OK) {
        h.color = s[4];
        h.depth = s[5];
        h.W = ((uint32_t)s[6] << 24) | ((uint32_t)s[7] << 16) | ((uint32_t)s[8] << 8) | s[9];
        h.H = ((uint32_t)s[10] << 24) | ((uint32_t)s[11] << 16) | ((uint32_t)s[12] << 8) | s[13];
        const uint64_t npix = (uint64_t)h.W * h.H;
        if (npix > 0xFFFFFFFFull) {
            h.dstatus = FELICS_E_INVALID_DIMENSIONS;
        } else {
            const uint64_t bits = (h.color ? 3u : 1u) * (64u + (npix > 2 ? npix - 2 : 0));
            if (len - FELICS_HEADER_BYTES < (bits + 7) / 8) h.dstatus = FELICS_E_IO;
        }
    }
    out[i] = h;
}

// the RGB conversion of `n` mixed rows (grid rows of at most 65 535)
template <typename P, typename T>
void launch_conv_rows(hipStream_t s, const DecodeRow *rows, uint32_t n, uint64_t max_npix, P *planes, T *pixels, int *status) {
    const uint32_t bx = (uint32_t)std::min<uint64_t>((max_npix + 255) / 256, 1024u);
    if (!bx) return;
    for (uint32_t r0 = 0; r0 < n; r0 += GRID_ROWS) {
        const uint32_t cnt = std::min(n - r0, GRID_ROWS);
        if constexpr (sizeof(T) == 1)
            hipLaunchKernelGGL(k_ycocg8_to_rgb<DecMixed>, dim3(bx, cnt), dim3(256), 0, s, planes, pixels, DecMixed{rows + r0}, status);
        else
            hipLaunchKernelGGL(k_ycocg16_to_rgb<DecMixed>, dim3(bx, cnt), dim3(256), 0, s, planes, pixels, DecMixed{rows + r0}, status);
    }
}

}  // namespace

hipError_t launch_read_headers(hipStream_t s, const uint8_t *streams, const uint64_t *offsets, const uint64_t *lens, uint32_t n,
                               DecodeHeader *out) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_read_headers, dim3((uint32_t)(((uint64_t)n + 255) / 256)), dim3(256), 0, s, streams, offsets, lens, n, out);
    return hipGetLastError();
}

uint32_t decode8_lds_bytes(uint32_t W, uint32_t color) {
    return (color ? nctx_of<int16_t>() : nctx_of<uint8_t>()) * 6 * 4 + 2u * decode8_row_stride(W) * 2u;
}

hipError_t launch_decode8(hipStream_t s, const uint8_t *streams, const uint64_t *offsets, const uint64_t *lens, uint32_t n,
                          uint32_t W, uint32_t H, uint32_t color, uint8_t *pixels, int16_t *planes, int *status) {
    if (n == 0) return hipSuccess;
    const uint32_t lds = decode8_lds_bytes(W, color);
    const hipError_t e = raise_lds(&k_decode8<DecUniform>, lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_decode8<DecUniform>, dim3(n), dim3(64), lds, s, streams, offsets, lens, DecUniform{W, H, color}, pixels, planes,
                       status);
    if (color) launch_conv_uniform(s, n, W, H, planes, pixels, status);
    return hipGetLastError();
}

hipError_t launch_decode8_seg(hipStream_t s, const uint8_t *streams, const uint64_t *offsets, const uint64_t *lens, const uint8_t *index,
                              uint64_t index_stride, uint32_t n, uint32_t W, uint32_t H, uint32_t color, uint32_t segment_pixels, uint32_t K,
                              uint8_t *pixels, int16_t *planes, int *seg_status, int *status) {
    if (n == 0) return hipSuccess;
    const uint32_t lds = decode8_lds_bytes(W, color);
    const hipError_t e = raise_lds(&k_decode8_seg, lds);
    if (e != hipSuccess) return e;
    const uint32_t per = (color ? 3u : 1u) * std::max(K, 1u);  // (n * per < 2^31: the caller's check)
    hipLaunchKernelGGL(k_decode8_seg, dim3(n * per), dim3(64), lds, s, streams, offsets, lens, index, index_stride, DecUniform{W, H, color},
                       segment_pixels, K, pixels, planes, seg_status);
    return launch_seg_finish(s, n, W, H, color, K, pixels, planes, seg_status, status);
}

size_t index8_lanes_table_bytes(uint64_t items, uint32_t color) { return (size_t)items * (color ? DEC8L_TABLE_DW_RGB : DEC8L_TABLE_DW) * 4; }

hipError_t launch_decode8_seg_lanes(hipStream_t s, const uint8_t *streams, const uint64_t *offsets, const uint64_t *lens, const uint8_t *index,
                                    uint64_t index_stride, uint32_t W, uint32_t H, uint32_t color, uint32_t segment_pixels, uint32_t K,
                                    uint32_t wave0, uint32_t nwaves, uint8_t *pixels, int16_t *planes, uint32_t *table, int *seg_status) {
    if (nwaves == 0) return hipSuccess;
    if (color)
        hipLaunchKernelGGL(k_decode8_seg_lanes<true>, dim3(nwaves), dim3(64), 0, s, streams, offsets, lens, index, index_stride, W, H, segment_pixels,
                           K, wave0, (void *)planes, table, seg_status);
    else
        hipLaunchKernelGGL(k_decode8_seg_lanes<false>, dim3(nwaves), dim3(64), 0, s, streams, offsets, lens, index, index_stride, W, H, segment_pixels,
                           K, wave0, (void *)pixels, table, seg_status);
    return hipGetLastError();
}

template <typename P, typename T>
hipError_t launch_seg_finish(hipStream_t s, uint32_t n, uint32_t W, uint32_t H, uint32_t color, uint32_t K, T *pixels, P *planes, const int *seg_status,
                             int *status) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_seg_status, dim3(n), dim3(64), 0, s, seg_status, (const RegionRow *)nullptr, (color ? 3u : 1u) * std::max(K, 1u), status);
    if (color) launch_conv_uniform(s, n, W, H, planes, pixels, status);
    return hipGetLastError();
}
template hipError_t launch_seg_finish(hipStream_t, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, uint8_t *, int16_t *, const int *, int *);
template hipError_t launch_seg_finish(hipStream_t, uint32_t, uint32_t, uint32_t, uint32_t, uint32_t, uint16_t *, int32_t *, const int *, int *);

hipError_t launch_decode8_regions(hipStream_t s, const uint8_t *streams, const uint64_t *offsets, const uint64_t *lens, const uint8_t *index,
                                  uint64_t index_stride, uint32_t W, uint32_t H, uint32_t color, uint32_t segment_pixels, uint32_t K,
                                  const RegionRow *rows, const RegionItem *items, uint32_t nitems, uint8_t *pixels, int16_t *planes,
                                  int *item_status) {
    if (nitems == 0) return hipSuccess;
    const uint32_t lds = decode8_lds_bytes(W, color);
    const hipError_t e = raise_lds(&k_decode8_region, lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_decode8_region, dim3(nitems), dim3(64), lds, s, streams, offsets, lens, index, index_stride, DecUniform{W, H, color},
                       segment_pixels, K, rows, items, pixels, planes, item_status);
    return hipGetLastError();
}

hipError_t launch_decode8_rows(hipStream_t s, const uint8_t *streams, const uint64_t *offsets, const uint64_t *lens, const DecodeRow *rows,
                               uint32_t n, uint32_t lds, uint64_t max_npix, bool any_rgb, uint8_t *pixels, int16_t *planes, int *status) {
    if (n == 0) return hipSuccess;
    const hipError_t e = raise_lds(&k_decode8<DecMixed>, lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_decode8<DecMixed>, dim3(n), dim3(64), lds, s, streams, offsets, lens, DecMixed{rows}, pixels, planes, status);
    if (any_rgb) launch_conv_rows(s, rows, n, max_npix, planes, pixels, status);
    return hipGetLastError();
}

hipError_t launch_decode8_lanes_waves(hipStream_t s, const uint8_t *streams, const uint64_t *offsets, const uint64_t *lens, const LaneWave *waves,
                                      uint32_t nwaves, const LaneSlot *slots, uint32_t color, const DecodeRow *conv, uint32_t nconv,
                                      uint64_t max_npix, uint8_t *pixels, int16_t *planes, uint32_t *table, int *status) {
    const LaneMixed g{waves, slots};
    return launch_lanes(s, streams, offsets, lens, nwaves, color, k_decode8_lanes<false, LaneMixed>, g, pixels, k_decode8_lanes<true, LaneMixed>, g,
                        planes, [&] { launch_conv_rows(s, conv, nconv, max_npix, planes, pixels, status); }, table, status);
}

hipError_t launch_decode16_lanes_waves(hipStream_t s, const uint8_t *streams, const uint64_t *offsets, const uint64_t *lens, const LaneWave *waves,
                                       uint32_t nwaves, const LaneSlot *slots, uint32_t color, const DecodeRow *conv, uint32_t nconv,
                                       uint64_t max_npix, uint16_t *pixels, int32_t *planes, uint32_t *table, uint32_t epoch0, int *status) {
    const LaneMixed g{waves, slots};
    return launch_lanes(s, streams, offsets, lens, nwaves, color, k_decode16_lanes<false, LaneMixed>, g, pixels, k_decode16_lanes<true, LaneMixed>, g,
                        planes, [&] { launch_conv_rows(s, conv, nconv, max_npix, planes, pixels, status); }, reinterpret_cast<uint4 *>(table), epoch0,
                        status);
}

hipError_t launch_decode16_rows(hipStream_t s, const uint8_t *streams, const uint64_t *offsets, const uint64_t *lens, const DecodeRow *rows,
                                uint32_t n, uint32_t lds, uint64_t max_npix, bool any_rgb, uint16_t *pixels, int32_t *planes, uint32_t *table,
                                uint32_t epoch0, int *status) {
    if (n == 0) return hipSuccess;
    const hipError_t e = raise_lds(&k_decode16<DecMixed>, lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_decode16<DecMixed>, dim3(n), dim3(64), lds, s, streams, offsets, lens, DecMixed{rows}, pixels, planes, table, epoch0,
                       status);
    if (any_rgb) launch_conv_rows(s, rows, n, max_npix, planes, pixels, status);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------
// felics_decompress_views_device: the launches above with the pitched / strided policies where a launch needs them.
// ------------------------------------------------------------------------------------------

namespace {

// the RGB conversion of `n` rows through their views (ConvStrided), or, where every row is the dense layout, launch_conv_rows as it is
template <typename P, typename T>
void launch_conv_views(hipStream_t s, const DecodeRow *rows, uint32_t n, uint64_t max_npix, P *planes, int *status, const DecodeViews &cv) {
    if (!cv.strided) return launch_conv_rows(s, rows, n, max_npix, planes, (T *)nullptr, status);
    const uint32_t bx = (uint32_t)std::min<uint64_t>((max_npix + 255) / 256, 1024u);
    if (!bx) return;
    for (uint32_t r0 = 0; r0 < n; r0 += GRID_ROWS) {
        const uint32_t cnt = std::min(n - r0, GRID_ROWS);
        const ConvStrided g{{rows + r0}, cv.views + r0};
        if constexpr (sizeof(T) == 1)
            hipLaunchKernelGGL(k_ycocg8_to_rgb<ConvStrided>, dim3(bx, cnt), dim3(256), 0, s, planes, (T *)nullptr, g, status);
        else
            hipLaunchKernelGGL(k_ycocg16_to_rgb<ConvStrided>, dim3(bx, cnt), dim3(256), 0, s, planes, (T *)nullptr, g, status);
    }
}

// k_scatter_view: the inverse of k_gather_view (felics_wide.hip) for a table of frames -- a dense frame in the context's staging
// buffer written through its view's strides, sample by sample.  blockIdx.z names the table row, a workgroup row (blockIdx.y, strided)
// an image row, consecutive threads consecutive samples of it: the reads are coalesced, the writes as far as the view allows.
template <typename T>
__global__ __launch_bounds__(256) void k_scatter_view(const ScatterRow *__restrict__ rows, const int *__restrict__ status) {
    const ScatterRow r = rows[blockIdx.z];
    if (status[r.stream] != FELICS_OK) return;
    uint8_t *data = reinterpret_cast<uint8_t *>(const_cast<void *>(r.v.data));
    const uint64_t row = (uint64_t)r.W * r.C;  // samples
    for (uint32_t y = blockIdx.y; y < r.H; y += gridDim.y) {
        uint8_t *dst = data + (int64_t)y * r.v.row_stride;
        const T *src = reinterpret_cast<const T *>(r.src) + (uint64_t)y * row;
        for (uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; j < row; j += (uint64_t)gridDim.x * blockDim.x) {
            const uint64_t x = r.C == 1 ? j : j / 3u;
            const int64_t c = (int64_t)(j - x * r.C);
            *reinterpret_cast<T *>(dst + (int64_t)x * r.v.pixel_stride + c * r.v.channel_stride) = src[j];
        }
    }
}

}  // namespace

template <typename T>
hipError_t launch_scatter_views(hipStream_t s, const ScatterRow *rows, uint32_t n, uint32_t max_row_samples, uint32_t max_h, const int *status) {
    if (!n || !max_row_samples || !max_h) return hipSuccess;
    const uint32_t bx = std::max(1u, std::min((max_row_samples + 255u) / 256u, 64u));
    const uint32_t by = std::min(max_h, 1024u);
    for (uint32_t r0 = 0; r0 < n; r0 += GRID_ROWS)
        hipLaunchKernelGGL((k_scatter_view<T>), dim3(bx, by, std::min(n - r0, GRID_ROWS)), dim3(256), 0, s, rows + r0, status);
    return hipGetLastError();
}
template hipError_t launch_scatter_views<uint8_t>(hipStream_t, const ScatterRow *, uint32_t, uint32_t, uint32_t, const int *);
template hipError_t launch_scatter_views<uint16_t>(hipStream_t, const ScatterRow *, uint32_t, uint32_t, uint32_t, const int *);

hipError_t launch_decode8_rows_views(hipStream_t s, const uint8_t *streams, const uint64_t *offsets, const uint64_t *lens, const DecodeRow *rows,
                                     uint32_t n, uint32_t lds, uint64_t max_npix, bool any_rgb, int16_t *planes, int *status, const DecodeViews &dv) {
    if (n == 0) return hipSuccess;
    const void *kernel = dv.pitched ? reinterpret_cast<const void *>(&k_decode8<DecPitched>) : reinterpret_cast<const void *>(&k_decode8<DecMixed>);
    const hipError_t e = raise_lds(kernel, lds);
    if (e != hipSuccess) return e;
    if (dv.pitched)
        hipLaunchKernelGGL(k_decode8<DecPitched>, dim3(n), dim3(64), lds, s, streams, offsets, lens, DecPitched{{rows}, dv.views}, (uint8_t *)nullptr,
                           planes, status);
    else
        hipLaunchKernelGGL(k_decode8<DecMixed>, dim3(n), dim3(64), lds, s, streams, offsets, lens, DecMixed{rows}, (uint8_t *)nullptr, planes, status);
    if (any_rgb) launch_conv_views<int16_t, uint8_t>(s, rows, n, max_npix, planes, status, dv);
    return hipGetLastError();
}

hipError_t launch_decode16_rows_views(hipStream_t s, const uint8_t *streams, const uint64_t *offsets, const uint64_t *lens, const DecodeRow *rows,
                                      uint32_t n, uint32_t lds, uint64_t max_npix, bool any_rgb, int32_t *planes, uint32_t *table, uint32_t epoch0,
                                      int *status, const DecodeViews &dv) {
    if (n == 0) return hipSuccess;
    const void *kernel = dv.pitched ? reinterpret_cast<const void *>(&k_decode16<DecPitched>) : reinterpret_cast<const void *>(&k_decode16<DecMixed>);
    const hipError_t e = raise_lds(kernel, lds);
    if (e != hipSuccess) return e;
    if (dv.pitched)
        hipLaunchKernelGGL(k_decode16<DecPitched>, dim3(n), dim3(64), lds, s, streams, offsets, lens, DecPitched{{rows}, dv.views},
                           (uint16_t *)nullptr, planes, table, epoch0, status);
    else
        hipLaunchKernelGGL(k_decode16<DecMixed>, dim3(n), dim3(64), lds, s, streams, offsets, lens, DecMixed{rows}, (uint16_t *)nullptr, planes, table,
                           epoch0, status);
    if (any_rgb) launch_conv_views<int32_t, uint16_t>(s, rows, n, max_npix, planes, status, dv);
    return hipGetLastError();
}

hipError_t launch_decode8_lanes_waves_views(hipStream_t s, const uint8_t *streams, const uint64_t *offsets, const uint64_t *lens, const LaneWave *waves,
                                            uint32_t nwaves, const LaneSlot *slots, uint32_t color, const DecodeRow *conv, uint32_t nconv,
                                            uint64_t max_npix, int16_t *planes, uint32_t *table, int *status, const DecodeViews &dv,
                                            const DecodeViews &cv) {
    const LaneMixed g{waves, slots};
    const auto convert = [&] { launch_conv_views<int16_t, uint8_t>(s, conv, nconv, max_npix, planes, status, cv); };
    if (dv.pitched)  // (gray lanes write through their views; RGB lanes write planes either way)
        return launch_lanes(s, streams, offsets, lens, nwaves, color, k_decode8_lanes<false, LanePitched>, LanePitched{g, dv.views}, nullptr,
                            k_decode8_lanes<true, LaneMixed>, g, planes, convert, table, status);
    return launch_lanes(s, streams, offsets, lens, nwaves, color, k_decode8_lanes<false, LaneMixed>, g, nullptr, k_decode8_lanes<true, LaneMixed>, g,
                        planes, convert, table, status);
}

hipError_t launch_decode16_lanes_waves_views(hipStream_t s, const uint8_t *streams, const uint64_t *offsets, const uint64_t *lens, const LaneWave *waves,
                                             uint32_t nwaves, const LaneSlot *slots, uint32_t color, const DecodeRow *conv, uint32_t nconv,
                                             uint64_t max_npix, int32_t *planes, uint32_t *table, uint32_t epoch0, int *status,
                                             const DecodeViews &dv, const DecodeViews &cv) {
    const LaneMixed g{waves, slots};
    const auto convert = [&] { launch_conv_views<int32_t, uint16_t>(s, conv, nconv, max_npix, planes, status, cv); };
    uint4 *const tab = reinterpret_cast<uint4 *>(table);
    if (dv.pitched)
        return launch_lanes(s, streams, offsets, lens, nwaves, color, k_decode16_lanes<false, LanePitched>, LanePitched{g, dv.views}, nullptr,
                            k_decode16_lanes<true, LaneMixed>, g, planes, convert, tab, epoch0, status);
    return launch_lanes(s, streams, offsets, lens, nwaves, color, k_decode16_lanes<false, LaneMixed>, g, nullptr, k_decode16_lanes<true, LaneMixed>, g,
                        planes, convert, tab, epoch0, status);
}

// ------------------------------------------------------------------------------------------
// felics_decompress_views_device_indexed: the walk from a checkpoint with the view sink, per LDS class; a pass's tail.
// ------------------------------------------------------------------------------------------

static_assert(INDEX_LDS_LIMIT == DECODE_LDS_LIMIT, "felics_index.h names the wave form's LDS limit for the host model");
static_assert(index16_lds_bytes(0) == DEC16_SLOTS * DEC16_ROW * 4 + DEC16_SLOTS * 4 && index16_lds_bytes(65) - index16_lds_bytes(0) == 2u * 128u * 4u,
              "felics_index.h repeats decode16_lds_bytes for the host model");

hipError_t launch_decode8_seg_views(hipStream_t s, const uint8_t *streams, const uint64_t *offsets, const uint64_t *lens, const uint8_t *index,
                                    const IndexViewRow *rows, const IndexViewItem *items, uint32_t nitems, uint32_t lds, int16_t *planes,
                                    int *item_status) {
    if (nitems == 0) return hipSuccess;
    const hipError_t e = raise_lds(&k_decode8_seg_views, lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_decode8_seg_views, dim3(nitems), dim3(64), lds, s, streams, offsets, lens, index, rows, items, planes, item_status);
    return hipGetLastError();
}

template <typename P, typename T>
hipError_t launch_seg_views_finish(hipStream_t s, uint32_t n, const RegionRow *regions, const int *item_status, const DecodeRow *conv,
                                   const ViewRow *views, uint64_t max_npix, P *planes, int *status) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_seg_status, dim3(n), dim3(64), 0, s, item_status, regions, 0u, status);
    if (max_npix) launch_conv_views<P, T>(s, conv, n, max_npix, planes, status, DecodeViews{views, false, true});
    return hipGetLastError();
}
template hipError_t launch_seg_views_finish<int16_t, uint8_t>(hipStream_t, uint32_t, const RegionRow *, const int *, const DecodeRow *, const ViewRow *,
                                                              uint64_t, int16_t *, int *);
template hipError_t launch_seg_views_finish<int32_t, uint16_t>(hipStream_t, uint32_t, const RegionRow *, const int *, const DecodeRow *, const ViewRow *,
                                                               uint64_t, int32_t *, int *);

// ------------------------------------------------------------------------------------------
// felics_decompress_batch_device_indexed16: a pass of k_decode16_seg (its tail: launch_seg_finish).
// ------------------------------------------------------------------------------------------

hipError_t launch_decode16_seg(hipStream_t s, const uint8_t *streams, const uint64_t *offsets, const uint64_t *lens, const uint8_t *index,
                               const uint64_t *idx_offsets, const uint64_t *idx_lens, uint32_t W, uint32_t H, uint32_t color, uint32_t segment_pixels,
                               uint32_t K, uint32_t item0, uint32_t nitems, uint16_t *pixels, int32_t *planes, uint32_t *table, uint32_t epoch,
                               int *seg_status, unsigned long long *rows_loaded) {
    if (nitems == 0) return hipSuccess;
    const uint32_t lds = decode16_lds_bytes(W);
    const hipError_t e = raise_lds(&k_decode16_seg, lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_decode16_seg, dim3(nitems), dim3(64), lds, s, streams, offsets, lens, index, idx_offsets, idx_lens, DecUniform{W, H, color},
                       segment_pixels, K, item0, pixels, planes, table, epoch, seg_status, rows_loaded);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------
// felics_decompress_regions_device_indexed16: a pass of k_decode16_region; the finish of both region calls.
// ------------------------------------------------------------------------------------------

hipError_t launch_decode16_regions(hipStream_t s, const uint8_t *streams, const uint64_t *offsets, const uint64_t *lens, const uint8_t *index,
                                   const uint64_t *idx_offsets, const uint64_t *idx_lens, uint32_t W, uint32_t H, uint32_t color,
                                   uint32_t segment_pixels, uint32_t K, const RegionRow *rows, const RegionItem *items, uint32_t item0, uint32_t nitems,
                                   uint8_t *pixels, int32_t *planes, uint32_t *table, uint32_t epoch, int *item_status,
                                   unsigned long long *rows_loaded) {
    if (nitems == 0) return hipSuccess;
    const uint32_t lds = decode16_lds_bytes(W);
    const hipError_t e = raise_lds(&k_decode16_region, lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_decode16_region, dim3(nitems), dim3(64), lds, s, streams, offsets, lens, index, idx_offsets, idx_lens,
                       DecUniform{W, H, color}, segment_pixels, K, rows, items, item0, pixels, planes, table, epoch, item_status, rows_loaded);
    return hipGetLastError();
}

template <typename P, typename T>
hipError_t launch_regions_finish(hipStream_t s, const RegionRow *rows, uint32_t nregions, uint64_t max_crop, T *pixels, P *planes,
                                 const int *item_status, int *status) {
    if (nregions == 0) return hipSuccess;
    hipLaunchKernelGGL(k_seg_status, dim3(nregions), dim3(64), 0, s, item_status, rows, 0u, status);
    // the crops differ in size: one launch (per GRID_ROWS regions) sized by the largest, a region's blocks stride over its own w * h
    const uint32_t bx = (uint32_t)std::min<uint64_t>((max_crop + 255) / 256, 1024u);
    for (uint32_t r0 = 0; bx && r0 < nregions; r0 += GRID_ROWS) {
        const dim3 grid(bx, std::min(nregions - r0, GRID_ROWS));
        if constexpr (sizeof(T) == 1) hipLaunchKernelGGL(k_ycocg8_to_rgb<ConvRegion>, grid, dim3(256), 0, s, planes, pixels, ConvRegion{rows, r0}, status);
        else hipLaunchKernelGGL(k_ycocg16_to_rgb<ConvRegion>, grid, dim3(256), 0, s, planes, pixels, ConvRegion{rows, r0}, status);
    }
    return hipGetLastError();
}
template hipError_t launch_regions_finish(hipStream_t, const RegionRow *, uint32_t, uint64_t, uint8_t *, int16_t *, const int *, int *);
template hipError_t launch_regions_finish(hipStream_t, const RegionRow *, uint32_t, uint64_t, uint16_t *, int32_t *, const int *, int *);

// ------------------------------------------------------------------------------------------
// felics_decompress_views_device_indexed16: a launch of k_decode16_seg_views (a stream pass's tail: launch_seg_views_finish).
// ------------------------------------------------------------------------------------------

hipError_t launch_decode16_seg_views(hipStream_t s, const uint8_t *streams, const uint64_t *offsets, const uint64_t *lens, const uint8_t *index,
                                     const uint64_t *idx_lens, const IndexViewRow *rows, const IndexViewItem *items, uint32_t nitems, uint32_t lds,
                                     int32_t *planes, uint32_t *table, uint32_t epoch, int *item_status, unsigned long long *rows_loaded) {
    if (nitems == 0) return hipSuccess;
    const hipError_t e = raise_lds(&k_decode16_seg_views, lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_decode16_seg_views, dim3(nitems), dim3(64), lds, s, streams, offsets, lens, index, idx_lens, rows, items, planes, table,
                       epoch, item_status, rows_loaded);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------
// felics_decompress_region_views_device_indexed and its 16-bit form: a launch of the region walk with the region view sink (a pass's
// tail: launch_seg_views_finish).
// ------------------------------------------------------------------------------------------

hipError_t launch_decode8_region_views(hipStream_t s, const uint8_t *streams, const uint64_t *offsets, const uint64_t *lens, const uint8_t *index,
                                       const RegionViewStream *srows, const RegionRow *regions, const ViewRow *views, const RegionItem *items,
                                       uint32_t nitems, uint32_t lds, int16_t *planes, int *item_status) {
    if (nitems == 0) return hipSuccess;
    const hipError_t e = raise_lds(&k_decode8_region_views, lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_decode8_region_views, dim3(nitems), dim3(64), lds, s, streams, offsets, lens, index, srows, regions, views, items, planes,
                       item_status);
    return hipGetLastError();
}

hipError_t launch_decode16_region_views(hipStream_t s, const uint8_t *streams, const uint64_t *offsets, const uint64_t *lens, const uint8_t *index,
                                        const uint64_t *idx_lens, const RegionViewStream *srows, const RegionRow *regions, const ViewRow *views,
                                        const RegionItem *items, uint32_t nitems, uint32_t lds, int32_t *planes, uint32_t *table, uint32_t epoch,
                                        int *item_status, unsigned long long *rows_loaded) {
    if (nitems == 0) return hipSuccess;
    const hipError_t e = raise_lds(&k_decode16_region_views, lds);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(k_decode16_region_views, dim3(nitems), dim3(64), lds, s, streams, offsets, lens, index, idx_lens, srows, regions, views, items,
                       planes, table, epoch, item_status, rows_loaded);
    return hipGetLastError();
}

hipError_t launch_read_index_headers(hipStream_t s, const uint8_t *index, const uint64_t *idx_offsets, const uint64_t *idx_lens, uint32_t n,
                                     uint8_t *out) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_read_index_headers, dim3((uint32_t)(((uint64_t)n * 4 + 255) / 256)), dim3(256), 0, s, index, idx_offsets, idx_lens, n, out);
    return hipGetLastError();
}

}  // namespace felics
