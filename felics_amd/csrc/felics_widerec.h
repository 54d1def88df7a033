// felics_widerec.h -- the event record of the 16-bit encode path and the words k_wide_plan leaves about the records, for the kernels
// that write and sort them (felics_wide.hip) and the ones that read the sorted records again (felics_index16.hip).
//
// One 64-bit record per out-of-range sample:
//     bits 0..17   context Delta = H - L            (<= 131 070)
//     bits 18..34  the value that gets Rice-coded   (<= 131 069)
//     bits 35..63  the sample's index in its plane  (< 2^29: the host bounds the image size)
#ifndef FELICS_WIDEREC_H
#define FELICS_WIDEREC_H

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace felics {

constexpr uint32_t REC_CTX_BITS = 18, REC_E_BITS = 17;

__device__ __forceinline__ uint64_t make_rec(uint32_t ctx, uint32_t e, uint32_t pix) {
    return (uint64_t)ctx | ((uint64_t)e << REC_CTX_BITS) | ((uint64_t)pix << (REC_CTX_BITS + REC_E_BITS));
}
__device__ __forceinline__ uint32_t rec_ctx(uint64_t r) { return (uint32_t)r & ((1u << REC_CTX_BITS) - 1u); }
__device__ __forceinline__ uint32_t rec_e(uint64_t r) { return (uint32_t)(r >> REC_CTX_BITS) & ((1u << REC_E_BITS) - 1u); }
__device__ __forceinline__ uint32_t rec_pix(uint64_t r) { return (uint32_t)(r >> (REC_CTX_BITS + REC_E_BITS)); }

// meta (u32): [0] records in all, [1] sort tiles in all, then plane_ev0[P + 1] at WMETA_EV0 (a plane's first record; the sorted records
// of plane p are plane_ev0[p] .. plane_ev0[p + 1] - 1), stile_first[P + 1] behind it.
constexpr uint32_t WMETA_EV0 = 4;

constexpr int WIDE_NK = 15;             // K_VALUES = 0..=14 (traits.rs:36)
constexpr uint32_t WIDE_HALVE = 1024;   // COUNT_SCALING (traits.rs:40)

}  // namespace felics

#endif
