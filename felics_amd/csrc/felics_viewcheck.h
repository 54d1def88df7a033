// felics_viewcheck.h -- the checks of a felics_view that need no device and nothing of HIP: what felics_view_extent, felics_view_writable
// and the device calls make of a view (felics_mixed.cpp, felics_decode_device.cpp), and what the host model of the indexed views call
// makes of it (felics_index.cpp, which the sanitizer driver links without the rest of the library).
#ifndef FELICS_VIEWCHECK_H
#define FELICS_VIEWCHECK_H

#include <stdint.h>

#include <algorithm>

#include "../../include/felics.h"

namespace felics {

// enums, w * h < 2^32 (compression.rs:86), NULL data only for a zero-sized view, even addresses and strides at depth 16
inline int view_args_check(const felics_view &v) {
    if (v.color != FELICS_COLOR_GRAY && v.color != FELICS_COLOR_RGB) return FELICS_E_INVALID_COLOR_TYPE;
    if (v.depth != FELICS_DEPTH_8 && v.depth != FELICS_DEPTH_16) return FELICS_E_INVALID_PIXEL_DEPTH;
    const uint64_t npix = (uint64_t)v.width * v.height;
    if (npix > 0xFFFFFFFFull) return FELICS_E_INVALID_DIMENSIONS;
    const bool rgb = v.color == FELICS_COLOR_RGB;
    if (!v.data && npix) return FELICS_E_INVALID_ARGUMENT;
    if (v.depth == FELICS_DEPTH_16 && (((uintptr_t)v.data | (uint64_t)v.row_stride | (uint64_t)v.pixel_stride | (rgb ? (uint64_t)v.channel_stride : 0u)) & 1u))
        return FELICS_E_INVALID_ARGUMENT;
    return FELICS_OK;
}

// the hull [lo, hi) of the samples' bytes relative to data (0, 0 for a zero-sized view); it must fit 64 bits
inline int view_hull(const felics_view &v, int64_t &lo, int64_t &hi) {
    lo = hi = 0;
    if (!v.width || !v.height) return FELICS_OK;
    const uint32_t planes = v.color == FELICS_COLOR_RGB ? 3 : 1;
    __int128 l = 0, h = v.depth == FELICS_DEPTH_16 ? 2 : 1;
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

// felics_view_writable: the two above, then the nested rule -- of the axes with more than one step, each stride (by size) at least
// the whole extent of the one below it
inline int view_writable_code(const felics_view &v) {
    int64_t lo, hi;
    int rc = view_args_check(v);
    if (!rc) rc = view_hull(v, lo, hi);
    if (rc || !v.width || !v.height) return rc;
    struct Axis {
        unsigned __int128 stride;
        uint64_t extent;
    } ax[3];
    int na = 0;
    auto mag = [](int64_t s) { return s < 0 ? (unsigned __int128)(-(__int128)s) : (unsigned __int128)s; };
    if (v.width > 1) ax[na++] = Axis{mag(v.pixel_stride), v.width};
    if (v.height > 1) ax[na++] = Axis{mag(v.row_stride), v.height};
    if (v.color == FELICS_COLOR_RGB) ax[na++] = Axis{mag(v.channel_stride), 3};
    for (int k = 1; k < na; k++)  // (by stride, ascending: three entries at the most)
        for (int m = k; m > 0 && ax[m].stride < ax[m - 1].stride; m--) std::swap(ax[m], ax[m - 1]);
    unsigned __int128 least = v.depth == FELICS_DEPTH_16 ? 2 : 1;  // the sample itself is the innermost extent
    for (int k = 0; k < na; k++) {
        if (ax[k].stride < least) return FELICS_E_INVALID_ARGUMENT;
        least = ax[k].stride * ax[k].extent;
    }
    return FELICS_OK;
}

}  // namespace felics

#endif
