"""What the tests of regions into views share (test_region_views_cpu.py, test_region_views_gpu.py, test_region16_views_gpu.py): streams
and indexes between guard bytes in device memory, the raw calls of both depths, the host models' raw calls, the windows of the 16-bit
cases, and the rules of the call that the GPU tests recompute from include/felics.h: the plan of a region by marking pixels, the LDS
class of a stream's row, the passes and the launches.  The layouts are index_views_common.layouts with the WINDOW's size."""
import ctypes as C
import os

import numpy as np

from tests import index16_views_common as vc16
from tests import index_views_common as vc
from tests import region_common as rc

OK = vc.OK
E_INVALID_DIMENSIONS = vc.E_INVALID_DIMENSIONS
E_UNSUPPORTED = vc.E_UNSUPPORTED
E_INVALID_ARGUMENT = vc.E_INVALID_ARGUMENT
E_INVALID_INDEX = vc.E_INVALID_INDEX
GUARD = 256
UNSET = 77  # a status word the call did not write

# Windows of the 16-bit cases whose shapes region_common.FIXED does not know, segments of 4096 pixels.  64 x 130: segment 0 is rows
# 0-63, 1 rows 64-127, 2 rows 128-129.  33 x 130: pixel 4096 is (4, 124), so segment 1 starts in mid-row.
FIXED16 = {
    (64, 130): [
        (10, 10, 5, 5),      # an early stop in segment 0
        (5, 60, 10, 8),      # segments 0 and 1, segment 0 walked to its end
        (0, 128, 64, 2),     # the last segment alone, to the image's end
        (0, 0, 64, 130),     # the full frame
    ],
    (33, 130): [
        (0, 124, 33, 1),     # straddles the boundary in mid-row
        (20, 100, 13, 30),   # the right edge through both segments
        (0, 0, 33, 130),
    ],
}


def fixed_windows(w, h):
    return rc.FIXED.get((w, h)) or FIXED16[(w, h)]


class Inputs:
    """Streams (at odd offsets too) and indexes (at multiples of `align`, 0x5A between them) in device memory, each blob between GUARD
    bytes of 0x5A.  check(): both buffers are what was uploaded."""

    def __init__(self, streams, indexes, align, ilens=None):
        import torch

        assert GUARD % align == 0
        blob, offs = bytearray(b"\x5a" * GUARD), []
        for i, s in enumerate(streams):
            blob += b"\x5a" * (i % 3)
            offs.append(len(blob) - GUARD)
            blob += s
        blob += b"\x5a" * GUARD
        iblob, ioffs = bytearray(b"\x5a" * GUARD), []
        for i, x in enumerate(indexes):
            iblob += b"\x5a" * ((-len(iblob)) % align + align * (i % 2))
            ioffs.append(len(iblob) - GUARD)
            iblob += x
        iblob += b"\x5a" * GUARD
        self.host_s, self.host_i = np.frombuffer(bytes(blob), np.uint8).copy(), np.frombuffer(bytes(iblob), np.uint8).copy()
        self.d_s, self.d_i = torch.from_numpy(self.host_s).cuda(), torch.from_numpy(self.host_i).cuda()
        torch.cuda.synchronize()
        assert (self.d_i.data_ptr() + GUARD) % align == 0
        self.offs = np.asarray(offs, np.uint64)
        self.lens = np.asarray([len(s) for s in streams], np.uint64)
        self.ioffs = np.asarray(ioffs, np.uint64)
        self.ilens = np.asarray([len(x) for x in indexes] if ilens is None else ilens, np.uint64)

    @property
    def streams_ptr(self):
        return self.d_s.data_ptr() + GUARD

    @property
    def index_ptr(self):
        return self.d_i.data_ptr() + GUARD

    def check(self):
        assert (self.d_s.cpu().numpy() == self.host_s).all() and (self.d_i.cpu().numpy() == self.host_i).all()


def _u64(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint64)) if a is not None else None


def device_call(api, enc, wide, p, regions, views, ready_event=None, ioffs=None, n_streams=None):
    """One felics_decompress_region_views_device_indexed (wide: _indexed_wide) call: (rc, stream headers as tuples, status per region);
    status is UNSET where the call wrote none."""
    nr = len(regions)
    n = len(p.offs) if n_streams is None else n_streams
    st = np.full(max(nr, 1), UNSET, np.int32)
    hd = (api._CHeader * max(n, 1))()
    regs = (api._CRegion * max(nr, 1))(*[api._CRegion(*(int(v) for v in r)) for r in regions])
    cv = (api._CView * max(nr, 1))(*[api._cview(v) for v in views])
    L = api.lib()
    call = L.felics_decompress_region_views_device_indexed_wide if wide else L.felics_decompress_region_views_device_indexed
    code = call(enc._h, n, p.streams_ptr, _u64(p.offs), _u64(p.lens), p.index_ptr, _u64(p.ioffs if ioffs is None else ioffs), _u64(p.ilens),
                nr, regs, cv, int(ready_event) if ready_event else None, hd, st.ctypes.data_as(C.POINTER(C.c_int)))
    return code, [(h.color_type, h.pixel_depth, h.width, h.height) for h in hd[:n]], st[:nr].copy()


def host_call(api, wide, stream, index, window, view):
    """the host model on raw arguments: window (x, y, w, h), view the library's tuple over HOST memory.  Returns the code."""
    s = np.frombuffer(stream, np.uint8)
    i = np.frombuffer(index, np.uint8)
    L = api.lib()
    call = L.felics_decompress_region_indexed_view_wide if wide else L.felics_decompress_region_indexed_view
    reg = api._CRegion(0, *window)
    cv = api._cview(view)
    return call(s.ctypes.data if len(s) else None, len(s), i.ctypes.data if len(i) else None, len(i), C.byref(reg), C.byref(cv), None)


def host_view(v, depth16):
    """the library's view tuple of numpy view v over host memory"""
    f = vc16.view_tuple if depth16 else vc.view_tuple
    base = v.__array_interface__["data"][0]
    return f(v, base, base)


# ---- the plan, written out from include/felics.h ---------------------------------------------------------------------------------------

def plan(w, h, seg, planes, window):
    """(needed segments, waves, pixels walked) of one window of a w x h stream cut every seg pixels: the segments by marking, each
    walked from its first pixel to min(its end, the image's end, the pixel behind the window's last one), once per plane"""
    x, y, ww, hh = window
    if ww == 0 or hh == 0:
        return [], 0, 0
    need = rc.needed_by_marking(w, h, seg, window)
    last = (y + hh - 1) * w + x + ww
    pixels = sum(min(w * h, (j + 1) * seg, last) - j * seg for j in need)
    return need, planes * len(need), planes * pixels


def lds8(w, rgb):
    """the dynamic LDS of the 8-bit wave form (include/felics.h): 256 or 512 estimator rows of six words, two rows of int16
    padded to whole blocks of 64"""
    return (512 if rgb else 256) * 6 * 4 + 2 * ((w + 63) // 64 * 64) * 2


def lds_class(w, rgb, depth16):
    b = vc16.lds_bytes(w) if depth16 else lds8(w, rgb)
    return next(c for c, top in enumerate((16 << 10, 32 << 10, 64 << 10, 160 << 10)) if b <= top)


def passes_and_launches(rows, cap, depth16, k=None):
    """rows: per region of the call, in order, (stream width, rgb, window w, window h, waves), the regions that launch waves only.
    Passes: consecutive regions whose crop-sized planes (6 or 12 bytes per RGB crop pixel) fit cap; launches: per pass and LDS class
    that holds a wave, one -- or, 16-bit with k tables, ceil(waves / k).  Returns (passes, launches, the largest pass's plane bytes)."""
    per = 12 if depth16 else 6
    groups, acc, most = [[]], 0, 0
    for row in rows:
        b = per * row[2] * row[3] if row[1] else 0
        if acc and acc + b > cap:
            groups.append([])
            acc = 0
        groups[-1].append(row)
        acc += b
        most = max(most, acc)
    n = 0
    for g in groups:
        for c in range(4):
            cnt = sum(r[4] for r in g if lds_class(r[0], r[1], depth16) == c)
            n += (cnt + k - 1) // k if k else int(cnt > 0)
    return len(groups), n, most


class Env:
    """Sets environment variables the library reads per call and restores them."""

    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        os.environ.update(self.kv)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def delta(after, before):
    return {k: after[k] - before[k] for k in after}
