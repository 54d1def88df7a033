"""What the tests of the indexed views call for 16-bit streams share (test_index16_views_cpu.py, test_index16_views_gpu.py): a uint16
surface whose every BYTE is 0xA5 before a call -- samples must be the image afterwards, every other byte must keep 0xA5 --, the view
tuples of its numpy views, and the rules of the call that the GPU tests recompute: the LDS class of a row and the stream passes.  The
layouts are index_views_common.layouts, the frames index16_common.cases()."""
import numpy as np

from tests.index_views_common import (E_INVALID_ARGUMENT, E_INVALID_DIMENSIONS, E_INVALID_INDEX, E_IO, E_UNSUPPORTED, FILL, OK,  # noqa: F401
                                      layouts)

FILL16 = FILL * 0x0101
WIDEST = 16128  # the widest row the 16-bit wave form's LDS holds (include/felics.h)


def filled(shape):
    return np.full(shape, FILL16, np.uint16)


def view_tuple(v, base_ptr, base_addr):
    """the library's view tuple (depth 16) of numpy view v of a uint16 host array at base_addr whose copy lies at base_ptr (the host
    array itself: base_ptr = base_addr)"""
    assert v.dtype == np.uint16
    h, w = v.shape[:2]
    rgb = int(v.ndim == 3)
    if h * w == 0:
        return (0, w, h, rgb, 1, 0, 0, 0)
    off = v.__array_interface__["data"][0] - base_addr
    return (base_ptr + off, w, h, rgb, 1, v.strides[0], v.strides[1], v.strides[2] if rgb else 0)


class Surface:
    """A uint16 host array of 0xA5 bytes and its copy in device memory.  view(f, img) gives the view tuple of f(host) in device memory
    and writes img into the same view of `want`; loose: the samples may hold anything afterwards (a stream that fails while decoding).
    check() compares the WHOLE device surface with `want`."""

    def __init__(self, shape, device=True):
        self.host = filled(shape)
        self.want = self.host.copy()
        self.loose = np.zeros(self.host.shape, bool)
        self.base = self.host.__array_interface__["data"][0]
        self.dev = None
        if device:
            import torch

            self.dev = torch.from_numpy(self.host.view(np.int16)).cuda()  # (torch's uint16 is younger than some of its builds)
            torch.cuda.synchronize()

    def view(self, f, img=None, loose=False):
        from felics_amd import api

        v = f(self.host)
        ptr = self.dev.data_ptr() if self.dev is not None else self.base
        t = view_tuple(v, ptr, self.base)
        if v.size:
            lo, hi = api.view_extent(t)  # the caller's bounds check
            off = t[0] - ptr
            assert off + lo >= 0 and off + hi <= self.host.nbytes, (lo, hi, off)
        if img is not None:
            assert img.shape == v.shape and img.dtype == np.uint16
            f(self.want)[...] = img
        if loose:
            f(self.loose)[...] = True
        return t

    def got(self):
        import torch

        torch.cuda.synchronize()
        return self.dev.cpu().numpy().view(np.uint16)

    def check(self, what=""):
        got = self.got()
        bad = (got != self.want) & ~self.loose
        assert not bad.any(), "%s: %d samples / fill words differ, first at %s" % (what, int(bad.sum()), np.argwhere(bad)[0])


def lds_bytes(w):
    """the dynamic LDS of the 16-bit wave form for a row of w samples (include/felics.h): 512 cached rows of sixteen words,
    their tags, two rows of int32 padded to whole blocks of 64"""
    return 512 * 16 * 4 + 512 * 4 + 2 * ((w + 63) // 64 * 64) * 4


def lds_class(w):
    """which of the call's launches of a pass a row of w samples joins: (16 KB, 32 KB, 64 KB, 160 KB] -> 0 .. 3"""
    return next(c for c, top in enumerate((16 << 10, 32 << 10, 64 << 10, 160 << 10)) if lds_bytes(w) <= top)


def stream_passes(imgs, cap):
    """the stream passes of a call on frames `imgs` (all decodable): consecutive streams whose int32 planes -- 12 bytes per RGB pixel,
    none for gray -- fit `cap` bytes; a single larger stream is a pass of its own.  A list of lists of stream numbers."""
    out, acc = [[]], 0
    for i, im in enumerate(imgs):
        b = 12 * im.shape[0] * im.shape[1] if im.ndim == 3 else 0
        if acc and acc + b > cap:
            out.append([])
            acc = 0
        out[-1].append(i)
        acc += b
    return out


def launches(imgs, items, passes, k):
    """kernel launches of that call: per pass and LDS class that holds an item, ceil(items of the class / k) -- a launch holds at most k
    items because every wave owns a table"""
    n = 0
    for p in passes:
        for c in range(4):
            cnt = sum(items[i] for i in p if lds_class(imgs[i].shape[1]) == c)
            n += (cnt + k - 1) // k
    return n
