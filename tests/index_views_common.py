"""What the tests of the indexed views call share (test_index_views_cpu.py, test_index_views_gpu.py): the layouts a target can have,
as numpy views of a surface filled with 0xA5, and the surface itself -- samples must be the image, every other byte must keep 0xA5."""
import numpy as np

OK = 0
E_IO = -1
E_INVALID_DIMENSIONS = -4
E_UNSUPPORTED = -10
E_INVALID_ARGUMENT = -11
E_INVALID_INDEX = -12
FILL = 0xA5


def layouts(h, w, rgb):
    """[(name, shape of the surface, [f]): f(surface) is an h x w (x 3) view of it; the mosaic has four, the others one"""
    c = (3,) if rgb else ()
    out = [
        ("dense", (h, w) + c, [lambda a: a]),
        ("pitched", (h, w + 13) + c, [lambda a: a[:, :w]]),
        ("bottom-up", (h, w) + c, [lambda a: a[::-1]]),
        ("every other column", (h, 2 * w) + c, [lambda a: a[:, ::2]]),
        ("mosaic", (2 * h + 3, 2 * w + 3) + c, [lambda a, y=y, x=x: a[y:y + h, x:x + w] for y in (1, h + 2) for x in (1, w + 2)]),
    ]
    if rgb:
        out += [
            ("RGBA", (h, w, 4), [lambda a: a[..., :3]]),
            ("BGR", (h, w, 3), [lambda a: a[..., ::-1]]),
            ("planar", (3, h, w), [lambda a: a.transpose(1, 2, 0)]),
        ]
    return out


def view_tuple(v, base_ptr, base_addr):
    """the library's view tuple of numpy view v of a host array at base_addr whose copy lies at base_ptr (the host array itself:
    base_ptr = base_addr)"""
    h, w = v.shape[:2]
    rgb = int(v.ndim == 3)
    if h * w == 0:
        return (0, w, h, rgb, 0, 0, 0, 0)
    off = v.__array_interface__["data"][0] - base_addr
    return (base_ptr + off, w, h, rgb, 0, v.strides[0], v.strides[1], v.strides[2] if rgb else 0)


class Surface:
    """A uint8 host array of 0xA5 and its copy in device memory.  view(f, img) gives the view tuple of f(host) in device memory and
    writes img into the same view of `want`; loose: the samples may hold anything afterwards (a stream that fails while decoding).
    check() compares the whole device surface with `want`."""

    def __init__(self, shape):
        import torch

        self.host = np.full(shape, FILL, np.uint8)
        self.want = self.host.copy()
        self.loose = np.zeros(self.host.shape, bool)
        self.dev = torch.from_numpy(self.host).cuda()
        torch.cuda.synchronize()
        self.base = self.host.__array_interface__["data"][0]

    def view(self, f, img=None, loose=False):
        from felics_amd import api

        v = f(self.host)
        t = view_tuple(v, self.dev.data_ptr(), self.base)
        if v.size:
            lo, hi = api.view_extent(t)  # the caller's bounds check
            off = t[0] - self.dev.data_ptr()
            assert off + lo >= 0 and off + hi <= self.host.nbytes, (lo, hi, off)
        if img is not None:
            assert img.shape == v.shape and img.dtype == np.uint8
            f(self.want)[...] = img
        if loose:
            f(self.loose)[...] = True
        return t

    def check(self, what=""):
        import torch

        torch.cuda.synchronize()
        got = self.dev.cpu().numpy()
        bad = (got != self.want) & ~self.loose
        assert not bad.any(), "%s: %d samples / fill bytes differ, first at %s" % (what, int(bad.sum()), np.argwhere(bad)[0])
