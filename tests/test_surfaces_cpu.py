"""Surfaces (felics_submit_surfaces_device and its companions) without a GPU: the ABI surface, felics_surfaces_extent against a
brute-force enumeration of every sample's bytes, the refusals, and surfaces_of_array's strides."""
import ctypes as C
import itertools

import numpy as np
import pytest

OK = 0
E_INVALID_DIMENSIONS = -4
E_INVALID_COLOR_TYPE = -5
E_INVALID_PIXEL_DEPTH = -6
E_UNSUPPORTED = -10
E_INVALID_ARGUMENT = -11
GRAY, RGB, D8, D16 = 0, 1, 0, 1
PTR = 1 << 20  # a stand-in address: never dereferenced


def _extent(view, frame_stride, count):
    from felics_amd import api

    lo, hi = C.c_int64(-1), C.c_int64(-1)
    cs = api._csurfaces((view, frame_stride, count))
    rc = api.lib().felics_surfaces_extent(C.byref(cs), C.byref(lo), C.byref(hi))
    return rc, lo.value, hi.value


def test_surfaces_abi_surface():
    """The entry points are exported and listed, reject NULL arguments, the structs have the C layout and the Python API has the
    methods."""
    from felics_amd import api

    L = api.lib()
    for name in ("felics_surfaces_extent", "felics_submit_surfaces_device", "felics_compress_surfaces_device", "felics_get_surface_stats"):
        assert hasattr(L, name), name
        assert name in api.EXPORTS
    assert C.sizeof(api._CSurfaces) == 64
    assert api._CSurfaces.frame_stride.offset == 48 and api._CSurfaces.count.offset == 56
    assert [n for n, _ in api._CSurfaceStats._fields_] == ["submissions", "queued", "immediate", "frames_in_place", "frames_gathered", "bytes_staged"]
    assert C.sizeof(api._CSurfaceStats) == 48
    assert C.sizeof(api._CViewStats) == 40  # (felics_view_stats did not grow)
    one = api._csurfaces(((PTR, 4, 4, GRAY, D8, 4, 1, 0), 16, 2))
    offs, lens = (C.c_uint64 * 2)(), (C.c_uint64 * 2)()
    out = C.c_void_p(16)
    ticket = C.c_int(-1)
    lo, hi = C.c_int64(), C.c_int64()
    assert L.felics_surfaces_extent(None, C.byref(lo), C.byref(hi)) == E_INVALID_ARGUMENT
    assert L.felics_surfaces_extent(C.byref(one), None, C.byref(hi)) == E_INVALID_ARGUMENT
    assert L.felics_surfaces_extent(C.byref(one), C.byref(lo), None) == E_INVALID_ARGUMENT
    assert L.felics_submit_surfaces_device(None, C.byref(one), None, out, 64, C.byref(ticket)) == E_INVALID_ARGUMENT
    assert L.felics_compress_surfaces_device(None, C.byref(one), None, out, 64, offs, lens) == E_INVALID_ARGUMENT
    st = api._CSurfaceStats(7, 7, 7, 7, 7, 7)
    assert L.felics_get_surface_stats(None, C.byref(st), C.sizeof(st)) == E_INVALID_ARGUMENT
    assert (st.submissions, st.bytes_staged) == (7, 7)
    for name in ("submit_surfaces_device", "compress_surfaces_device", "surface_stats", "wait_batch"):
        assert callable(getattr(api.Encoder, name, None)), name
    assert callable(api.surfaces_extent) and callable(api.surfaces_of_array)


def _brute(w, h, planes, size, rs, ps, cs, fs, n):
    """[lo, hi) of every byte of every sample of every frame, by enumeration."""
    i, y, x, c = np.meshgrid(np.arange(n), np.arange(h), np.arange(w), np.arange(planes), indexing="ij")
    at = i * fs + y * rs + x * ps + c * cs
    return int(at.min()), int(at.max()) + size


@pytest.mark.parametrize("shape", [(1, 1), (7, 3), (17, 33)])
@pytest.mark.parametrize("color,depth", [(GRAY, D8), (RGB, D8), (GRAY, D16), (RGB, D16)])
def test_surfaces_extent_against_enumeration(shape, color, depth):
    """Positive, zero and negative row, pixel, channel and frame strides: the hull equals the enumeration's."""
    w, h = shape
    size, planes = (2 if depth == D16 else 1), (3 if color == RGB else 1)
    px = size * planes
    rows = [w * px, w * px + 10, 0, -(w * px + 6)]
    pixels = [px, 2 * px, 0, -px]
    chans = [size, -size, w * h * size] if planes == 3 else [0]
    frames = [h * w * px + 32, 2 * w * px, 0, -(h * w * px + 8)]
    checked = 0
    for rs, ps, cs, fs, n in itertools.product(rows, pixels, chans, frames, (1, 3)):
        want = _brute(w, h, planes, size, rs, ps, cs, fs, n)
        got = _extent((PTR, w, h, color, depth, rs, ps, cs), fs, n)
        assert got == (OK,) + want, (shape, color, depth, rs, ps, cs, fs, n, got, want)
        checked += 1
    assert checked >= 96
    # no frames, or frames without samples: an empty range
    assert _extent((PTR, w, h, color, depth, rows[1], px, size), frames[0], 0) == (OK, 0, 0)
    assert _extent((0, 0, h, color, depth, rows[1], px, size), frames[0], 5) == (OK, 0, 0)
    assert _extent((0, w, 0, color, depth, rows[1], px, size), frames[0], 5) == (OK, 0, 0)


def test_surfaces_refusals():
    """felics_view_extent's refusals on frame 0, then the frame axis."""
    g8 = (PTR, 4, 4, GRAY, D8, 4, 1, 0)
    g16 = (PTR, 4, 4, GRAY, D16, 8, 2, 0)
    assert _extent(g8, 17, 3)[0] == OK  # depth 8: any frame stride
    assert _extent(g16, 32, 3)[0] == OK
    assert _extent(g16, 33, 3)[0] == E_INVALID_ARGUMENT  # depth 16: an even frame stride ...
    assert _extent(g16, -31, 3)[0] == E_INVALID_ARGUMENT
    assert _extent((PTR + 1, 4, 4, GRAY, D16, 8, 2, 0), 32, 3)[0] == E_INVALID_ARGUMENT  # ... and an even address, as for a view
    assert _extent((PTR, 4, 4, RGB, D16, 24, 6, 1), 96, 3)[0] == E_INVALID_ARGUMENT
    assert _extent((0, 4, 4, GRAY, D8, 4, 1, 0), 16, 3)[0] == E_INVALID_ARGUMENT  # NULL data only for zero-sized frames
    assert _extent((PTR, 4, 4, 2, D8, 4, 1, 0), 16, 3)[0] == E_INVALID_COLOR_TYPE
    assert _extent((PTR, 4, 4, GRAY, 2, 4, 1, 0), 16, 3)[0] == E_INVALID_PIXEL_DEPTH
    assert _extent((PTR, 1 << 31, 2, GRAY, D8, 0, 1, 0), 16, 3)[0] == E_INVALID_DIMENSIONS
    assert _extent((PTR, 1 << 16, 57344, GRAY, D8, 0, 1, 0), 16, 3)[0] == E_UNSUPPORTED
    # an extent beyond 64 bits: along the frame axis alone, in either direction, and where only the sum overflows
    assert _extent(g8, 1 << 62, 3)[0] == E_INVALID_ARGUMENT
    assert _extent(g8, -(1 << 62), 4)[0] == E_INVALID_ARGUMENT
    assert _extent(g8, 1, (1 << 64) - 1)[0] == E_INVALID_ARGUMENT
    assert _extent(g8, (1 << 62) - 8, 3)[0] == E_INVALID_ARGUMENT  # 2^63 - 16 + the frame's 16 bytes = 2^63
    assert _extent(g8, (1 << 62) - 9, 3) == (OK, 0, (1 << 63) - 18 + 16)
    assert _extent((PTR, 4, 4, GRAY, D8, 1 << 61, 1, 0), 1 << 62, 2)[0] == E_INVALID_ARGUMENT
    assert _extent(g8, 0, (1 << 64) - 1) == (OK, 0, 16)  # a zero stride: any count
    # the Python wrapper raises with the code
    from felics_amd import api

    with pytest.raises(api.FelicsError) as ei:
        api.surfaces_extent((g16, 33, 3))
    assert ei.value.code == E_INVALID_ARGUMENT
    assert api.surfaces_extent((g16, 64, 3)) == (0, 2 * 64 + 3 * 8 + 8)


class _Dev:
    """A host array dressed as a device array: surfaces_of_array reads the interface and nothing else."""

    def __init__(self, a):
        self.__cuda_array_interface__ = dict(a.__array_interface__)
        self.a = a


def _base(a):
    return a.__array_interface__["data"][0]


def test_surfaces_of_array_strides():
    from felics_amd import api

    t = np.zeros((5, 40, 64), np.uint8)
    s = t[:, 3:20, 5:40]
    assert api.surfaces_of_array(_Dev(s)) == ((_base(s), 35, 17, GRAY, D8, 64, 1, 0), 40 * 64, 5)
    assert api.surfaces_of_array(_Dev(t)) == ((_base(t), 64, 40, GRAY, D8, 64, 1, 0), 40 * 64, 5)
    t16 = np.zeros((4, 30, 50), np.uint16)
    s = t16[1:4, 2:9, 3:10]
    assert api.surfaces_of_array(_Dev(s)) == ((_base(s), 7, 7, GRAY, D16, 100, 2, 0), 3000, 3)
    s = t16[::-1]
    assert api.surfaces_of_array(_Dev(s)) == ((_base(s), 50, 30, GRAY, D16, 100, 2, 0), -3000, 4)
    rgba = np.zeros((3, 20, 30, 4), np.uint8)
    s = rgba[..., :3]
    assert api.surfaces_of_array(_Dev(s)) == ((_base(s), 30, 20, RGB, D8, 120, 4, 1), 2400, 3)
    rgb = np.zeros((3, 20, 30, 3), np.uint16)
    s = rgb[..., ::-1]
    assert api.surfaces_of_array(_Dev(s)) == ((_base(s), 30, 20, RGB, D16, 180, 6, -2), 3600, 3)
    nchw = np.zeros((6, 3, 20, 30), np.uint8)
    s = nchw.transpose(0, 2, 3, 1)  # torch: nchw.permute(0, 2, 3, 1)
    assert api.surfaces_of_array(_Dev(s)) == ((_base(s), 30, 20, RGB, D8, 30, 1, 600), 1800, 6)
    assert api.surfaces_of_array(_Dev(nchw)) == ((_base(nchw), 30, 20, RGB, D8, 30, 1, 600), 1800, 6)  # N x C x H x W as it is
    one = t[2:3]
    assert api.surfaces_of_array(_Dev(one))[1:] == (0, 1)
    # lists of frames: equally spaced ones are a descriptor, anything else is refused
    assert api.surfaces_of_array([_Dev(t[i, 1:9, 2:8]) for i in (0, 2, 4)]) == ((_base(t[0, 1:9, 2:8]), 6, 8, GRAY, D8, 64, 1, 0), 2 * 40 * 64, 3)
    with pytest.raises(ValueError):
        api.surfaces_of_array([_Dev(t[i, 1:9, 2:8]) for i in (0, 1, 3)])
    with pytest.raises(ValueError):
        api.surfaces_of_array([_Dev(t[0, 1:9, 2:8]), _Dev(t[1, 1:9, 2:9])])
    with pytest.raises(TypeError):
        api.surfaces_of_array(_Dev(np.zeros((4, 4), np.uint8)))
    with pytest.raises(TypeError):
        api.surfaces_of_array(_Dev(np.zeros((2, 4, 4, 2), np.uint8)))
    with pytest.raises(TypeError):
        api.surfaces_of_array(_Dev(np.zeros((2, 4, 4), np.float32)))
    # the extent of what it returns is the array's own hull
    s = t[:, 3:20, 5:40]
    lo, hi = api.surfaces_extent(api.surfaces_of_array(_Dev(s)))
    assert (lo, hi) == (0, 4 * 2560 + 16 * 64 + 35)
