"""Indexed decode into views, host side (no GPU): the ABI of felics_decompress_views_device_indexed and its stats, and the host model
felics_decompress_indexed_view -- every shape of index_common.SHAPES, gray and RGB, at both segment sizes, decoded through its
restart index into numpy buffers of every layout, filled with 0xA5 beforehand: the samples must be felics_decompress's, every other
byte must still hold 0xA5; then the model's refusals, each with its code."""
import ctypes as C

import numpy as np
import pytest

from tests import index_common as ic
from tests import index_views_common as vc

SYMBOLS = ("felics_decompress_views_device_indexed", "felics_decompress_indexed_view", "felics_get_index_view_stats")


@pytest.fixture(scope="module")
def api():
    from felics_amd import api as a

    a.lib()
    return a


@pytest.fixture(scope="module")
def cases(oracle, api):
    """(w, h, rgb) -> (image, oracle stream, {segment size: index}): computed once, read by every test"""
    out = {}
    for w, h in ic.SHAPES:
        for rgb in (0, 1):
            im = ic.images(w, h, rgb, 1)[0]
            stream = oracle.compress(im)
            out[(w, h, rgb)] = (im, stream, {seg: api.index_build(stream, seg) for seg in ic.SEGMENTS})
    return out


def _model(api, stream, index, view):
    """felics_decompress_indexed_view on raw bytes and a view tuple: the code"""
    s = np.frombuffer(stream, np.uint8)
    i = np.frombuffer(index, np.uint8)
    cv = api._cview(view)
    return api.lib().felics_decompress_indexed_view(s.ctypes.data if len(s) else None, len(s), i.ctypes.data if len(i) else None, len(i), C.byref(cv), None)


def test_abi_surface(api):
    L = api.lib()
    for name in SYMBOLS:
        assert hasattr(L, name) and name in api.EXPORTS, name
    assert [n for n, _ in api._CIndexViewStats._fields_] == ["streams", "undecoded", "items", "launches", "passes", "plane_bytes"]
    assert C.sizeof(api._CIndexViewStats) == 48
    assert [getattr(api._CIndexViewStats, n).offset for n, _ in api._CIndexViewStats._fields_] == [0, 8, 16, 24, 32, 40]
    assert C.sizeof(api._CIndexStats) == 32  # (felics_index_stats keeps its four fields)
    # NULL is refused before a device is touched, and nothing is written
    offs, lens, st = (C.c_uint64 * 1)(), (C.c_uint64 * 1)(14), (C.c_int * 1)(77)
    vw = (api._CView * 1)(api._cview((16, 4, 4, 0, 0, 4, 1, 0)))
    f = L.felics_decompress_views_device_indexed
    assert f(None, 1, C.c_void_p(16), offs, lens, C.c_void_p(16), offs, lens, vw, None, None, st) == vc.E_INVALID_ARGUMENT and st[0] == 77
    assert f(None, 0, None, None, None, None, None, None, None, None, None, None) == vc.E_INVALID_ARGUMENT
    assert L.felics_decompress_indexed_view(None, 0, None, 0, None, None) == vc.E_INVALID_ARGUMENT
    # the getter refuses NULL and writes nothing then (min(out_size, sizeof) with a context: test_index_views_gpu.py, where one exists)
    stats = api._CIndexViewStats(7, 7, 7, 7, 7, 7)
    assert L.felics_get_index_view_stats(None, C.byref(stats), C.sizeof(stats)) == vc.E_INVALID_ARGUMENT and stats.items == 7
    for name in ("decompress_views_device_indexed", "decompress_arrays_device_indexed", "index_view_stats"):
        assert callable(getattr(api.Encoder, name, None)), name
    assert callable(api.decompress_indexed_view)


def test_every_shape_into_every_layout(api, cases):
    for (w, h, rgb), (img, stream, indexes) in cases.items():
        plain = api.decompress_bytes(stream)
        assert (plain == img).all()
        for seg in ic.SEGMENTS:
            for name, shape, views in vc.layouts(h, w, rgb):
                buf = np.full(shape, vc.FILL, np.uint8)
                want = buf.copy()
                for f in views:
                    got = api.decompress_indexed_view(stream, indexes[seg], f(buf))
                    assert got.shape == img.shape
                    f(want)[...] = plain
                # the samples are felics_decompress's, and every byte that is no sample still holds 0xA5
                assert (buf == want).all(), (w, h, rgb, seg, name, np.argwhere(buf != want)[:1])


def test_refusals_of_the_model(api, cases, oracle):
    for rgb in (0, 1):
        img, stream, indexes = cases[(100, 100, rgb)]
        index = indexes[4096]
        c = (3,) if rgb else ()
        buf = np.full((100, 113) + c, vc.FILL, np.uint8)
        base = buf.__array_interface__["data"][0]
        good = vc.view_tuple(buf[:, :100], base, base)
        assert _model(api, stream, index, good) == vc.OK and (buf[:, :100] == img).all() and (buf[:, 100:] == vc.FILL).all()
        buf[...] = vc.FILL
        # a view whose rows share bytes: felics_view_writable's code, before anything else is looked at
        alias = good[:5] + (50,) + good[6:]
        assert api.view_writable(alias) == vc.E_INVALID_ARGUMENT and _model(api, stream, index, alias) == vc.E_INVALID_ARGUMENT
        assert _model(api, b"", index, alias) == vc.E_INVALID_ARGUMENT
        # another shape, another colour, another depth: nothing written
        for other in (vc.view_tuple(buf[:99, :100], base, base), vc.view_tuple(buf[:, :101], base, base),
                      good[:3] + (1 - rgb,) + good[4:7] + (1 if not rgb else 0,), good[:4] + (1, 226 * (3 if rgb else 1), 2 * (3 if rgb else 1), 2 if rgb else 0)):
            if api.view_writable(other) != vc.OK:
                continue
            assert _model(api, stream, index, other) == vc.E_INVALID_DIMENSIONS, other
        assert (buf == vc.FILL).all()
        # every corruption of the index
        bad = ic.corruptions(index)
        assert ("co_300" in bad) == bool(rgb)
        for name, idx in bad.items():
            assert _model(api, stream, idx, good) == vc.E_INVALID_INDEX, (rgb, name)
        assert _model(api, stream, index[:63], good) == vc.E_INVALID_INDEX and _model(api, stream, b"", good) == vc.E_INVALID_INDEX
        # a truncated stream: felics_decompress's own code where the stream cannot hold what its header claims; where only its
        # last bytes are missing the index no longer names the stream's last byte, and that is the first check to fail
        cut = stream[:len(stream) // 16]
        s = np.frombuffer(cut, np.uint8)
        out = np.zeros(img.size, np.uint8)
        plain_rc = api.lib().felics_decompress(s.ctypes.data, len(s), out.ctypes.data, out.nbytes, None)
        assert plain_rc == vc.E_IO and _model(api, cut, index, good) == plain_rc
        assert _model(api, stream[:-5], index, good) == vc.E_INVALID_INDEX
        for k in (0, 3, 4, 5, 13):  # inside the header: felics_read_header's codes
            s = np.frombuffer(stream[:k], np.uint8)
            hh = api._CHeader()
            assert _model(api, stream[:k], index, good) == api.lib().felics_read_header(s.ctypes.data if k else None, k, C.byref(hh)) != 0
        assert _model(api, b"XLCS" + stream[4:], index, good) == -7
    # a 16-bit stream has no index
    s16 = oracle.compress(np.arange(70 * 70, dtype=np.uint16).reshape(70, 70))
    buf = np.full((70, 70), 0, np.uint16)
    base = buf.__array_interface__["data"][0]
    v16 = (base, 70, 70, 0, 1, 140, 2, 0)
    assert _model(api, s16, cases[(64, 65, 0)][2][4096], v16) == vc.E_UNSUPPORTED and not buf.any()
    # a row too wide for the wave form's LDS: the model refuses what the kernel cannot hold
    wide = np.zeros((1, 90000), np.uint8)
    sw = oracle.compress(wide)
    buf = np.full((1, 90000), vc.FILL, np.uint8)
    base = buf.__array_interface__["data"][0]
    assert _model(api, sw, api.index_build(sw, 4096), vc.view_tuple(buf, base, base)) == vc.E_UNSUPPORTED and (buf == vc.FILL).all()
    # the Python wrapper raises what the code says
    img, stream, indexes = cases[(64, 65, 0)]
    with pytest.raises(api.FelicsError) as ei:
        api.decompress_indexed_view(stream, indexes[4096] + bytes(16), np.zeros((65, 64), np.uint8))
    assert ei.value.code == vc.E_INVALID_INDEX
    ro = np.zeros((65, 64), np.uint8)
    ro.flags.writeable = False
    with pytest.raises(ValueError):
        api.decompress_indexed_view(stream, indexes[4096], ro)
