"""Indexed decode of 16-bit streams into views, host side (no GPU): the ABI of felics_decompress_views_device_indexed16 and its stats,
and the host model felics_decompress_indexed16_view -- every frame of index16_common.cases() decoded through its version-2 index into
uint16 numpy buffers of every layout, every byte 0xA5 beforehand: the samples must be the oracle's decode, every other byte must still
hold 0xA5; then the model's refusals in the order include/felics.h lists them, every corruption of index16_common.corruptions, and
that a failing RGB stream leaves its view untouched."""
import ctypes as C

import numpy as np
import pytest

from tests import index16_common as ic
from tests import index16_views_common as vc

SYMBOLS = ("felics_decompress_views_device_indexed_wide", "felics_decompress_indexed_view_wide", "felics_get_index_view_wide_stats")
FIELDS = ["streams", "undecoded", "items", "launches", "passes", "rows_loaded", "plane_bytes", "table_bytes"]


@pytest.fixture(scope="module")
def api():
    from felics_amd import api as a

    a.lib()
    return a


@pytest.fixture(scope="module")
def cases(oracle, api):
    """name -> (frame, oracle stream, the oracle's decode of it, {segment size: index}): computed once, read by every test"""
    out = {}
    for name, (img, _) in ic.cases().items():
        stream = oracle.compress(img)
        plain = oracle.decompress(stream) if img.size else img
        out[name] = (img, stream, np.asarray(plain).reshape(img.shape), {seg: api.index16_build(stream, seg) for seg in ic.SEGMENTS})
    return out


def _model(api, stream, index, view):
    """felics_decompress_indexed16_view on raw bytes and a view tuple: the code"""
    s = np.frombuffer(stream, np.uint8)
    i = np.frombuffer(index, np.uint8)
    cv = api._cview(view)
    return api.lib().felics_decompress_indexed_view_wide(s.ctypes.data if len(s) else None, len(s), i.ctypes.data if len(i) else None, len(i),
                                                         C.byref(cv), None)


def test_abi_surface(api):
    L = api.lib()
    for name in SYMBOLS:
        assert hasattr(L, name) and name in api.EXPORTS, name
    assert [n for n, _ in api._CIndex16ViewStats._fields_] == FIELDS
    assert C.sizeof(api._CIndex16ViewStats) == 64
    assert [getattr(api._CIndex16ViewStats, n).offset for n in FIELDS] == list(range(0, 64, 8))
    assert C.sizeof(api._CIndexViewStats) == 48 and C.sizeof(api._CIndex16Stats) == 40  # (the neighbours keep their fields)
    # NULL is refused before a device is touched, and nothing is written
    offs, lens, st = (C.c_uint64 * 1)(), (C.c_uint64 * 1)(14), (C.c_int * 1)(77)
    vw = (api._CView * 1)(api._cview((16, 4, 4, 0, 1, 8, 2, 0)))
    f = L.felics_decompress_views_device_indexed_wide
    assert f(None, 1, C.c_void_p(64), offs, lens, C.c_void_p(64), offs, lens, vw, None, None, st) == vc.E_INVALID_ARGUMENT and st[0] == 77
    assert f(None, 0, None, None, None, None, None, None, None, None, None, None) == vc.E_INVALID_ARGUMENT
    assert L.felics_decompress_indexed_view_wide(None, 0, None, 0, None, None) == vc.E_INVALID_ARGUMENT
    stats = api._CIndex16ViewStats(*([7] * 8))
    assert L.felics_get_index_view_wide_stats(None, C.byref(stats), C.sizeof(stats)) == vc.E_INVALID_ARGUMENT and stats.items == 7
    for name in ("decompress_views_device_indexed16", "decompress_arrays_device_indexed16", "index16_view_stats"):
        assert callable(getattr(api.Encoder, name, None)), name
    assert callable(api.decompress_indexed16_view)


def test_every_case_into_every_layout(api, cases, oracle):
    """the samples are the oracle's decode of the stream, every byte that is no sample still holds 0xA5; the segment size rotates from
    layout to layout, the dense layout takes all three"""
    turn = 0
    for name, (img, stream, plain, indexes) in cases.items():
        assert (plain == img).all(), name
        h, w = img.shape[:2]
        for lname, shape, views in vc.layouts(h, w, img.ndim == 3):
            for seg in ic.SEGMENTS if lname == "dense" else (ic.SEGMENTS[turn % 3],):
                buf = vc.filled(shape)
                want = buf.copy()
                for f in views:
                    got = api.decompress_indexed16_view(stream, indexes[seg], f(buf))
                    assert got.shape == img.shape
                    f(want)[...] = plain
                assert (buf == want).all(), (name, seg, lname, np.argwhere(buf != want)[:1])
            turn += 1


def _target(img, pad=13):
    """a pitched buffer of 0xA5 bytes for a frame of img's shape, and the view tuple of the frame's place in it"""
    buf = vc.filled((img.shape[0], img.shape[1] + pad) + img.shape[2:])
    base = buf.__array_interface__["data"][0]
    return buf, base, vc.view_tuple(buf[:, :img.shape[1]], base, base)


def test_refusals_in_order(api, cases, oracle):
    """each code of the per-stream list, and of two that apply the one that stands first in the list"""
    img, stream, _, indexes = cases["100x100"]
    index = indexes[4096]
    buf, base, good = _target(img)
    assert _model(api, stream, index, good) == vc.OK and (buf[:, :100] == img).all() and (buf[:, 100:] == vc.FILL16).all()
    buf[...] = vc.FILL16
    bad_index = ic.corruptions(index)["K"]
    # a view that is not writable comes before anything of the stream: rows that share bytes, an odd stride, an odd address
    for unwritable in (good[:5] + (50,) + good[6:], good[:5] + (227,) + good[6:], (good[0] + 1,) + good[1:]):
        assert api.view_writable(unwritable) == vc.E_INVALID_ARGUMENT
        assert _model(api, stream, index, unwritable) == vc.E_INVALID_ARGUMENT and _model(api, b"", index, unwritable) == vc.E_INVALID_ARGUMENT
    # 1. felics_read_header's codes, in front of everything else (a bad index, another shape)
    other = vc.view_tuple(buf[:99, :100], base, base)
    for k in (0, 3, 4, 5, 13):
        s = np.frombuffer(stream[:k], np.uint8)
        hh = api._CHeader()
        want = api.lib().felics_read_header(s.ctypes.data if k else None, k, C.byref(hh))
        assert want != 0 and _model(api, stream[:k], bad_index, other) == want
    assert _model(api, b"XLCS" + stream[4:], bad_index, other) == -7
    # 2. the header claims more than the stream holds: FELICS_E_IO, in front of a bad index and another shape; where only the last
    #    bytes are missing the index names another last byte
    cut = stream[:len(stream) // 16]
    assert _model(api, cut, index, good) == vc.E_IO and _model(api, cut, bad_index, other) == vc.E_IO
    assert _model(api, stream[:-5], index, good) == vc.E_INVALID_INDEX
    # 3. an 8-bit stream: FELICS_E_UNSUPPORTED, whatever the view (16-bit of its shape, 8-bit of its shape, another shape) and the index
    s8 = oracle.compress(np.arange(100 * 100, dtype=np.uint32).reshape(100, 100).astype(np.uint8))
    view8 = good[:4] + (0,) + good[5:]
    for v in (good, view8, other):
        for ix in (index, api.index_build(s8, 4096)):
            assert _model(api, s8, ix, v) == vc.E_UNSUPPORTED
    # 4. a row wider than the wave form's LDS holds: the model refuses what the kernel cannot hold, in front of a shape mismatch
    wide = np.zeros((1, vc.WIDEST + 1), np.uint16)
    sw = oracle.compress(wide)
    wbuf, wbase, wview = _target(wide, 3)
    iw = api.index16_build(sw, 4096)
    assert _model(api, sw, iw, wview) == vc.E_UNSUPPORTED and _model(api, sw, iw, good) == vc.E_UNSUPPORTED and (wbuf == vc.FILL16).all()
    widest = np.zeros((1, vc.WIDEST), np.uint16)
    swt = oracle.compress(widest)
    tbuf, tbase, tview = _target(widest, 3)
    assert _model(api, swt, api.index16_build(swt, 4096), tview) == vc.OK and not tbuf[:, :vc.WIDEST].any() and (tbuf[:, vc.WIDEST:] == vc.FILL16).all()
    # 5. another shape, colour or depth than the view's: FELICS_E_INVALID_DIMENSIONS in front of a bad index, nothing written
    cbuf, cbase, rgb_view = _target(cases["100x100_rgb"][0])
    for v in (other, vc.view_tuple(buf[:, :101], base, base), view8, rgb_view):
        assert api.view_writable(v) == vc.OK
        assert _model(api, stream, index, v) == vc.E_INVALID_DIMENSIONS and _model(api, stream, bad_index, v) == vc.E_INVALID_DIMENSIONS, v
    assert (cbuf == vc.FILL16).all()
    # 6. idx_len < 64, a header that fails its checks (the index of another stream of the same shape names another last byte or another
    #    length; a version-1 index)
    for ix in (index[:63], b"", index[:64], cases["100x100_rgb"][3][4096], indexes[4096] + bytes(64), api.index_build(s8, 4096)):
        assert _model(api, stream, ix, good) == vc.E_INVALID_INDEX
    assert (buf == vc.FILL16).all()
    # the Python wrapper raises what the code says
    with pytest.raises(api.FelicsError) as ei:
        api.decompress_indexed16_view(stream, index + bytes(64), np.zeros((100, 100), np.uint16))
    assert ei.value.code == vc.E_INVALID_INDEX
    with pytest.raises(api.FelicsError) as ei:
        api.decompress_indexed16_view(s8, index, np.zeros((100, 100), np.uint16))
    assert ei.value.code == vc.E_UNSUPPORTED
    ro = np.zeros((100, 100), np.uint16)
    ro.flags.writeable = False
    with pytest.raises(ValueError):
        api.decompress_indexed16_view(stream, index, ro)


@pytest.mark.parametrize("name", ["100x100", "100x100_rgb"])
def test_corruptions(api, cases, name):
    """every entry of index16_common.corruptions is FELICS_E_INVALID_INDEX; no byte outside the view's samples changes, and an RGB
    stream that fails leaves the view untouched altogether"""
    img, stream, _, indexes = cases[name]
    bad = ic.corruptions(indexes[4096])
    assert ("co_sample_70000" in bad) == (img.ndim == 3)
    for cname, idx in bad.items():
        buf, base, good = _target(img)
        assert _model(api, stream, idx, good) == vc.E_INVALID_INDEX, (name, cname)
        assert (buf[:, 100:] == vc.FILL16).all(), (name, cname)
        if img.ndim == 3:
            assert (buf == vc.FILL16).all(), (name, cname)


def test_rgb_failure_leaves_the_view_untouched(api, cases):
    """failures found with two planes decoded already -- the last plane's last checkpoint a bit off, the stream's last byte missing:
    every byte still 0xA5; and the same buffer then takes the image"""
    img, stream, _, indexes = cases["100x100_rgb"]
    index = indexes[4096]
    lay = ic.Layout16(index)
    last = lay.entry(2, lay.k - 1)
    bit = lay.get(2, lay.k - 1)[0]
    late = bytearray(index)
    late[last:last + 8] = (bit + 1).to_bytes(8, "little")  # the end check of segment (2, K - 2); the walk of (2, K - 1) from a wrong bit
    buf, base, good = _target(img)
    assert _model(api, stream, bytes(late), good) == vc.E_INVALID_INDEX and (buf == vc.FILL16).all()
    assert _model(api, stream[:-1], index, good) == vc.E_INVALID_INDEX and (buf == vc.FILL16).all()  # (the index names another last byte)
    assert _model(api, stream, index, good) == vc.OK and (buf[:, :100] == img).all() and (buf[:, 100:] == vc.FILL16).all()
