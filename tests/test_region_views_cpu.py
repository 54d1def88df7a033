"""Regions into views, host side (no GPU): the ABI surface, the host models felics_decompress_region_indexed_view and
felics_decompress_region_indexed16_view against numpy crops of the oracle's decode in every layout of index_views_common -- the samples
are the crop, every other byte of the poisoned buffer keeps its value --, their equality with the dense region models, the refusals
made before a byte is written, and that a corrupted pair gets the same code from the view model as from the dense region model."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import index16_common as ic16
from tests import index16_views_common as vc16
from tests import index_common as ic
from tests import index_views_common as vc
from tests import region_common as rc
from tests import region_views_common as rv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("felics_decompress_region_views_device_indexed", "felics_decompress_region_views_device_indexed_wide",
           "felics_decompress_region_indexed_view", "felics_decompress_region_indexed_view_wide", "felics_get_region_view_stats",
           "felics_get_region_view_wide_stats")


@pytest.fixture(scope="module")
def api():
    from felics_amd import api as a

    a.lib()
    return a


def _model(api, depth16):
    return (api.decompress_region_indexed16_view, api.decompress_region_indexed16) if depth16 else \
        (api.decompress_region_indexed_view, api.decompress_region_indexed)


def _into_layouts(api, stream, index, full, window, depth16):
    """the window into every layout: the samples are the crop of `full`, the rest of the poisoned surface is unchanged; the dense
    region model gives the same samples"""
    view_model, dense_model = _model(api, depth16)
    want_crop = rc.crop(full, window)
    rgb = full.ndim == 3
    dense = dense_model(stream, index, *window)
    assert dense.shape == want_crop.shape and (dense == want_crop).all(), window
    for name, shape, fs in vc.layouts(window[3], window[2], rgb):
        surface = vc16.filled(shape) if depth16 else np.full(shape, vc.FILL, np.uint8)
        want = surface.copy()
        for f in fs:
            f(want)[...] = want_crop
            view_model(stream, index, *window, f(surface))
        assert (surface == want).all(), (name, window)


@pytest.mark.parametrize("w,h", ic.SHAPES)
@pytest.mark.parametrize("rgb", (0, 1))
def test_host_model_8bit(api, oracle, w, h, rgb):
    """every fixed, edge and empty window and two random ones of every shape of index_common"""
    img = ic.images(w, h, rgb, 1)[0]
    stream = oracle.compress(img)
    full = oracle.decompress(stream)
    assert (full == img).all()
    for k, window in enumerate(rc.all_regions(w, h, 2, seed=3)):
        index = api.index_build(stream, ic.SEGMENTS[k % 2])
        _into_layouts(api, stream, index, full, window, False)


@pytest.mark.parametrize("name", list(ic16.cases()))
def test_host_model_16bit(api, oracle, name):
    """the same for every case of index16_common (gray and RGB among them)"""
    img = ic16.cases()[name][0]
    h, w = img.shape[:2]
    stream = oracle.compress(img)
    index = api.index16_build(stream, 4096)
    full = oracle.decompress(stream)
    assert (full == img).all()
    for window in rc.all_regions(w, h, 2, seed=3):
        _into_layouts(api, stream, index, full, window, True)


def test_abi_surface(api, tmp_path):
    """the six symbols are exported and bound, the aliases compile as C and C++, NULL arguments are refused, the getters write
    min(out_size, sizeof) bytes"""
    L = api.lib()
    for name in SYMBOLS:
        assert hasattr(L, name) and name in api.EXPORTS, name
    for name in ("decompress_region_views_device_indexed", "decompress_region_arrays_device_indexed", "decompress_region_views_device_indexed16",
                 "decompress_region_arrays_device_indexed16", "region_view_stats", "region16_view_stats"):
        assert callable(getattr(api.Encoder, name)), name
    assert C.sizeof(api._CRegionViewStats) == 64 and C.sizeof(api._CRegion16ViewStats) == 80
    st = api._CRegionViewStats(*[7] * 8)
    assert L.felics_get_region_view_stats(None, C.byref(st), C.sizeof(st)) == -11 and st.regions == 7
    st16 = api._CRegion16ViewStats(*[7] * 10)
    assert L.felics_get_region_view_wide_stats(None, C.byref(st16), C.sizeof(st16)) == -11 and st16.table_bytes == 7
    for call in (L.felics_decompress_region_views_device_indexed, L.felics_decompress_region_views_device_indexed_wide):
        assert call(None, 1, None, None, None, None, None, None, 1, None, None, None, None, None) == -11
    b = np.zeros(64, np.uint8)
    reg = api._CRegion(0, 0, 0, 1, 1)
    view = api._CView(b.ctypes.data, 1, 1, 0, 0, 1, 1, 0)
    for call in (L.felics_decompress_region_indexed_view, L.felics_decompress_region_indexed_view_wide):
        assert call(b.ctypes.data, 64, b.ctypes.data, 64, None, C.byref(view), None) == -11
        assert call(b.ctypes.data, 64, b.ctypes.data, 64, C.byref(reg), None, None) == -11
        assert call(None, 64, b.ctypes.data, 64, C.byref(reg), C.byref(view), None) == -11
    src = tmp_path / "alias.c"
    src.write_text('#include "felics.h"\n'
                   "int f(felics_ctx *c, const uint8_t *p, const uint64_t *a, const felics_region *r, const felics_view *v, int *st,\n"
                   "      felics_region_view_stats *s, felics_region16_view_stats *t) {\n"
                   "    return felics_decompress_region_views_device_indexed(c, 1, p, a, a, p, a, a, 1, r, v, 0, 0, st)\n"
                   "         + felics_decompress_region_views_device_indexed16(c, 1, p, a, a, p, a, a, 1, r, v, 0, 0, st)\n"
                   "         + felics_decompress_region_indexed_view(p, 1, p, 1, r, v, 0)\n"
                   "         + felics_decompress_region_indexed16_view(p, 1, p, 1, r, v, 0)\n"
                   "         + felics_get_region_view_stats(c, s, sizeof *s) + felics_get_region16_view_stats(c, t, sizeof *t);\n"
                   "}\n")
    for cc, std in (("cc", "-std=c99"), ("c++", "-std=c++11")):
        subprocess.run([cc, std, "-Wall", "-Werror", "-x", "c" if cc == "cc" else "c++", "-c", str(src), "-I", os.path.join(ROOT, "include"),
                        "-o", str(tmp_path / "alias.o")], check=True)


@pytest.mark.parametrize("depth16", (False, True))
def test_refusals_before_a_byte_is_written(api, oracle, depth16):
    """a view that is not writable, a view of another size than the window, a window outside the image (x + w wrapping in 32 bits
    among them), a colour or depth mismatch: the code, and the poisoned buffer as it was"""
    img = ic16.noise(100, 100, 1, 10, 5) if depth16 else ic.images(100, 100, 1, 1)[0]
    gray = img[..., 1].copy()
    dt, sz = (np.uint16, 2) if depth16 else (np.uint8, 1)
    build = api.index16_build if depth16 else api.index_build
    s_rgb, s_gray = oracle.compress(img), oracle.compress(gray)
    i_rgb, i_gray = build(s_rgb, 4096), build(s_gray, 4096)
    buf = vc16.filled((40, 64, 3)) if depth16 else np.full((40, 64, 3), vc.FILL, np.uint8)
    before = buf.copy()
    base = buf.ctypes.data
    d = int(depth16)

    def dense(w, h, rgb, depth=d):
        return (base, w, h, rgb, depth, 64 * 3 * sz, 3 * sz if rgb else sz, sz if rgb else 0)

    def refused(stream, index, window, view, code):
        assert rv.host_call(api, depth16, stream, index, window, view) == code, (window, view)
        assert (buf == before).all()

    ok_view = dense(10, 10, 1)
    alias = (base, 10, 10, 1, d, 0, 3 * sz, sz)  # every row on the first
    assert api.view_writable(ok_view) == 0 and api.view_writable(alias) != 0
    refused(s_rgb, i_rgb, (5, 5, 10, 10), alias, api.view_writable(alias))
    refused(s_rgb, i_rgb, (5, 5, 10, 10), dense(10, 9, 1), rv.E_INVALID_ARGUMENT)
    refused(s_rgb, i_rgb, (5, 5, 10, 10), dense(11, 10, 1), rv.E_INVALID_ARGUMENT)
    for window in ((95, 0, 10, 10), (0, 95, 10, 10), (0xFFFFFFFF, 0, 2, 1), (1, 0, 0xFFFFFFFF, 1), (0, 0xFFFFFFFF, 1, 2)):
        view = dense(min(window[2], 10), min(window[3], 10), 1) if window[2] <= 10 else (base, window[2], 1, 1, d, 0, 0, 0)
        if window[2] > 10:  # (a view that wide is not this buffer's: the model must refuse before it looks at it; any code but OK)
            assert rv.host_call(api, depth16, s_rgb, i_rgb, window, view) != rv.OK and (buf == before).all()
        else:
            refused(s_rgb, i_rgb, window, view, rv.E_INVALID_ARGUMENT)
    refused(s_rgb, i_rgb, (5, 5, 10, 10), dense(10, 10, 0), rv.E_INVALID_DIMENSIONS)        # a gray view of an RGB stream
    refused(s_gray, i_gray, (5, 5, 10, 10), dense(10, 10, 1), rv.E_INVALID_DIMENSIONS)      # an RGB view of a gray stream
    other = (base, 10, 10, 1, 1 - d, 64 * 6, 6, 2)  # the other depth (even strides: writable at either)
    refused(s_rgb, i_rgb, (5, 5, 10, 10), other, rv.E_INVALID_DIMENSIONS)
    # an empty window with a zero-sized view is served: nothing to write
    assert rv.host_call(api, depth16, s_rgb, i_rgb, (100, 100, 0, 0), (0, 0, 0, 1, d, 0, 0, 0)) == rv.OK and (buf == before).all()
    # and the accepted call writes the window
    assert rv.host_call(api, depth16, s_rgb, i_rgb, (5, 5, 10, 10), ok_view) == rv.OK
    assert (buf[:10, :10] == img[5:15, 5:15]).all()
    before[:10, :10] = img[5:15, 5:15]
    assert (buf == before).all()
    assert dt == buf.dtype


def _codes(api, depth16, stream, index, window, rgb):
    """(the view model's code, the dense region model's code) on one pair and window; the view is a dense poisoned buffer"""
    dense_call = api.lib().felics_decompress_region_indexed_wide if depth16 else api.lib().felics_decompress_region_indexed
    s = np.frombuffer(stream, np.uint8)
    i = np.frombuffer(index, np.uint8)
    x, y, w, h = window
    shape = (h, w, 3) if rgb else (h, w)
    out = np.zeros(shape, np.uint16 if depth16 else np.uint8)
    reg = api._CRegion(0, *window)
    dense = dense_call(s.ctypes.data, len(s), i.ctypes.data, len(i), C.byref(reg), out.ctypes.data if out.size else None, out.nbytes, None)
    target = vc16.filled(shape) if depth16 else np.full(shape, vc.FILL, np.uint8)
    code = rv.host_call(api, depth16, stream, index, window, rv.host_view(target, depth16))
    if code != rv.OK and rgb:
        assert (target == (vc16.FILL16 if depth16 else vc.FILL)).all()  # a failing RGB region leaves the view untouched
    if code == rv.OK:
        assert (target == out).all()
    return code, dense


WINDOWS = {"early_0": (10, 10, 5, 5), "end_of_0": (0, 40, 96, 1), "both_01": (90, 40, 10, 2), "in_1": (10, 70, 20, 5), "in_2": (0, 83, 100, 10),
           "full": (0, 0, 100, 100), "empty": (0, 0, 0, 0)}


@pytest.mark.parametrize("depth16", (False, True))
def test_corruption_gets_the_dense_models_code(api, oracle, depth16):
    """100 x 100 RGB cut every 4096 pixels, windows that need every subset of its segments: for a forged bit offset, a forged window
    sample, a forged state row and a truncated stream the view model answers what the dense region model answers -- refused where
    that one refuses, served where it serves"""
    img = ic16.noise(100, 100, 1, 10, 5) if depth16 else ic.images(100, 100, 1, 1)[0]
    stream = oracle.compress(img)
    index = (api.index16_build if depth16 else api.index_build)(stream, 4096)
    if depth16:
        lay = ic16.Layout16(index)
        bad = ic16.corruptions(index)
        row = lay.get(0, 1)[1]
        forged = {"bit offset": bad["bit_offset_plus_1"], "window sample": bad["co_sample_70000"], "state row": bad["contexts_swapped"],
                  "state row counters": index[:row] + bytes([index[row] ^ 0x55]) + index[row + 1:]}
    else:
        lay = ic.Layout(index)
        bad = ic.corruptions(index)
        at = lay.at(0, 1) + 8  # checkpoint (0, 1)'s first state row
        forged = {"bit offset": bad["offset_plus_1"], "window sample": bad["co_300"],
                  "state row": index[:at] + bytes([index[at] ^ 0x55, index[at + 1] ^ 0x2A]) + index[at + 2:]}
    pairs = [(what, stream, b) for what, b in forged.items()]
    pairs += [("truncated stream", stream[:-5], index), ("truncated stream, header only", stream[:9], index),
              ("truncated stream, a sixteenth", stream[:len(stream) // 16], index)]
    refused = 0
    for what, s, b in pairs:
        for name, window in WINDOWS.items():
            code, dense = _codes(api, depth16, s, b, window, True)
            assert code == dense, (what, name, code, dense)
            refused += code != rv.OK
    assert refused >= len(pairs)  # (every forgery is met by a window that needs it)
    # and the intact pair is served for every window
    for name, window in WINDOWS.items():
        assert _codes(api, depth16, stream, index, window, True) == (rv.OK, rv.OK), name
