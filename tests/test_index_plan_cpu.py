"""Indexed encode of views and mixed shapes, host side (no GPU): the ABI of felics_index_plan, felics_compress_views_device_indexed and
felics_get_index_emit_stats, the planner's arithmetic against the format's formula, and what the planner and the GPU entry point
refuse before a device is touched."""
import ctypes as C

import pytest

from tests import index_common as ic

SYMBOLS = ("felics_index_plan", "felics_compress_views_device_indexed", "felics_get_index_emit_stats")
E_BUFFER_TOO_SMALL, E_UNSUPPORTED, E_INVALID_ARGUMENT = -8, -10, -11


@pytest.fixture(scope="module")
def api():
    from felics_amd import api as a

    a.lib()
    return a


def dense(w, h, rgb, depth=0, ptr=4096):
    """the view tuple of a dense frame at a made-up address (nothing here reads it)"""
    size = 2 if depth else 1
    px = size * (3 if rgb else 1)
    return (ptr if w * h else 0, w, h, rgb, depth, w * px, px, size)


def _plan(api, views, segs):
    """felics_index_plan on raw arrays: (rc, offsets, lens, total); the outputs hold 77 where the call wrote nothing"""
    n = len(views)
    cv = (api._CView * max(n, 1))(*[api._cview(v) for v in views])
    sg = (C.c_uint32 * max(n, 1))(*segs)
    offs, lens, total = (C.c_uint64 * max(n, 1))(*[77] * max(n, 1)), (C.c_uint64 * max(n, 1))(*[77] * max(n, 1)), C.c_uint64(77)
    rc = api.lib().felics_index_plan(n, cv, sg, offs, lens, C.byref(total))
    return rc, list(offs)[:n], list(lens)[:n], total.value


def test_abi_surface(api):
    L = api.lib()
    for name in SYMBOLS:
        assert hasattr(L, name) and name in api.EXPORTS, name
    assert [n for n, _ in api._CIndexEmitStats._fields_] == ["indexes", "checkpoints", "in_mixed", "redone"]
    assert C.sizeof(api._CIndexEmitStats) == 32
    for name in ("compress_views_device_indexed", "compress_arrays_device_indexed", "index_emit_stats"):
        assert callable(getattr(api.Encoder, name, None)), name
    assert callable(api.index_plan)
    # the getter refuses NULL and writes nothing then
    stats = api._CIndexEmitStats(7, 7, 7, 7)
    assert L.felics_get_index_emit_stats(None, C.byref(stats), C.sizeof(stats)) == E_INVALID_ARGUMENT and stats.in_mixed == 7


@pytest.mark.parametrize("rgb", (0, 1))
def test_plan_against_the_formula(api, rgb):
    """every shape of index_common.SHAPES (the empty ones: a header alone), segments alternating: the lengths are the format's
    formula, the offsets the running sum of the lengths rounded up to 16"""
    views = [dense(w, h, rgb) for w, h in ic.SHAPES]
    segs = [ic.SEGMENTS[i % 2] for i in range(len(views))]
    offs, lens, total = api.index_plan(views, segs)
    at = 0
    for (w, h), seg, o, ln in zip(ic.SHAPES, segs, offs, lens):
        assert int(ln) == ic.index_size(w, h, rgb, seg) == api.index_size(w, h, rgb, 0, seg), (w, h, seg)
        assert int(o) == at and at % 16 == 0
        at += (int(ln) + 15) // 16 * 16
    assert total == at
    assert all(int(a) < int(b) for a, b in zip(offs, offs[1:]))  # every index has at least its header
    # one segment for all views
    offs1, lens1, total1 = api.index_plan(views, 12288)
    assert [int(v) for v in lens1] == [ic.index_size(w, h, rgb, 12288) for w, h in ic.SHAPES]
    assert total1 == sum((int(v) + 15) // 16 * 16 for v in lens1)
    assert api.index_plan([], 4096)[2] == 0


def test_segment_zero_means_no_index(api):
    views = [dense(100, 100, 0), dense(64, 65, 1), dense(37, 120, 0), dense(64, 65, 0, depth=1), dense(0, 5, 0), dense(130, 70, 1)]
    segs = [4096, 0, 8192, 0, 0, 4096]
    rc, offs, lens, total = _plan(api, views, segs)
    assert rc == 0
    want = [ic.index_size(100, 100, 0, 4096), 0, ic.index_size(37, 120, 0, 8192), 0, 0, ic.index_size(130, 70, 1, 4096)]
    assert lens == want
    at = 0
    for o, ln in zip(offs, lens):
        assert o == at and o % 16 == 0  # (a view without an index: the offset the next index gets, not advanced)
        at += (ln + 15) // 16 * 16
    assert total == at
    assert offs[1] == offs[2] and offs[3] == offs[4] == offs[5]
    # a 37-wide gray checkpoint is 8 + 3072 + 74 bytes, rounded up to 16: lengths are multiples of 16 already, offsets ascend
    assert all(ln % 16 == 0 for ln in lens)


def test_plan_refusals(api):
    good = dense(100, 100, 0)
    for seg in (1, 4095, 4097, 6000, 0xFFFFFFFF):
        assert _plan(api, [good, good], [4096, seg])[0] == E_INVALID_ARGUMENT, seg
        with pytest.raises(api.FelicsError) as ei:
            api.index_plan([good], seg)
        assert ei.value.code == E_INVALID_ARGUMENT
    assert _plan(api, [good, dense(64, 65, 0, depth=1)], [4096, 4096])[0] == E_UNSUPPORTED  # 16-bit streams have no index
    assert _plan(api, [good, dense(64, 65, 1, depth=1)], [4096, 0])[0] == 0
    # a view felics_view_extent refuses: its own code, in view order
    odd16 = (4097, 8, 8, 0, 1, 16, 2, 0)
    lo, hi = C.c_int64(), C.c_int64()
    cv = api._cview(odd16)
    code = api.lib().felics_view_extent(C.byref(cv), C.byref(lo), C.byref(hi))
    assert code != 0
    assert _plan(api, [good, odd16], [4096, 0])[0] == code
    assert _plan(api, [odd16, good], [4096, 6000])[0] == code
    bad_color = (4096, 8, 8, 7, 0, 8, 1, 0)
    assert _plan(api, [bad_color], [4096])[0] == -5
    # NULL arrays
    L = api.lib()
    total = C.c_uint64(0)
    cv1 = (api._CView * 1)(api._cview(good))
    sg, arr = (C.c_uint32 * 1)(4096), (C.c_uint64 * 1)()
    assert L.felics_index_plan(1, None, sg, arr, arr, C.byref(total)) == E_INVALID_ARGUMENT
    assert L.felics_index_plan(1, cv1, None, arr, arr, C.byref(total)) == E_INVALID_ARGUMENT
    assert L.felics_index_plan(1, cv1, sg, None, arr, C.byref(total)) == E_INVALID_ARGUMENT
    assert L.felics_index_plan(1, cv1, sg, arr, None, C.byref(total)) == E_INVALID_ARGUMENT
    assert L.felics_index_plan(1, cv1, sg, arr, arr, None) == E_INVALID_ARGUMENT
    assert L.felics_index_plan(0, None, None, None, None, C.byref(total)) == 0 and total.value == 0


def test_gpu_entry_point_refuses_null_without_a_device(api):
    f = api.lib().felics_compress_views_device_indexed
    cv = (api._CView * 1)(api._cview(dense(100, 100, 0)))
    sg, io = (C.c_uint32 * 1)(4096), (C.c_uint64 * 1)(0)
    offs, lens = (C.c_uint64 * 1)(77), (C.c_uint64 * 1)(77)
    out, idx = C.c_void_p(4096), C.c_void_p(8192)
    assert f(None, 1, cv, sg, None, out, 1 << 20, idx, 1 << 20, io, offs, lens) == E_INVALID_ARGUMENT
    assert f(None, 0, None, None, None, None, 0, None, 0, None, None, None) == E_INVALID_ARGUMENT
    assert f(None, 1, None, sg, None, out, 1 << 20, idx, 1 << 20, io, offs, lens) == E_INVALID_ARGUMENT
    assert f(None, 1, cv, None, None, out, 1 << 20, idx, 1 << 20, None, None, None) == E_INVALID_ARGUMENT
    # (with a context the NULL arrays are refused in the same first check: test_index_views_encode_gpu.py, where one exists)
    assert offs[0] == 77 and lens[0] == 77
