"""Decoding straight into strided device surfaces (felics_decompress_views_device).

Expected pixels are always the numpy image a stream was made from; streams come from the CPU oracle.  Every GPU test builds a host
surface filled with a fixed byte pattern, copies it to the device, decodes into views of it, copies it back and compares the WHOLE
surface with the pattern that has the images written into the views' samples: the samples must be the images, and every other byte
-- alpha bytes, the bytes between a row's end and the pitch, the gaps between the cells of a mosaic -- must still hold the pattern
(the write guarantee of felics.h)."""
import ctypes as C
import os

import numpy as np
import pytest

OK = 0
E_IO = -1
E_INVALID_DIMENSIONS = -4
E_INVALID_ARGUMENT = -11
GRAY, RGB, D8, D16 = 0, 1, 0, 1


# ---------------------------------------------------------------------------------------------------------------- without a GPU

def test_decode_views_abi_surface():
    """The entry points are exported and listed; NULL arguments are refused; felics_decode_view_stats has its five fields; the
    Python methods exist."""
    from felics_amd import api

    L = api.lib()
    for name in ("felics_decompress_views_device", "felics_get_decode_view_stats", "felics_view_writable"):
        assert hasattr(L, name) and name in api.EXPORTS, name
    offs = (C.c_uint64 * 1)()
    lens = (C.c_uint64 * 1)(14)
    st = (C.c_int * 1)(77)
    hd = (api._CHeader * 1)()
    vw = (api._CView * 1)(api._cview((16, 4, 4, GRAY, D8, 4, 1, 0)))
    f = L.felics_decompress_views_device
    assert f(None, 1, C.c_void_p(16), offs, lens, vw, None, hd, st) == E_INVALID_ARGUMENT
    assert f(None, 0, None, None, None, None, None, None, None) == E_INVALID_ARGUMENT
    assert st[0] == 77  # (nothing written)
    stats = api._CDecodeViewStats()
    assert L.felics_get_decode_view_stats(None, C.byref(stats), C.sizeof(stats)) == E_INVALID_ARGUMENT
    assert L.felics_view_writable(None) == E_INVALID_ARGUMENT
    assert [n for n, _ in api._CDecodeViewStats._fields_] == ["views", "dense", "in_place", "scattered", "bytes_staged"]
    assert C.sizeof(api._CDecodeViewStats) == 40
    assert C.sizeof(api._CDecodeStats) == 64  # (felics_decode_stats keeps its eight fields)
    for name in ("decompress_views_device", "decompress_arrays_device", "decode_view_stats"):
        assert callable(getattr(api.Encoder, name, None)), name


def test_aliasing_rule():
    """The nested-strides rule on hand-computed views (felics_view_writable: the check the call makes before it touches anything)."""
    from felics_amd import api

    P = 4096  # (any non-NULL address: nothing is dereferenced)
    accepted = {
        "interleaved": (P, 10, 6, RGB, D8, 30, 3, 1),
        "BGR": (P + 2, 10, 6, RGB, D8, 30, 3, -1),
        "RGBA": (P, 10, 6, RGB, D8, 40, 4, 1),
        "RGBA16": (P, 10, 6, RGB, D16, 80, 8, 2),
        "planar": (P, 10, 6, RGB, D8, 10, 1, 60),
        "planar, pitched": (P, 10, 6, RGB, D8, 16, 1, 6 * 16),
        "bottom-up": (P + 5 * 10, 10, 6, GRAY, D8, -10, 1, 0),
        "crop at pitch 4096": (P + 3 * 4096 + 7, 100, 50, GRAY, D8, 4096, 1, 0),
        "crop at pitch 4096, 16 bit": (P + 3 * 4096 + 6, 100, 50, GRAY, D16, 4096, 2, 0),
        "[::2, ::3]": (P, 10, 6, GRAY, D8, 2 * 64, 3, 0),
        "transposed": (P, 10, 6, GRAY, D8, 1, 6, 0),
        "one pixel, zero strides": (P, 1, 1, GRAY, D8, 0, 0, 0),
        "one row, row stride 0": (P, 10, 1, GRAY, D8, 0, 1, 0),
        "zero-sized, NULL": (0, 0, 5, RGB, D16, 0, 0, 0),
        "zero-high, NULL": (0, 7, 0, GRAY, D8, 0, 0, 0),
    }
    for name, v in accepted.items():
        assert api.view_writable(v) == OK, name
    refused = {
        "row_stride 0, height > 1": (P, 10, 6, GRAY, D8, 0, 1, 0),
        "pixel_stride 0": (P, 10, 6, GRAY, D8, 10, 0, 0),
        "pixel_stride 1 at depth 16": (P, 10, 6, GRAY, D16, 20, 1, 0),
        "pixel_stride 1 at depth 16, one row": (P, 10, 1, GRAY, D16, 20, 1, 0),
        "row_stride < width * pixel_stride": (P, 10, 6, GRAY, D8, 9, 1, 0),
        "row_stride < width * pixel_stride, RGBA": (P, 10, 6, RGB, D8, 39, 4, 1),
        "negative row_stride too short": (P + 5 * 9, 10, 6, GRAY, D8, -9, 1, 0),
        "planar channel stride smaller than a plane": (P, 10, 6, RGB, D8, 10, 1, 59),
        "channel_stride 0": (P, 10, 6, RGB, D8, 30, 3, 0),
        "channels overlap the next pixel": (P, 10, 6, RGB, D8, 20, 2, 1),
        "odd address at depth 16": (P + 1, 10, 6, GRAY, D16, 20, 2, 0),
        "NULL data": (0, 10, 6, GRAY, D8, 10, 1, 0),
    }
    for name, v in refused.items():
        assert api.view_writable(v) == E_INVALID_ARGUMENT, name
    assert api.view_writable((P, 4, 4, 2, D8, 4, 1, 0)) == -5  # (felics_view_extent's own codes: colour, depth)
    assert api.view_writable((P, 4, 4, GRAY, 2, 4, 1, 0)) == -6
    # the encoder's size limit does not apply: 2^16 x 2^15 gray16 pixels is a view the decoder takes (and the encoder does not)
    big = (P, 1 << 16, 1 << 15, GRAY, D16, 2 << 16, 2, 0)
    assert api.view_writable(big) == OK and api.lib().felics_view_extent(C.byref(api._cview(big)), C.byref(C.c_int64()), C.byref(C.c_int64())) == -10


# ---------------------------------------------------------------------------------------------------------------------- helpers

def _rand(rng, h, w, kind):
    """Smooth-ish random content (so that both kinds of code and many contexts appear), full range at the edges."""
    hi = 65536 if kind.endswith("16") else 256
    shape = (h, w, 3) if kind.startswith("rgb") else (h, w)
    a = rng.integers(0, hi, size=shape)
    if h * w:
        a = (a // 8 + rng.integers(0, hi - hi // 8)) % hi if rng.integers(0, 2) else a
    return a.astype(np.uint16 if hi == 65536 else np.uint8)


class Surface:
    """A host array filled with a fixed byte pattern and its copy in device memory.  view(f, img) turns the numpy view f(host) into
    the library's view tuple and writes img into the same view of `want`; check() compares the whole device surface with `want`."""

    def __init__(self, shape, dtype=np.uint8):
        import torch

        self.host = np.empty(shape, dtype)
        b = self.host.reshape(-1).view(np.uint8)
        b[:] = (np.arange(b.size, dtype=np.uint64) * 37 + 11) & 0xFF
        self.want = self.host.copy()
        self.loose = np.zeros(self.host.shape, bool)  # samples of a stream that failed while decoding: written or not
        self.dev = torch.from_numpy(self.host).cuda()
        torch.cuda.synchronize()
        self.base = self.host.__array_interface__["data"][0]

    def view(self, f, img=None, loose=False):
        from felics_amd import api

        v = f(self.host)
        assert v.dtype == self.host.dtype and v.ndim in (2, 3) and (v.ndim == 2 or v.shape[2] == 3)
        color, depth = (RGB if v.ndim == 3 else GRAY), (D16 if v.dtype == np.uint16 else D8)
        h, w = v.shape[:2]
        if h * w == 0:
            return (0, w, h, color, depth, 0, 0, 0)
        off = v.__array_interface__["data"][0] - self.base
        t = (self.dev.data_ptr() + off, w, h, color, depth, v.strides[0], v.strides[1], v.strides[2] if v.ndim == 3 else 0)
        lo, hi = api.view_extent(t)  # the caller's bounds check
        assert off + lo >= 0 and off + hi <= self.host.nbytes, (lo, hi, off)
        if img is not None:
            assert img.shape == v.shape and img.dtype == v.dtype
            f(self.want)[...] = img
        if loose:
            f(self.loose)[...] = True
        return t

    def check(self):
        import torch

        torch.cuda.synchronize()
        got = self.dev.cpu().numpy()
        bad = (got != self.want) & ~self.loose
        assert not bad.any(), "%d samples / pattern bytes differ, first at %s" % (int(bad.sum()), np.argwhere(bad)[0])


def _pack(streams):
    import torch

    offs, blob = [], bytearray()
    for i, s in enumerate(streams):
        blob += bytes(i % 3)  # (unaligned offsets too)
        offs.append(len(blob))
        blob += s
    d = torch.from_numpy(np.frombuffer(bytes(blob) + bytes(16), dtype=np.uint8).copy()).cuda()
    torch.cuda.synchronize()
    return d, np.asarray(offs, np.uint64), np.asarray([len(s) for s in streams], np.uint64)


def _call(enc, d, offs, lens, views, ready_event=None):
    """One felics_decompress_views_device call: (rc, headers as tuples, status)."""
    from felics_amd import api

    n = len(views)
    st = np.full(max(n, 1), 77, np.int32)
    hd = (api._CHeader * max(n, 1))()
    cv = (api._CView * max(n, 1))(*[api._cview(v) for v in views])
    rc = api.lib().felics_decompress_views_device(enc._h, n, d.data_ptr(), offs.ctypes.data_as(C.POINTER(C.c_uint64)),
                                                  lens.ctypes.data_as(C.POINTER(C.c_uint64)), cv, int(ready_event) if ready_event else None,
                                                  hd, st.ctypes.data_as(C.POINTER(C.c_int)))
    return rc, [(h.color_type, h.pixel_depth, h.width, h.height) for h in hd[:n]], st[:n].copy()


def _decode(enc, streams, views):
    d, offs, lens = _pack(streams)
    return _call(enc, d, offs, lens, views)


def _cls(v):
    """The class felics.h gives a view (rows the LDS holds): 'dense', 'in_place' or 'scattered'."""
    _, w, h, color, depth, rs, ps, cs = v
    size, ch = (2 if depth else 1), (3 if color else 1)
    if w * h == 0 or (ps == size * ch and rs == w * ps and (not color or cs == size)):
        return "dense"
    if color or (ps == size and rs >= w * size):
        return "in_place"
    return "scattered"


def _hdr(im):
    return (int(im.ndim == 3), int(im.dtype == np.uint16), im.shape[1], im.shape[0])


class _Env:
    """Sets environment variables the library reads per call and restores them (as tests/test_mixed_decode.py does)."""

    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        for k, v in self.kv.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _delta(after, before):
    return {k: after[k] - before[k] for k in after}


@pytest.fixture(scope="module")
def enc():
    import felics_amd

    e = felics_amd.Encoder(0)
    yield e
    e.close()


# ------------------------------------------------------------------------------------------------------------------- on the GPU

@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["gray8", "gray16"])
def test_wave_form_pitched_gray(enc, oracle, kind):
    """Widths 1 .. 130 (the 64-sample store blocks and a row's masked last block) x heights 1, 2, 5, as crops at odd offsets of two
    surfaces: one of pitch 4096, one where every view's pitch is its width plus one sample.  A wave per stream."""
    rng = np.random.default_rng(101)
    dt = np.uint16 if kind == "gray16" else np.uint8
    size = np.dtype(dt).itemsize
    shapes = [(h, w) for w in (1, 7, 8, 63, 64, 65, 130) for h in (1, 2, 5)]
    wide = Surface((sum(h + 1 for h, _ in shapes) + 2, 4096 // size), dt)
    tight = Surface((sum(h * (w + 1) + 3 for h, w in shapes) + 8,), dt)
    imgs, views = [], []
    y0 = 1
    for k, (h, w) in enumerate(shapes):  # pitch 4096: x0 odd, a row of the pattern between two views
        x0 = 1 + 2 * (k * 37 % 900)
        im = _rand(rng, h, w, kind)
        views.append(wide.view(lambda a, y0=y0, x0=x0, h=h, w=w: a[y0:y0 + h, x0:x0 + w], im))
        imgs.append(im)
        y0 += h + 1
    at = 1
    for h, w in shapes:  # pitch = (W + 1) samples: the view is [:, 1:] of an h x (w + 1) block at an odd offset
        im = _rand(rng, h, w, kind)
        views.append(tight.view(lambda a, at=at, h=h, w=w: a[at:at + h * (w + 1)].reshape(h, w + 1)[:, 1:], im))
        imgs.append(im)
        at += h * (w + 1) + (3 if (h * (w + 1)) % 2 else 2)  # (the next offset odd again)
        assert at % 2 == 1
    streams = [oracle.compress(im) for im in imgs]
    s0, v0 = enc.decode_stats(), enc.decode_view_stats()
    with _Env(FELICS_TEST_DECODE_LANES="0", FELICS_TEST_DECODE16_LANES="0"):
        rc, hdrs, st = _decode(enc, streams, views)
    assert rc == OK and (st == OK).all()
    assert hdrs == [_hdr(im) for im in imgs]
    wide.check()
    tight.check()
    n = len(imgs)
    ds, dv = _delta(enc.decode_stats(), s0), _delta(enc.decode_view_stats(), v0)
    assert ds["streams"] == n and ds["wave16" if size == 2 else "wave8"] == n and ds["undecoded"] == 0
    assert dv == {"views": n, "dense": 0, "in_place": n, "scattered": 0, "bytes_staged": 0}


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["1", "0"])
@pytest.mark.parametrize("kind", ["gray8", "gray16", "rgb8", "rgb16"])
def test_lane_form_mosaic_cells(enc, oracle, kind, form):
    """70 views of one shape as the cells of a mosaic, for W = 8, 9, 10, 11, 13 (every W mod 4 of the four-sample stores) and H = 3
    (the row above at -pitch), in one call: 64 lanes with 64 bases plus a partial group.  form 1: a lane per stream, form 0 (the
    control): a wave per stream."""
    rng = np.random.default_rng(202)
    dt = np.uint16 if kind.endswith("16") else np.uint8
    rgb = kind.startswith("rgb")
    H, per_row, ncell = 3, 10, 70
    surfs, imgs, views = [], [], []
    for W in (8, 9, 10, 11, 13):
        shape = (7 * (H + 1) + 1, per_row * (W + 2) + 1) + ((3,) if rgb else ())
        m = Surface(shape, dt)
        surfs.append(m)
        for c in range(ncell):
            y0, x0 = 1 + (c // per_row) * (H + 1), 1 + (c % per_row) * (W + 2)
            im = _rand(rng, H, W, kind)
            views.append(m.view(lambda a, y0=y0, x0=x0, W=W: a[y0:y0 + H, x0:x0 + W], im))
            imgs.append(im)
    order = rng.permutation(len(imgs))  # (the groups are formed by the library, not by the caller's order)
    imgs, views = [imgs[i] for i in order], [views[i] for i in order]
    streams = [oracle.compress(im) for im in imgs]
    s0, v0 = enc.decode_stats(), enc.decode_view_stats()
    with _Env(FELICS_TEST_DECODE_LANES=form, FELICS_TEST_DECODE16_LANES=form):
        rc, hdrs, st = _decode(enc, streams, views)
    assert rc == OK and (st == OK).all()
    for m in surfs:
        m.check()
    n = len(imgs)
    ds, dv = _delta(enc.decode_stats(), s0), _delta(enc.decode_view_stats(), v0)
    wave, lanes = ("wave16", "lanes16") if dt == np.uint16 else ("wave8", "lanes8")
    if form == "0":
        assert ds[wave] == n and ds[lanes] == 0
    elif dt == np.uint16:  # whole waves only; the rest of a group a wave per stream
        assert ds[lanes] == 5 * 64 and ds[wave] == 5 * 6
    else:
        assert ds[lanes] == n and ds[wave] == 0
    assert dv == {"views": n, "dense": 0, "in_place": n, "scattered": 0, "bytes_staged": 0}


def _rgb_layouts(dt, h, w):
    """(surface shape, view of the surface) for every layout the conversion kernels write."""
    return [
        ("interleaved", (h, w, 3), lambda a: a),
        ("BGR", (h, w, 3), lambda a: a[..., ::-1]),
        ("RGBA", (h, w, 4), lambda a: a[..., :3]),
        ("BGRA", (h, w, 4), lambda a: a[..., 2::-1]),
        ("planar", (3, h, w), lambda a: a.transpose(1, 2, 0)),
        ("bottom-up", (h, w, 3), lambda a: a[::-1]),
        ("crop of a pitched RGBA surface", (h + 3, w + 5, 4), lambda a: a[2:2 + h, 3:3 + w, :3]),
    ]


@pytest.mark.gpu
@pytest.mark.parametrize("lanes", ["0", "1"])
@pytest.mark.parametrize("depth", [8, 16])
def test_rgb_layouts(enc, oracle, depth, lanes):
    """RGB8 / RGB16 through the conversion kernels: seven layouts x 1x1, 5x3, 17x4, 66x2; alpha bytes and pitch gaps keep the pattern."""
    rng = np.random.default_rng(303)
    dt = np.uint16 if depth == 16 else np.uint8
    surfs, imgs, views, names = [], [], [], []
    for w, h in ((1, 1), (5, 3), (17, 4), (66, 2)):
        for name, shape, f in _rgb_layouts(dt, h, w):
            m = Surface(shape, dt)
            im = _rand(rng, h, w, "rgb16" if depth == 16 else "rgb8")
            views.append(m.view(f, im))
            surfs.append(m)
            imgs.append(im)
            names.append((name, w, h))
    v0 = enc.decode_view_stats()
    with _Env(FELICS_TEST_DECODE_LANES=lanes, FELICS_TEST_DECODE16_LANES=lanes):
        rc, hdrs, st = _decode(enc, [oracle.compress(im) for im in imgs], views)
    assert rc == OK and (st == OK).all()
    for m, nm in zip(surfs, names):
        try:
            m.check()
        except AssertionError as e:
            raise AssertionError("%s: %s" % (nm, e))
    dv = _delta(enc.decode_view_stats(), v0)
    dense = sum(_cls(v) == "dense" for v in views)
    assert dense >= 4 and [n for n, v in zip(names, views) if _cls(v) == "scattered"] == []
    assert dv == {"views": 28, "dense": dense, "in_place": 28 - dense, "scattered": 0, "bytes_staged": 0}


@pytest.mark.gpu
@pytest.mark.parametrize("stage_bytes", [None, "600"])
def test_scattered_class(enc, oracle, stage_bytes):
    """gray8 / gray16 [::-1, :], [::2, ::3] and gray as the green channel of an interleaved surface: staged and scattered,
    bytes_staged grows by exactly the frames' bytes.  With FELICS_TEST_VIEW_STAGE_BYTES=600 the same in several passes."""
    rng = np.random.default_rng(404)
    surfs, imgs, views = [], [], []
    for dt, kind in ((np.uint8, "gray8"), (np.uint16, "gray16")):
        for h, w in ((1, 1), (5, 9), (4, 70)):
            for shape, f in (((h + 1, w + 2), lambda a, h=h, w=w: a[h - 1::-1, 1:1 + w]),
                             ((2 * h, 3 * w + 1), lambda a: a[::2, 1::3]),
                             ((h, w, 3), lambda a: a[..., 1])):
                m = Surface(shape, dt)
                im = _rand(rng, h, w, kind)
                views.append(m.view(f, im))
                surfs.append(m)
                imgs.append(im)
    # (a dense and an in-place view between them: the passes cut the call anywhere)
    m = Surface((6, 40), np.uint8)
    for f, hw in ((lambda a: a[0:2, :], (2, 40)), (lambda a: a[3:6, 1:30], (3, 29))):
        im = _rand(rng, hw[0], hw[1], "gray8")
        views.insert(7, m.view(f, im))
        imgs.insert(7, im)
    surfs.append(m)
    s0, v0 = enc.decode_stats(), enc.decode_view_stats()
    with _Env(FELICS_TEST_VIEW_STAGE_BYTES=stage_bytes, FELICS_TEST_DECODE_LANES=None, FELICS_TEST_DECODE16_LANES=None):
        rc, hdrs, st = _decode(enc, [oracle.compress(im) for im in imgs], views)
    assert rc == OK and (st == OK).all()
    assert hdrs == [_hdr(im) for im in imgs]
    for s in surfs:
        s.check()
    ds, dv = _delta(enc.decode_stats(), s0), _delta(enc.decode_view_stats(), v0)
    staged = sum(im.nbytes for im, v in zip(imgs, views) if _cls(v) == "scattered")
    nscat = sum(_cls(v) == "scattered" for v in views)
    assert nscat >= 16  # (a 1 x 1 view's strides may come out as the dense ones)
    assert dv["views"] == len(imgs) and dv["scattered"] == nscat and dv["bytes_staged"] == staged
    assert dv["dense"] == sum(_cls(v) == "dense" for v in views) and dv["in_place"] == sum(_cls(v) == "in_place" for v in views)
    assert ds["streams"] == len(imgs) and ds["wave8"] + ds["wave16"] == len(imgs) and ds["host"] == 0


@pytest.mark.gpu
def test_host_decoder_row_into_a_pitched_view(enc, oracle):
    """A gray8 40 000 x 3 stream (rows beyond the LDS: the host decoder) into a pitched view, a small stream beside it."""
    rng = np.random.default_rng(505)
    m = Surface((5, 40100), np.uint8)
    big, small = _rand(rng, 3, 40000, "gray8"), _rand(rng, 2, 9, "gray8")
    views = [m.view(lambda a: a[1:4, 37:40037], big), m.view(lambda a: a[0:2, 3:12], small)]
    s0, v0 = enc.decode_stats(), enc.decode_view_stats()
    rc, hdrs, st = _decode(enc, [oracle.compress(big), oracle.compress(small)], views)
    assert rc == OK and (st == OK).all()
    m.check()
    ds, dv = _delta(enc.decode_stats(), s0), _delta(enc.decode_view_stats(), v0)
    assert ds["host"] == 1 and ds["wave8"] == 1
    assert dv == {"views": 2, "dense": 0, "in_place": 1, "scattered": 1, "bytes_staged": big.nbytes}


@pytest.mark.gpu
def test_stats_of_a_mixed_call(enc, oracle):
    """Dense, in-place and scattered views of all four types plus a zero-sized one in one call: exact deltas."""
    rng = np.random.default_rng(606)
    surfs, imgs, views = [], [], []
    want = {"views": 0, "dense": 0, "in_place": 0, "scattered": 0, "bytes_staged": 0}
    forms = {"wave8": 0, "wave16": 0}
    for kind, dt in (("gray8", np.uint8), ("rgb8", np.uint8), ("gray16", np.uint16), ("rgb16", np.uint16)):
        c = (3,) if kind.startswith("rgb") else ()
        h, w = 6, 11
        cases = [("dense", (h, w) + c, lambda a: a), ("in_place", (h + 2, w + 3) + c, lambda a: a[1:1 + h, 2:2 + w])]
        if not c:
            cases.append(("scattered", (h, 2 * w), lambda a: a[:, ::2]))
        else:
            cases.append(("in_place", (h, w, 4), lambda a: a[..., 2::-1]))
        for cls, shape, f in cases:
            m = Surface(shape, dt)
            im = _rand(rng, h, w, kind)
            views.append(m.view(f, im))
            surfs.append(m)
            imgs.append(im)
            want["views"] += 1
            want[cls] += 1
            want["bytes_staged"] += im.nbytes if cls == "scattered" else 0
            forms["wave16" if dt == np.uint16 else "wave8"] += 1
    empty = np.zeros((0, 5, 3), np.uint16)
    views.append((0, 5, 0, RGB, D16, 0, 0, 0))
    imgs.append(empty)
    want["views"] += 1
    want["dense"] += 1
    forms["wave16"] += 1
    s0, v0 = enc.decode_stats(), enc.decode_view_stats()
    with _Env(FELICS_TEST_DECODE_LANES=None, FELICS_TEST_DECODE16_LANES=None):
        rc, hdrs, st = _decode(enc, [oracle.compress(im) for im in imgs], views)
    assert rc == OK and (st == OK).all() and hdrs == [_hdr(im) for im in imgs]
    for m in surfs:
        m.check()
    ds, dv = _delta(enc.decode_stats(), s0), _delta(enc.decode_view_stats(), v0)
    assert dv == want
    assert ds["streams"] == len(imgs) and ds["wave8"] == forms["wave8"] and ds["wave16"] == forms["wave16"]
    assert ds["lanes8"] == ds["lanes16"] == ds["host"] == ds["undecoded"] == 0
    # a shorter struct gets its bytes and no more
    from felics_amd import api

    buf = (C.c_uint64 * 5)(*([0xEE] * 5))
    assert api.lib().felics_get_decode_view_stats(enc._h, C.cast(buf, C.POINTER(api._CDecodeViewStats)), 16) == OK
    assert buf[0] == enc.decode_view_stats()["views"] and list(buf[2:]) == [0xEE] * 3


@pytest.mark.gpu
def test_errors_among_valid_streams(enc, oracle):
    """A truncated stream, bit-flipped ones, a bad signature and a valid stream whose view says another width, between valid
    neighbours, in a pitched mosaic: the neighbours are exact, the mismatched view keeps the pattern whole, a stream that failed
    while decoding touched nothing but its own samples, codes as in test_corrupt_streams_among_valid_ones."""
    from felics_amd import api

    rng = np.random.default_rng(707)
    h, w = 20, 31
    img = _rand(rng, h, w, "gray8")
    good = oracle.compress(img)
    wider = _rand(rng, h, w + 1, "gray8")
    rgb = _rand(rng, 6, 7, "rgb8")
    bad = [good[: len(good) // 2], good[:20], b"XLCS" + good[4:], good[:4] + b"\x07" + good[5:], good[:30] + b"\xff" * (len(good) - 30),
           good[:30] + bytes(len(good) - 30), good[:9]]
    for _ in range(6):
        b = bytearray(good)
        b[int(rng.integers(14, len(b)))] ^= 1 << int(rng.integers(0, 8))
        bad.append(bytes(b))
    streams = [good, oracle.compress(rgb)] + bad + [oracle.compress(wider), good]
    n = len(streams)
    m = Surface((n * (h + 1) + 1, w + 9), np.uint8)
    rgba = Surface((6, 7, 4), np.uint8)
    views, accepted = [], {}
    for i, s in enumerate(streams):
        cell = lambda a, i=i: a[1 + i * (h + 1): 1 + i * (h + 1) + h, 3:3 + w]  # noqa: E731
        if i == 1:
            views.append(rgba.view(lambda a: a[..., :3], rgb))
        elif i in (0, n - 1):
            views.append(m.view(cell, img))
        elif i == n - 2:
            views.append(m.view(cell))  # the view says w, the stream w + 1: nothing written
        else:
            try:
                ok = oracle.decompress(s)
            except Exception:
                ok = None
            # a stream that fails while decoding may leave its own samples either way; one the decoder accepts holds the oracle's pixels
            accepted[i] = ok if ok is not None and ok.shape == img.shape else None
            views.append(m.view(cell, accepted[i], loose=True))
    s0 = enc.decode_stats()
    rc, hdrs, st = _decode(enc, streams, views)
    assert rc != OK and rc == next(int(c) for c in st if c != OK)
    assert st[0] == OK and st[1] == OK and st[-1] == OK
    assert st[n - 2] == E_INVALID_DIMENSIONS and hdrs[n - 2] == _hdr(wider)  # (the header the stream has)
    for i, s in enumerate(streams):
        hb = np.frombuffer(s, np.uint8)
        hh = api._CHeader()
        hrc = api.lib().felics_read_header(hb.ctypes.data if len(hb) else None, len(hb), C.byref(hh))
        if hrc != 0:
            assert st[i] == hrc, (i, st[i], hrc)
        if i in range(2, n - 2):
            try:
                oracle.decompress(s)
            except Exception:
                assert st[i] != OK, i
    for i in range(2, n - 2):
        if st[i] == OK:  # (then its samples are not loose: they are the oracle's)
            assert accepted[i] is not None, i
            m.loose[1 + i * (h + 1): 1 + i * (h + 1) + h, 3:3 + w] = False
    m.check()
    rgba.check()
    assert _delta(enc.decode_stats(), s0)["undecoded"] >= 4


@pytest.mark.gpu
def test_refusals(enc, oracle):
    """An aliasing view anywhere in the list: nothing touched, its code in every status.  A call while a ticket is outstanding.  n = 0."""
    import torch

    rng = np.random.default_rng(808)
    m = Surface((12, 40), np.uint8)
    imgs = [_rand(rng, 4, 10, "gray8") for _ in range(3)]
    views = [m.view(lambda a, k=k: a[1 + 5 * (k % 2): 5 + 5 * (k % 2), 2 + 12 * k: 12 + 12 * k]) for k in range(3)]
    alias = list(views)
    alias[2] = alias[2][:5] + (0, 1, 0)  # row_stride = 0 with four rows
    streams = [oracle.compress(im) for im in imgs]
    v0 = enc.decode_view_stats()
    rc, hdrs, st = _decode(enc, streams, alias)
    assert rc == E_INVALID_ARGUMENT and (st == E_INVALID_ARGUMENT).all() and hdrs == [(0, 0, 0, 0)] * 3
    m.check()
    assert enc.decode_view_stats() == v0  # (the call did not pass the checks)
    # while a ticket is outstanding
    frames = torch.zeros((2, 64, 64), dtype=torch.uint8, device="cuda")
    out = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    sub = enc.submit_batch_device(frames.data_ptr(), 2, 64, 64, 0, 0, out.data_ptr(), 1 << 15)
    try:
        rc, hdrs, st = _decode(enc, streams, views)
        assert rc == E_INVALID_ARGUMENT and (st == E_INVALID_ARGUMENT).all()
    finally:
        enc.wait_batch(sub)
    m.check()
    # n = 0
    hd, st = enc.decompress_views_device(0, [], [], [])
    assert hd == [] and len(st) == 0
    # and the same views decode once nothing stands in the way
    for k in range(3):
        m.view(lambda a, k=k: a[1 + 5 * (k % 2): 5 + 5 * (k % 2), 2 + 12 * k: 12 + 12 * k], imgs[k])
    rc, hdrs, st = _decode(enc, streams, views)
    assert rc == OK and (st == OK).all()
    m.check()


@pytest.mark.gpu
def test_ready_event(oracle):
    """As tests/test_views.py::test_ready_event, the other way round: a side stream stalls for tens of milliseconds, then copies the
    streams to the device and writes the pattern over the surfaces; the call gets the event recorded behind that work and no host
    synchronisation.  Had a library stream started early it would have read zeros for streams (a status) or been overwritten by
    the pattern.  (A race test in the one direction that cannot fail falsely; run once.)"""
    import torch

    import felics_amd

    rng = np.random.default_rng(909)
    e = felics_amd.Encoder(0)
    try:
        specs = [("gray8", (40, 300), lambda a: a[3:35, 5:290]), ("rgb8", (30, 64, 4), lambda a: a[..., :3]),
                 ("gray16", (20, 90), lambda a: a[::-1, ::2]), ("rgb16", (3, 12, 33), lambda a: a.transpose(1, 2, 0)),
                 ("gray8", (16, 64), lambda a: a)]
        surfs, imgs, views = [], [], []
        for kind, shape, f in specs:
            m = Surface(shape, np.uint16 if kind.endswith("16") else np.uint8)
            v = f(m.host)
            im = _rand(rng, v.shape[0], v.shape[1], kind)
            views.append(m.view(f, im))
            surfs.append(m)
            imgs.append(im)
        d_final, offs, lens = _pack([oracle.compress(im) for im in imgs])
        d = torch.zeros_like(d_final)
        patterns = [m.dev.clone() for m in surfs]
        for m in surfs:
            m.dev.zero_()
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            big = torch.zeros(1 << 26, dtype=torch.float32, device="cuda")
            for _ in range(600):
                big.add_(1.0)
            d.copy_(d_final, non_blocking=True)
            for m, p in zip(surfs, patterns):
                m.dev.copy_(p, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(side)
        rc, hdrs, st = _call(e, d, offs, lens, views, ready_event=ev.cuda_event)
        assert rc == OK and (st == OK).all(), "a stream was read before the producer had written it"
        for m in surfs:
            m.check()
        del big
    finally:
        e.close()


@pytest.mark.gpu
def test_equal_to_the_mixed_call(enc, oracle):
    """300 random small streams of mixed types, decoded once by felics_decompress_images_device and once into views scattered over
    one surface per sample type: identical samples (and the images)."""
    import torch

    rng = np.random.default_rng(1010)
    kinds = ("gray8", "rgb8", "gray16", "rgb16")
    imgs = [_rand(rng, int(rng.integers(0, 24)), int(rng.integers(0, 80)), kinds[int(rng.integers(0, 4))]) for _ in range(300)]
    streams = [oracle.compress(im) for im in imgs]
    d, offs, lens = _pack(streams)
    need = sum((im.nbytes + 15) // 16 * 16 for im in imgs)
    px = torch.full((need + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    po, hd, st = enc.decompress_images_device(d.data_ptr(), offs, lens, px.data_ptr(), need)
    assert (st == OK).all()
    dense = px.cpu().numpy()
    # the views: bands of 24 rows in four surfaces (gray / RGBA, 8 / 16 bit), every image at its own odd x of its own band
    surf = {k: Surface((24 * 120, 90) + ((4,) if k.startswith("rgb") else ()), np.uint16 if k.endswith("16") else np.uint8) for k in kinds}
    band = dict.fromkeys(kinds, 0)
    views = []
    for im in imgs:
        k = ("rgb" if im.ndim == 3 else "gray") + ("16" if im.dtype == np.uint16 else "8")
        h, w = im.shape[:2]
        y0, x0 = band[k] * 24, 1 + 2 * int(rng.integers(0, 4))
        band[k] += 1
        f = (lambda a, y0=y0, x0=x0, h=h, w=w: a[y0:y0 + h, x0:x0 + w, :3]) if im.ndim == 3 else (lambda a, y0=y0, x0=x0, h=h, w=w: a[y0:y0 + h, x0:x0 + w])
        frame = dense[int(po[len(views)]): int(po[len(views)]) + im.nbytes].view(im.dtype).reshape(im.shape)
        assert (frame == im).all()
        views.append(surf[k].view(f, frame))
    assert max(band.values()) <= 120
    rc, hdrs, st = _call(enc, d, offs, lens, views)
    assert rc == OK and (st == OK).all()
    for s in surf.values():
        s.check()


@pytest.mark.gpu
def test_torch_targets(enc, oracle):
    """decompress_arrays_device into batch[i].permute(1, 2, 0) of an N x 3 x H x W uint8 tensor and into mosaic[y0:y1, x0:x1]."""
    import torch

    rng = np.random.default_rng(1111)
    N, H, W = 5, 12, 20
    rgb = [_rand(rng, H, W, "rgb8") for _ in range(N)]
    cells = [_rand(rng, 9, 14, "gray8") for _ in range(4)]
    batch = torch.full((N, 3, H, W), 0x5A, dtype=torch.uint8, device="cuda")
    mosaic = torch.full((2 * 9 + 3, 2 * 14 + 3), 0x5A, dtype=torch.uint8, device="cuda")
    where = [(1 + (k // 2) * 10, 1 + (k % 2) * 15) for k in range(4)]
    arrays = [batch[i].permute(1, 2, 0) for i in range(N)] + [mosaic[y0:y0 + 9, x0:x0 + 14] for y0, x0 in where]
    imgs = rgb + cells
    d, offs, lens = _pack([oracle.compress(im) for im in imgs])
    hd, st = enc.decompress_arrays_device(d.data_ptr(), offs, lens, arrays)
    assert (st == OK).all()
    assert torch.equal(batch, torch.from_numpy(np.stack([im.transpose(2, 0, 1) for im in rgb])).cuda())
    wm = np.full(tuple(mosaic.shape), 0x5A, np.uint8)
    for (y0, x0), im in zip(where, cells):
        wm[y0:y0 + 9, x0:x0 + 14] = im
    assert torch.equal(mosaic, torch.from_numpy(wm).cuda())
