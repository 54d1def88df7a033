"""Views (felics_compress_views_device): device surfaces encoded where they lie -- row pitch, crops, RGBA / BGR / planar layouts,
negative and zero strides -- plus felics_view_extent (the caller's bounds check, host only) and felics_get_view_stats.

The CPU tests check the ABI surface and felics_view_extent on hand-computed cases.  The GPU tests build every view as a numpy
view of a host surface and hand the library the same strides over a device copy of that surface; the expected stream is always the
CPU oracle's of np.ascontiguousarray(view), never this library's."""
import ctypes as C
import io
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
OK = 0
E_INVALID_COLOR_TYPE = -5
E_INVALID_PIXEL_DEPTH = -6
E_INVALID_DIMENSIONS = -4
E_BUFFER_TOO_SMALL = -8
E_UNSUPPORTED = -10
E_INVALID_ARGUMENT = -11
GRAY, RGB, D8, D16 = 0, 1, 0, 1
PTR = 1 << 20  # a stand-in address for the host-only checks: never dereferenced


# ---- without a GPU ----------------------------------------------------------------------------------------------------------

def _extent(view):
    from felics_amd import api

    lo, hi = C.c_int64(-1), C.c_int64(-1)
    v = api._cview(view)
    rc = api.lib().felics_view_extent(C.byref(v), C.byref(lo), C.byref(hi))
    return rc, lo.value, hi.value


def test_views_abi_surface():
    """The three entry points are exported and listed, reject NULL arguments, and the Python API has the methods."""
    from felics_amd import api

    L = api.lib()
    for name in ("felics_compress_views_device", "felics_view_extent", "felics_get_view_stats"):
        assert hasattr(L, name), name
        assert name in api.EXPORTS
    one = (api._CView * 1)(api._CView(None, 0, 0, 0, 0, 0, 0, 0))
    offs, lens = (C.c_uint64 * 1)(), (C.c_uint64 * 1)()
    out = C.c_void_p(16)
    assert L.felics_compress_views_device(None, 1, one, None, out, 64, offs, lens) == E_INVALID_ARGUMENT
    assert L.felics_compress_views_device(None, 1, None, None, out, 64, offs, lens) == E_INVALID_ARGUMENT
    assert L.felics_compress_views_device(None, 1, one, None, None, 64, offs, lens) == E_INVALID_ARGUMENT
    assert L.felics_compress_views_device(None, 1, one, None, out, 64, None, lens) == E_INVALID_ARGUMENT
    assert L.felics_compress_views_device(None, 1, one, None, out, 64, offs, None) == E_INVALID_ARGUMENT
    lo, hi = C.c_int64(), C.c_int64()
    assert L.felics_view_extent(None, C.byref(lo), C.byref(hi)) == E_INVALID_ARGUMENT
    assert L.felics_view_extent(one, None, C.byref(hi)) == E_INVALID_ARGUMENT
    assert L.felics_view_extent(one, C.byref(lo), None) == E_INVALID_ARGUMENT
    st = api._CViewStats()
    assert L.felics_get_view_stats(None, C.byref(st), C.sizeof(st)) == E_INVALID_ARGUMENT
    for name in ("compress_views_device", "compress_arrays_device", "view_stats"):
        assert callable(getattr(api.Encoder, name, None)), name
    assert callable(getattr(api, "view_extent", None))


def test_view_extent_hand_computed():
    """[lo, hi) relative to data: the hull of the samples an encode reads."""
    # a dense gray8 frame, a dense RGB16 frame
    assert _extent((PTR, 640, 360, GRAY, D8, 640, 1, 0)) == (OK, 0, 640 * 360)
    assert _extent((PTR, 100, 50, RGB, D16, 600, 6, 2)) == (OK, 0, 100 * 50 * 6)
    # a 1000 x 700 crop of a gray8 surface at pitch 4096: 699 whole pitches and the last row's 1000 bytes
    assert _extent((PTR + 12345, 1000, 700, GRAY, D8, 4096, 1, 0)) == (OK, 0, 699 * 4096 + 1000)
    # RGBA read as RGB: the last sample is B of the last pixel, the alpha byte behind it is not in the range
    assert _extent((PTR, 1920, 1080, RGB, D8, 1920 * 4, 4, 1)) == (OK, 0, 1079 * 7680 + 1919 * 4 + 3)
    # BGR: data points at R = byte 2 of a pixel, channel_stride -1
    assert _extent((PTR + 2, 10, 4, RGB, D8, 30, 3, -1)) == (OK, -2, 3 * 30 + 9 * 3 + 1)
    # planar C x H x W (torch): channel stride = one plane
    assert _extent((PTR, 64, 32, RGB, D8, 64, 1, 64 * 32)) == (OK, 0, 3 * 64 * 32)
    # bottom-up: data is the first sample of the LAST row in memory
    assert _extent((PTR + 99 * 512, 512, 100, GRAY, D8, -512, 1, 0)) == (OK, -99 * 512, 512)
    # row_stride 0 repeats one row
    assert _extent((PTR, 300, 1000, GRAY, D8, 0, 1, 0)) == (OK, 0, 300)
    # gray16 taken from the green channel of an interleaved RGB16 surface of 200 x 80
    assert _extent((PTR + 2, 200, 80, GRAY, D16, 1200, 6, 0)) == (OK, 0, 79 * 1200 + 199 * 6 + 2)
    # a gray view ignores channel_stride
    assert _extent((PTR, 8, 8, GRAY, D8, 8, 1, 1 << 40)) == (OK, 0, 64)
    # zero-sized views: an empty range, NULL data allowed
    assert _extent((0, 0, 7, GRAY, D8, 0, 1, 0)) == (OK, 0, 0)
    assert _extent((0, 5, 0, RGB, D16, 30, 6, 2)) == (OK, 0, 0)
    assert _extent((PTR, 0, 0, GRAY, D16, 2, 2, 0)) == (OK, 0, 0)


def test_view_refusals():
    """What the encode call refuses, felics_view_extent refuses with the same code."""
    # depth 16: data and every stride even (the channel stride only where it is used)
    assert _extent((PTR + 1, 4, 4, GRAY, D16, 8, 2, 0))[0] == E_INVALID_ARGUMENT
    assert _extent((PTR, 4, 4, GRAY, D16, 9, 2, 0))[0] == E_INVALID_ARGUMENT
    assert _extent((PTR, 4, 4, GRAY, D16, 8, 3, 0))[0] == E_INVALID_ARGUMENT
    assert _extent((PTR, 4, 4, RGB, D16, 24, 6, 1))[0] == E_INVALID_ARGUMENT
    assert _extent((PTR, 4, 4, GRAY, D16, 8, 2, 1))[0] == OK
    assert _extent((PTR + 1, 4, 4, GRAY, D8, 9, 3, 0))[0] == OK  # depth 8: anything goes
    # NULL data only for a zero-sized view
    assert _extent((0, 4, 4, GRAY, D8, 4, 1, 0))[0] == E_INVALID_ARGUMENT
    # enums: felics_compress_images' codes
    assert _extent((PTR, 4, 4, 2, D8, 4, 1, 0))[0] == E_INVALID_COLOR_TYPE
    assert _extent((PTR, 4, 4, GRAY, 2, 4, 1, 0))[0] == E_INVALID_PIXEL_DEPTH
    # sizes: felics_compress_images' limits, whatever the strides (row_stride 0: one row of memory)
    assert _extent((PTR, 1 << 31, 2, GRAY, D8, 0, 1, 0))[0] == E_INVALID_DIMENSIONS       # w * h = 2^32
    assert _extent((PTR, 1 << 16, 57344, GRAY, D8, 0, 1, 0))[0] == E_UNSUPPORTED          # 0xE0000000 samples
    assert _extent((PTR, 1 << 16, 57343, GRAY, D8, 0, 1, 0))[0] == OK
    assert _extent((PTR, 1 << 15, 40000, RGB, D8, 0, 3, 1))[0] == E_UNSUPPORTED           # 3 932 160 000 samples
    assert _extent((PTR, 1 << 15, 38000, RGB, D8, 0, 3, 1))[0] == OK                      # 3 735 552 000
    assert _extent((PTR, 1 << 15, (1 << 14) + 1, GRAY, D16, 0, 2, 0))[0] == E_UNSUPPORTED  # a 16-bit plane of > 2^29 pixels
    assert _extent((PTR, 1 << 15, 1 << 14, GRAY, D16, 0, 2, 0))[0] == OK
    # an extent that does not fit 64 bits
    assert _extent((PTR, 1 << 16, 1 << 15, GRAY, D8, 1 << 62, 1, 0))[0] == E_INVALID_ARGUMENT
    assert _extent((PTR, 1 << 16, 1 << 15, GRAY, D8, -(1 << 62), 1, 0))[0] == E_INVALID_ARGUMENT


def test_view_structs_and_stats_without_a_context():
    """The mirrored structs have the C layout; felics_get_view_stats refuses a NULL context and writes nothing then.  (That it
    never writes more than out_size bytes needs a context: test_views_placement_and_refusal.)"""
    from felics_amd import api

    st = api._CViewStats(7, 7, 7, 7, 7)
    assert api.lib().felics_get_view_stats(None, C.byref(st), C.sizeof(st)) == E_INVALID_ARGUMENT
    assert (st.views, st.dense, st.in_place, st.gathered, st.bytes_staged) == (7, 7, 7, 7, 7)
    assert C.sizeof(api._CViewStats) == 40
    assert [n for n, _ in api._CViewStats._fields_] == ["views", "dense", "in_place", "gathered", "bytes_staged"]
    assert C.sizeof(api._CView) == 48 and api._CView.row_stride.offset == 24


# ---- on the GPU -------------------------------------------------------------------------------------------------------------

def _encoder(**env):
    """A fresh context; FELICS_POISON (and `env`) are read when it is created."""
    import felics_amd

    env = dict(env, FELICS_POISON="1")
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return felics_amd.Encoder(0)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


@pytest.fixture(scope="module")
def enc():
    e = _encoder()
    yield e
    e.close()


class Surface:
    """A host array and its copy in device memory; view(v) turns a numpy view of the host array into the library's view tuple."""

    def __init__(self, host):
        import torch

        self.host = np.ascontiguousarray(host)  # (host itself where it is contiguous: its numpy views are then views of the surface)
        self.dev = torch.from_numpy(self.host).cuda()
        torch.cuda.synchronize()
        self.base = self.host.__array_interface__["data"][0]

    def view(self, v):
        assert v.dtype == self.host.dtype and v.ndim in (2, 3)
        color = RGB if v.ndim == 3 else GRAY
        assert v.ndim == 2 or v.shape[2] == 3
        depth = D16 if v.dtype == np.uint16 else D8
        h, w = v.shape[:2]
        if h * w == 0:
            return (0, w, h, color, depth, 0, 0, 0)
        off = v.__array_interface__["data"][0] - self.base
        ptr = self.dev.data_ptr() + off
        lo_hi = _extent((ptr, w, h, color, depth, v.strides[0], v.strides[1], v.strides[2] if v.ndim == 3 else 0))
        assert lo_hi[0] == OK and off + lo_hi[1] >= 0 and off + lo_hi[2] <= self.host.nbytes, (lo_hi, off)  # the caller's bounds check
        return (ptr, w, h, color, depth, v.strides[0], v.strides[1], v.strides[2] if v.ndim == 3 else 0)


def _cap_for(arrs):
    return sum(a.size * a.itemsize * 5 // 4 + 96 for a in arrs) + 4096


def _encode(e, views, cap, ready_event=None):
    import torch

    out = torch.zeros(max(cap, 16), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    offs, lens = e.compress_views_device(views, out.data_ptr(), cap, ready_event)
    host = out.cpu().numpy()
    return offs, lens, [host[int(o):int(o) + int(n)].tobytes() for o, n in zip(offs, lens)]


def _check(e, pairs, oracle, what="", decode=True, **kw):
    """pairs = [(surface, numpy view), ...]: one call, every stream against the oracle's of the dense copy."""
    import felics_amd

    dense = [np.ascontiguousarray(v) for _, v in pairs]
    _, _, got = _encode(e, [s.view(v) for s, v in pairs], _cap_for(dense), **kw)
    assert len(got) == len(dense)
    for i, (g, img) in enumerate(zip(got, dense)):
        want = oracle.compress(img)
        assert g == want, "%s view %d shape %s %s strides %s: %d vs %d bytes" % (what, i, img.shape, img.dtype, pairs[i][1].strides, len(g), len(want))
        if decode:
            back = felics_amd.decompress_image(io.BytesIO(g))
            assert back.shape == img.shape and (back == img).all(), (what, i, img.shape)
    return got


def _golden(name):
    from PIL import Image

    a = np.ascontiguousarray(np.array(Image.open(os.path.join(GOLDEN, name))))
    return a if a.dtype == np.uint8 else (a >> 8).astype(np.uint8)


def _mosaic(h, w):
    """Golden gray images tiled to h x w."""
    tiles = [t for t in (_golden("suite/boat.tiff"), _golden("man.tiff"), _golden("suite/5.3.01.tiff")) if t.ndim == 2]
    assert tiles
    out = np.zeros((h, w), np.uint8)
    k = 0
    for y in range(0, h, 512):
        for x in range(0, w, 512):
            t = tiles[k % len(tiles)]
            k += 1
            ty, tx = (37 * k) % max(1, t.shape[0] - 511), (53 * k) % max(1, t.shape[1] - 511)
            piece = t[ty:ty + 512, tx:tx + 512]
            ph, pw = min(piece.shape[0], h - y), min(piece.shape[1], w - x)
            out[y:y + ph, x:x + pw] = piece[:ph, :pw]
    return out


@pytest.mark.gpu
def test_crops_of_a_mosaic_in_place(enc, oracle):
    """More than 150 windows of a 2048 x 2048 gray8 mosaic of the golden images (and strips of a wider surface) in one call: every
    width 1..19 at heights 1..3, widths 255 / 256 / 257, 4095-wide strips, windows on every edge, odd and even addresses,
    overlapping windows, one window twice.  All are read in place: nothing is staged."""
    rng = np.random.default_rng(31)
    s = Surface(_mosaic(2048, 2048))
    wide = Surface(_mosaic(40, 4200))
    S, Wd = s.host, wide.host
    pairs = []
    for w in range(1, 20):
        for h in range(1, 4):
            y, x = int(rng.integers(0, 2048 - h)), int(rng.integers(0, 2048 - w))
            pairs.append((s, S[y:y + h, x:x + w]))
    for w in (255, 256, 257):
        for x in (0, 1, 2048 - w):
            pairs.append((s, S[100 + w:100 + w + 33, x:x + w]))
    pairs += [(wide, Wd[0:3, 0:4095]), (wide, Wd[5:12, 105:4200]), (wide, Wd[30:40, 52:4147])]
    # every edge (never the full width: that would be the dense layout), the corners
    pairs += [(s, S[0:300, 0:500]), (s, S[0:7, 1001:2048]), (s, S[1500:2048, 0:333]), (s, S[2047:2048, 1:2048]), (s, S[1800:2048, 1531:2048]),
              (s, S[0:2048, 0:1]), (s, S[0:2048, 2047:2048]), (s, S[1:2047, 777:778 + 64])]
    # overlapping windows, one of them twice
    twice = S[600:1100, 601:1300]
    pairs += [(s, twice), (s, S[700:1200, 650:1250]), (s, twice), (s, S[600:1100, 600:1300])]
    while len(pairs) < 160:
        h, w = int(rng.integers(1, 400)), int(rng.integers(1, 700))
        y, x = int(rng.integers(0, 2048 - h)), int(rng.integers(0, 2048 - w))
        pairs.append((s, S[y:y + h, x:x + w]))
    assert len(pairs) >= 150
    parity = {(su.view(v)[0]) & 1 for su, v in pairs}
    assert parity == {0, 1}
    before = enc.view_stats()
    _check(enc, pairs, oracle, "crops")
    after = enc.view_stats()
    assert after["views"] - before["views"] == len(pairs)
    assert after["in_place"] - before["in_place"] == len(pairs), (before, after)
    assert after["dense"] == before["dense"] and after["gathered"] == before["gathered"]
    assert after["bytes_staged"] == before["bytes_staged"], (before, after)


@pytest.mark.gpu
def test_pitched_4k_frames(enc, oracle):
    """Eight S1 3840 x 2160 frames at pitch 4096: the streams equal the oracle's and those of the dense frames through
    felics_compress_images_device."""
    import torch

    from felics_amd import synth

    frames = [synth.gray8(3840, 2160, f, "S1") for f in range(8)]
    host = np.full((8, 2160, 4096), 0xEE, np.uint8)
    for f in range(8):
        host[f, :, :3840] = frames[f]
    s = Surface(host)
    got = _check(enc, [(s, s.host[f, :, :3840]) for f in range(8)], oracle, "4K", decode=False)
    dense = torch.from_numpy(np.stack(frames)).cuda()
    cap = _cap_for(frames)
    out = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    offs, lens = enc.compress_images_device([(dense[f].data_ptr(), 3840, 2160, GRAY, D8) for f in range(8)], out.data_ptr(), cap)
    h = out.cpu().numpy()
    assert [h[int(o):int(o) + int(n)].tobytes() for o, n in zip(offs, lens)] == got


def _layouts(img, rng):
    """The forms of one dense (H, W, 3) image: [(name, surface array, view of it equal to img)]."""
    H, W = img.shape[:2]
    fill = lambda shape: rng.integers(0, np.iinfo(img.dtype).max, size=shape).astype(img.dtype)  # noqa: E731
    forms = []
    a = fill((H, W, 4))
    a[..., :3] = img
    forms.append(("RGBA", a, a[..., :3]))
    a = fill((H, W, 4))
    a[..., 2::-1] = img
    forms.append(("BGRA", a, a[..., 2::-1]))
    a = np.ascontiguousarray(img[..., ::-1])
    forms.append(("BGR", a, a[..., ::-1]))
    a = np.ascontiguousarray(img.transpose(2, 0, 1))
    forms.append(("planar", a, a.transpose(1, 2, 0)))
    a = fill((3, H, W + 13))
    a[:, :, :W] = img.transpose(2, 0, 1)
    forms.append(("planar pitched", a, a[:, :, :W].transpose(1, 2, 0)))
    a = fill((H + 9, W + 10, 4))
    a[5:5 + H, 3:3 + W, :3] = img
    forms.append(("RGBA crop at odd x", a, a[5:5 + H, 3:3 + W, :3]))
    a = np.ascontiguousarray(img[::-1])
    forms.append(("bottom-up", a, a[::-1]))
    for _, _, v in forms:
        assert (v == img).all()
    return forms


@pytest.mark.gpu
def test_layouts(enc, oracle):
    """RGBA, BGRA, BGR, planar, planar with a row pitch, a crop of an RGBA surface at odd x and bottom-up, RGB8 and RGB16: each
    equals the oracle's stream of the dense image.  Gray taken from the green channel of an interleaved surface is gathered, and
    exactly its frame bytes are staged; row_stride 0 repeats a row."""
    from felics_amd import synth

    rng = np.random.default_rng(41)
    lena = _golden("suite/lena_color_512.tif")
    assert lena.ndim == 3
    for img in (synth.rgb8(331, 207, 3), lena, synth.rgb8(64, 5, 1)):
        for img_d in (img, img.astype(np.uint16) * 257 + (rng.integers(0, 200, size=img.shape).astype(np.uint16) if img is not lena else 0)):
            if img_d.dtype == np.uint16 and img is lena:
                img_d = img_d[100:300, 50:350]  # (a crop keeps the test short)
            want = oracle.compress(np.ascontiguousarray(img_d))
            forms = _layouts(np.ascontiguousarray(img_d), rng)
            before = enc.view_stats()
            pairs = []
            for _, arr, v in forms:  # (arr is contiguous: the surface's host side is arr itself, v a view of it)
                pairs.append((Surface(arr), v))
            got = _check(enc, pairs, oracle, "layouts %s" % (img_d.dtype,))
            for (name, _, _), g in zip(forms, got):
                assert g == want, name
            after = enc.view_stats()
            if img_d.dtype == np.uint8:
                assert after["in_place"] - before["in_place"] == len(forms) and after["bytes_staged"] == before["bytes_staged"], (before, after)
            else:
                assert after["gathered"] - before["gathered"] == len(forms), (before, after)
    # gray from the green channel: gathered, exactly the frame bytes staged
    for dtype in (np.uint8, np.uint16):
        base = synth.rgb8(300, 170, 2).astype(dtype) * (257 if dtype == np.uint16 else 1)
        s = Surface(base)
        before = enc.view_stats()
        _check(enc, [(s, s.host[..., 1])], oracle, "green %s" % dtype)
        after = enc.view_stats()
        assert after["gathered"] - before["gathered"] == 1
        assert after["bytes_staged"] - before["bytes_staged"] == 300 * 170 * np.dtype(dtype).itemsize, (before, after)
    # row_stride 0
    s = Surface(synth.gray8(500, 3, 0, "S2"))
    _check(enc, [(s, np.broadcast_to(s.host[1], (40, 500)))], oracle, "row_stride 0")
    s = Surface(synth.rgb8(100, 2, 0))
    _check(enc, [(s, np.broadcast_to(s.host[1], (9, 100, 3)))], oracle, "row_stride 0 rgb")


def _mixed_pairs(rng):
    """Dense, in-place and gathered views of gray8 / RGB8 / gray16 / RGB16, and zero-sized ones."""
    from felics_amd import synth

    g8 = Surface(synth.gray8(700, 400, 5, "S1"))
    c8 = Surface(np.concatenate([synth.rgb8(320, 200, 4), rng.integers(0, 256, size=(200, 320, 1), dtype=np.uint8)], axis=2))
    g16 = Surface(synth.gray16(260, 150, 6))
    c16 = Surface((synth.rgb8(150, 90, 7).astype(np.uint16) * 251))
    d8 = Surface(synth.gray8(123, 77, 8, "S2"))
    dc = Surface(synth.rgb8(90, 60, 9))
    pairs = [
        (d8, d8.host), (dc, dc.host), (g16, g16.host), (c16, c16.host),                      # dense
        (g8, g8.host[10:390, 33:600]), (g8, g8.host[0:400, 1:2]), (c8, c8.host[..., :3]),    # in place
        (c8, c8.host[7:150, 11:300, 2::-1]), (g8, g8.host[200:201, 5:695]),
        (g8, g8.host[::-1, :]), (g8, g8.host[::2, ::3]), (c8, c8.host[..., 3]),               # gathered: gray8
        (g16, g16.host[5:140, 9:250]), (c16, c16.host[::-1, ::-1, :]), (c16, c16.host[..., 2]),  # gathered: 16 bit
        (g8, g8.host[0:0, 0:5]), (c8, c8.host[0:3, 0:0, :3]), (g16, g16.host[0:0, 0:0]),     # zero-sized
    ]
    return [pairs[i] for i in rng.permutation(len(pairs))]


@pytest.mark.gpu
def test_one_call_of_everything(oracle):
    """Every class of view of every type in one call, permuted, with zero-sized views; then 64 gray8 windows of distinct shapes
    between 500 x 500 and 600 x 600 from one surface, which share at most two submissions."""
    e = _encoder()
    try:
        rng = np.random.default_rng(43)
        pairs = _mixed_pairs(rng)
        before = e.view_stats()
        _check(e, pairs, oracle, "everything")
        after = e.view_stats()
        assert after["views"] - before["views"] == len(pairs)
        assert after["dense"] - before["dense"] == 4 + 3 and after["in_place"] - before["in_place"] == 5 and after["gathered"] - before["gathered"] == 6, after
        s = Surface(_mosaic(1400, 5000) // 8 * 8)
        shapes = set()
        while len(shapes) < 64:
            shapes.add((int(rng.integers(500, 601)), int(rng.integers(500, 601))))
        wins = []
        for k, (h, w) in enumerate(sorted(shapes)):
            y, x = int(rng.integers(0, 1400 - h)), int(rng.integers(0, 5000 - w))
            wins.append((s, s.host[y:y + h, x:x + w]))
        before = e.stats()["submissions"]
        _check(e, wins, oracle, "share", decode=False)
        assert e.stats()["submissions"] - before <= 2, e.stats()
    finally:
        e.close()


@pytest.mark.gpu
@pytest.mark.parametrize("env", ["FELICS_TEST_TILE_CAP", "FELICS_TEST_LOOKBACK_FAIL", "FELICS_TEST_SCATTER_ORDER", "FELICS_TWO_PASS"])
def test_remedies_inside_a_views_call(oracle, env):
    """Each remedy of a sub-batch inside a call of pitched gray8, RGBA and gray16 views, on a fresh context: the streams still
    equal the oracle's, the matching counter moved, and a second call on the context passes as well."""
    from felics_amd import synth

    e = _encoder(**{env: "1"})
    try:
        rng = np.random.default_rng(47)
        g8 = Surface(synth.gray8(900, 500, 1, "S1"))
        c8 = Surface(np.concatenate([synth.rgb8(300, 220, 2), rng.integers(0, 256, size=(220, 300, 1), dtype=np.uint8)], axis=2))
        g16 = Surface(synth.gray16(200, 120, 3))
        pairs = [(g8, g8.host[3 * i:300 + 17 * i, 5 + i:400 + 31 * i]) for i in range(6)]
        pairs += [(c8, c8.host[i:120 + 9 * i, 2 * i:150 + 7 * i, :3]) for i in range(4)]
        pairs += [(g16, g16.host[4:100, 6:180]), (g16, g16.host[::-1, 1:199])]
        staged = e.view_stats()["bytes_staged"]
        _check(e, pairs, oracle, env)
        st = e.stats()
        if env == "FELICS_TEST_TILE_CAP":
            assert st["tile_overflows"] >= 1, st
        elif env == "FELICS_TEST_LOOKBACK_FAIL":
            assert st["lookback_fallbacks"] >= 1, st
        elif env == "FELICS_TEST_SCATTER_ORDER":
            assert st["scatter_fallbacks"] >= 1, st
        else:
            assert st["two_pass"] == 1, st
        # the redone sub-batches wanted dense frames: more than the two 16-bit views was staged
        assert e.view_stats()["bytes_staged"] - staged > sum(v.size * 2 for _, v in pairs[-2:]), e.view_stats()
        _check(e, pairs[::-1], oracle, env + " again")
    finally:
        e.close()


@pytest.mark.gpu
def test_views_placement_and_refusal(enc, oracle):
    """Offsets 16-byte aligned, ascending, non-overlapping; a buffer of exactly the rounded stream sizes still works (exact
    placement), 16 bytes less reports the size needed; refused while a ticket is outstanding."""
    import torch

    from felics_amd import api, synth

    rng = np.random.default_rng(53)
    g8 = Surface(rng.integers(0, 256, size=(300, 400), dtype=np.uint8))
    c8 = Surface(rng.integers(0, 256, size=(200, 300, 4), dtype=np.uint8))
    g16 = Surface(rng.integers(0, 65536, size=(64, 64), dtype=np.uint16))
    low = Surface(rng.integers(0, 40, size=(600, 800), dtype=np.uint8))
    pairs = [(g8, g8.host[5:42, 7:58]), (c8, c8.host[..., :3]), (g16, g16.host), (g8, g8.host[0:0, 0:4]), (low, low.host[20:533, 50:750]),
             (c8, c8.host[1:10, 3:4, 2::-1]), (g8, g8.host[::-3, ::2])]
    dense = [np.ascontiguousarray(v) for _, v in pairs]
    want = [oracle.compress(d) for d in dense]
    views = [s.view(v) for s, v in pairs]
    big = sum(len(w) for w in want) * 2 + 4096 * len(want)
    exact = sum((len(w) + 15) // 16 * 16 for w in want)
    for cap in (big, exact):
        offs, lens, got = _encode(enc, views, cap)
        assert got == want, cap
        assert all(int(o) % 16 == 0 for o in offs)
        for i in range(1, len(offs)):
            assert offs[i] >= offs[i - 1] + lens[i - 1]
    with pytest.raises(api.FelicsError) as ei:
        _encode(enc, views, exact - 16)
    assert ei.value.code == E_BUFFER_TOO_SMALL and ("need %d bytes" % exact) in str(ei.value)

    frames = torch.zeros((2, 64, 64), dtype=torch.uint8, device="cuda")
    out = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    out2 = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    sub = enc.submit_batch_device(frames.data_ptr(), 2, 64, 64, 0, 0, out.data_ptr(), out.numel())
    try:
        with pytest.raises(api.FelicsError) as ei:
            enc.compress_views_device([(frames.data_ptr(), 60, 60, GRAY, D8, 64, 1, 0)], out2.data_ptr(), out2.numel())
        assert ei.value.code == E_INVALID_ARGUMENT
    finally:
        enc.wait_batch(sub)
    # the stats struct: a short out_size leaves the rest of the caller's struct alone
    st = api._CViewStats(7, 7, 7, 7, 7)
    assert api.lib().felics_get_view_stats(enc._h, C.byref(st), 16) == OK
    assert st.views > 7 and (st.in_place, st.gathered, st.bytes_staged) == (7, 7, 7)
    assert api.lib().felics_get_view_stats(enc._h, C.byref(st), 1 << 20) == OK
    assert st.in_place > 7 and st.bytes_staged > 7


def _slow_producer(stream, finals, surfaces):
    """On `stream`: tens of milliseconds of element-wise passes over a large tensor, then the copies that write the frames."""
    import torch

    with torch.cuda.stream(stream):
        big = torch.zeros(1 << 26, dtype=torch.float32, device="cuda")
        for _ in range(600):
            big.add_(1.0)
        for f, s in zip(finals, surfaces):
            s.copy_(f, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(stream)
    return ev, big


@pytest.mark.gpu
def test_ready_event(oracle):
    """The surfaces hold zeros; a producer on a side stream takes tens of milliseconds and writes the frames last; the call gets the
    event recorded behind it and no host synchronisation.  Streams must be those of the final frames.  (A race test in the one
    direction that cannot fail falsely; run once.)"""
    import torch

    from felics_amd import synth

    e = _encoder()
    try:
        rng = np.random.default_rng(59)
        final = [synth.gray8(1024, 600, 1, "S1"), np.concatenate([synth.rgb8(640, 360, 2), np.zeros((360, 640, 1), np.uint8)], axis=2),
                 synth.gray16(300, 200, 3), synth.gray8(333, 222, 4, "S2")]
        for round_ in range(2):
            surfs = [Surface(np.zeros_like(f)) for f in final]
            finals_dev = [torch.from_numpy(f).cuda() for f in final]
            if round_ == 0:  # pitched gray8 alone
                pick = [(0, lambda a: a[3:590, 5:1000])]
            else:  # in place, gathered and dense in one call: every lane and the gather stage wait
                pick = [(0, lambda a: a[3:590, 5:1000]), (1, lambda a: a[..., :3]), (2, lambda a: a[10:190, 20:280]), (0, lambda a: a[::-1, ::2]),
                        (3, lambda a: a), (2, lambda a: a), (1, lambda a: a[5:300, 7:600, 2::-1])]
            views = [surfs[k].view(f(surfs[k].host)) for k, f in pick]
            want = [oracle.compress(np.ascontiguousarray(f(final[k]))) for k, f in pick]
            cap = sum(len(w) for w in want) * 2 + 8192 * len(want)
            out = torch.zeros(cap, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            side = torch.cuda.Stream()
            ev, keep = _slow_producer(side, finals_dev, [s.dev for s in surfs])
            offs, lens = e.compress_views_device(views, out.data_ptr(), cap, ready_event=ev.cuda_event)
            host = out.cpu().numpy()
            got = [host[int(o):int(o) + int(n)].tobytes() for o, n in zip(offs, lens)]
            assert got == want, "round %d: a stream was encoded from a surface the producer had not finished" % round_
            del keep
    finally:
        e.close()


@pytest.mark.gpu
def test_python_arrays(enc, oracle):
    """compress_arrays_device on torch slices, [..., :3] of an RGBA tensor and permute(1, 2, 0) of a C x H x W tensor."""
    import torch

    from felics_amd import synth

    rng = np.random.default_rng(61)
    gray = rng.integers(0, 256, size=(480, 640), dtype=np.uint8) // 4
    rgba = np.concatenate([synth.rgb8(320, 240, 5), rng.integers(0, 256, size=(240, 320, 1), dtype=np.uint8)], axis=2)
    chw = np.ascontiguousarray(synth.rgb8(200, 100, 6).transpose(2, 0, 1))
    t_gray, t_rgba, t_chw = (torch.from_numpy(a).cuda() for a in (gray, rgba, chw))
    arrays = [t_gray[10:400, 33:600], t_rgba[..., :3], t_chw.permute(1, 2, 0), t_gray, t_gray[100:101, :], t_rgba[20:200, 5:300, :3]]
    dense = [gray[10:400, 33:600], rgba[..., :3], chw.transpose(1, 2, 0), gray, gray[100:101, :], rgba[20:200, 5:300, :3]]
    cap = _cap_for(dense)
    out = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    offs, lens = enc.compress_arrays_device(arrays, out.data_ptr(), cap)
    host = out.cpu().numpy()
    for i, d in enumerate(dense):
        assert host[int(offs[i]):int(offs[i]) + int(lens[i])].tobytes() == oracle.compress(np.ascontiguousarray(d)), i


@pytest.mark.gpu
def test_random_views_sweep(enc, oracle):
    """About 30 calls of 1-40 views over three surfaces (gray8, RGBA8, RGB16): random rectangles, channel orders, the occasional
    flip."""
    rng = np.random.default_rng(2025)
    g8 = Surface(_mosaic(1024, 1536))
    lena = _golden("suite/lena_color_512.tif")
    c8 = Surface(np.concatenate([lena, rng.integers(0, 256, size=lena.shape[:2] + (1,), dtype=np.uint8)], axis=2))
    c16 = Surface(lena[:256, :300].astype(np.uint16) * 257 + rng.integers(0, 256, size=(256, 300, 3)).astype(np.uint16))
    for call in range(30):
        pairs = []
        for _ in range(int(rng.integers(1, 41))):
            s = (g8, c8, c16)[int(rng.choice(3, p=[0.5, 0.35, 0.15]))]
            H, W = s.host.shape[:2]
            side = int(rng.choice([4, 40, 400, 1500]))
            h, w = min(H, int(rng.integers(1, side + 1))), min(W, int(rng.integers(1, side + 1)))
            if s is c16:
                h, w = max(1, h // 3), max(1, w // 3)
            y, x = int(rng.integers(0, H - h + 1)), int(rng.integers(0, W - w + 1))
            v = s.host[y:y + h, x:x + w]
            if s is not g8:
                order = int(rng.integers(0, 3))
                v = v[..., :3] if order == 0 else v[..., 2::-1] if order == 1 else v[..., int(rng.integers(0, s.host.shape[2]))]
            if rng.integers(0, 6) == 0:
                v = v[::-1]
            if rng.integers(0, 10) == 0:
                v = v[:, ::-1]
            pairs.append((s, v))
        _check(enc, pairs, oracle, "call %d" % call)
