"""Mixed-shape decode (felics_decompress_images_device): streams of any shapes, colours and depths decoded in one call.

Every frame must equal its source image (or the oracle decoder's pixels), frames sit at ascending 16-byte aligned offsets, bytes
outside the frames stay untouched, every stream has its own status."""
import ctypes as C
import glob
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
E_BUFFER_TOO_SMALL = -8
E_INVALID_ARGUMENT = -11


def test_mixed_decode_abi_surface():
    """Both symbols are exported and listed; a NULL context, or NULL offsets / lens / status with n > 0, is refused; the Python
    methods exist."""
    from felics_amd import api

    L = api.lib()
    for name in ("felics_read_headers_device", "felics_decompress_images_device"):
        assert hasattr(L, name) and name in api.EXPORTS, name
    offs = (C.c_uint64 * 1)()
    lens = (C.c_uint64 * 1)(14)
    pix = (C.c_uint64 * 1)()
    st = (C.c_int * 1)()
    hd = (api._CHeader * 1)()
    f = L.felics_decompress_images_device
    assert f(None, 1, C.c_void_p(16), offs, lens, C.c_void_p(16), 64, pix, hd, st) == E_INVALID_ARGUMENT
    assert f(None, 0, None, None, None, None, 0, None, None, None) == E_INVALID_ARGUMENT
    assert L.felics_read_headers_device(None, 1, C.c_void_p(16), offs, lens, hd, st) == E_INVALID_ARGUMENT
    assert callable(getattr(api.Encoder, "read_headers_device", None))
    assert callable(getattr(api.Encoder, "decompress_images_device", None))


def _rand(rng, h, w, kind):
    if kind == "gray8":
        return rng.integers(0, 256, size=(h, w), dtype=np.uint8)
    if kind == "rgb8":
        return rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
    if kind == "gray16":
        return rng.integers(0, 65536, size=(h, w), dtype=np.uint16)
    return rng.integers(0, 65536, size=(h, w, 3), dtype=np.uint16)


def _pack(streams):
    import torch

    offs, blob = [], bytearray()
    for i, s in enumerate(streams):
        blob += bytes(i % 3)  # (unaligned offsets too)
        offs.append(len(blob))
        blob += s
    d = torch.from_numpy(np.frombuffer(bytes(blob) + bytes(16), dtype=np.uint8).copy()).cuda()
    return d, offs, [len(s) for s in streams]


def _decode(enc, streams, cap=None, fill=0xA5):
    """One felics_decompress_images_device call: (host bytes of d_pixels, pix_offsets, headers, status, rc)."""
    import torch

    from felics_amd import api

    d, offs, lens = _pack(streams)
    n = len(streams)
    L = api.lib()
    po = np.zeros(max(n, 1), np.uint64)
    st = np.zeros(max(n, 1), np.int32)
    hd = (api._CHeader * max(n, 1))()
    oa, la = np.asarray(offs, np.uint64), np.asarray(lens, np.uint64)
    if cap is None:  # ask for the size with a capacity of 0
        rc = L.felics_decompress_images_device(enc._h, n, d.data_ptr(), oa.ctypes.data_as(C.POINTER(C.c_uint64)),
                                               la.ctypes.data_as(C.POINTER(C.c_uint64)), None, 0, po.ctypes.data_as(C.POINTER(C.c_uint64)),
                                               hd, st.ctypes.data_as(C.POINTER(C.c_int)))
        cap = int(po[0]) if rc == E_BUFFER_TOO_SMALL else 0
    px = torch.full((cap + 64,), fill, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    rc = L.felics_decompress_images_device(enc._h, n, d.data_ptr(), oa.ctypes.data_as(C.POINTER(C.c_uint64)),
                                           la.ctypes.data_as(C.POINTER(C.c_uint64)), px.data_ptr(), cap, po.ctypes.data_as(C.POINTER(C.c_uint64)),
                                           hd, st.ctypes.data_as(C.POINTER(C.c_int)))
    hdrs = [(h.color_type, h.pixel_depth, h.width, h.height) for h in hd[:n]]
    return px.cpu().numpy(), po[:n].copy(), hdrs, st[:n].copy(), rc, cap


def _frame(host, off, img):
    return host[int(off): int(off) + img.nbytes].view(img.dtype).reshape(img.shape)


def _check_frames(host, po, imgs, cap, fill=0xA5):
    """frames equal, offsets ascending and aligned, the fill intact in every gap and behind the end"""
    assert all(int(o) % 16 == 0 for o in po)
    assert all(int(a) <= int(b) for a, b in zip(po, po[1:]))
    used = np.zeros(len(host), bool)
    for o, im in zip(po, imgs):
        if im is None:
            continue
        assert (_frame(host, o, im) == im).all(), im.shape
        used[int(o): int(o) + im.nbytes] = True
    assert (host[~used] == fill).all()


@pytest.fixture(scope="module")
def enc():
    import felics_amd

    e = felics_amd.Encoder(0)
    yield e
    e.close()


def _encode(enc, imgs):
    return enc.compress_images(imgs)


@pytest.mark.gpu
def test_every_small_shape_in_one_call(enc):
    """Every w, h <= 19 in gray8 and RGB8, <= 12 in gray16 and RGB16, 0-wide and 0-high included, shuffled, in ONE call."""
    rng = np.random.default_rng(31)
    imgs = [_rand(rng, h, w, k) for k in ("gray8", "rgb8") for h in range(0, 20) for w in range(0, 20)]
    imgs += [_rand(rng, h, w, k) for k in ("gray16", "rgb16") for h in range(0, 13) for w in range(0, 13)]
    imgs = [imgs[i] for i in rng.permutation(len(imgs))]
    streams = _encode(enc, imgs)
    host, po, hdrs, st, rc, cap = _decode(enc, streams)
    assert rc == 0 and (st == 0).all()
    for h, im in zip(hdrs, imgs):
        assert h == (int(im.ndim == 3), int(im.dtype == np.uint16), im.shape[1], im.shape[0])
    _check_frames(host, po, imgs, cap)


@pytest.mark.gpu
def test_golden_streams_in_one_call(enc, oracle):
    paths = sorted(glob.glob(os.path.join(GOLDEN, "*.felics")) + glob.glob(os.path.join(GOLDEN, "suite", "*.felics")))
    assert len(paths) == 23
    streams = [open(p, "rb").read() for p in paths]
    want = [oracle.decompress(s) for s in streams]
    host, po, hdrs, st, rc, cap = _decode(enc, streams)
    assert rc == 0 and (st == 0).all()
    _check_frames(host, po, want, cap)


@pytest.mark.gpu
def test_corrupt_streams_among_valid_ones(enc, oracle):
    """The corrupt-stream list of the same-shape tests, colour 2, depth 2, < 14 bytes, a 100-byte stream claiming 60000 x 60000:
    valid neighbours exact, header codes as felics_read_header's, a stream the oracle rejects fails, one the GPU accepts equals the
    oracle, the huge claim gets -1 and no room."""
    from felics_amd import api

    rng = np.random.default_rng(8)
    img = rng.integers(0, 256, size=(60, 70), dtype=np.uint8)
    good = oracle.compress(img)
    other = oracle.compress(rng.integers(0, 256, size=(61, 70), dtype=np.uint8))
    huge = good[:6] + (60000).to_bytes(4, "big") + (60000).to_bytes(4, "big") + bytes(86)
    bad = [good[: len(good) // 2], good[:20], b"XLCS" + good[4:], good[:4] + b"\x07" + good[5:], good[:5] + b"\x09" + good[6:],
           good[:30] + b"\xff" * (len(good) - 30), good[:30] + bytes(len(good) - 30), good[:4] + b"\x02" + good[5:],
           good[:5] + b"\x02" + good[6:], good[:9], huge]
    for _ in range(12):
        b = bytearray(good)
        b[int(rng.integers(14, len(b)))] ^= 1 << int(rng.integers(0, 8))
        bad.append(bytes(b))
    streams = [good, other] + bad + [good]
    host, po, hdrs, st, rc, cap = _decode(enc, streams)
    assert rc != 0
    assert st[0] == 0 and st[1] == 0 and st[-1] == 0
    assert (_frame(host, po[0], img) == img).all() and (_frame(host, po[-1], img) == img).all()
    for i, s in enumerate(streams):
        hb = np.frombuffer(s, np.uint8)
        h = api._CHeader()
        hrc = api.lib().felics_read_header(hb.ctypes.data if len(hb) else None, len(hb), C.byref(h))
        if hrc != 0:
            assert st[i] == hrc, (i, st[i], hrc)
        try:
            want = oracle.decompress(s)
        except Exception:
            want = None
        if want is None:
            assert st[i] != 0, i
        elif st[i] == 0:
            assert (_frame(host, po[i], want) == want).all(), i
    k = streams.index(huge)
    assert st[k] == -1
    # the huge claim takes no room: the capacity equals that of the call without it
    _, _, _, _, _, cap2 = _decode(enc, [s for s in streams if s is not huge])
    assert cap == cap2


@pytest.mark.gpu
def test_read_headers_device_matches_the_host(enc, oracle):
    """Every prefix 0..14 of a valid stream and mutations of bytes 0..13: code for code felics_read_header; NULL arrays refused."""
    from felics_amd import api

    rng = np.random.default_rng(3)
    streams = []
    for im in (_rand(rng, 5, 7, "gray8"), _rand(rng, 3, 30, "rgb8"), _rand(rng, 9, 2, "gray16"), _rand(rng, 1, 1, "rgb16")):
        v = oracle.compress(im)
        streams += [v[:k] for k in range(15)]
        for pos in range(14):
            for val in (0, 1, 2, 0x46, 0xFF):
                b = bytearray(v)
                b[pos] = val
                streams += [bytes(b), bytes(b[: pos + 1])]
    d, offs, lens = _pack(streams)
    import torch

    torch.cuda.synchronize()
    hdrs, status = enc.read_headers_device(d.data_ptr(), offs, lens)
    for i, s in enumerate(streams):
        hb = np.frombuffer(s, np.uint8)
        h = api._CHeader()
        rc = api.lib().felics_read_header(hb.ctypes.data if len(hb) else None, len(hb), C.byref(h))
        assert status[i] == rc, i
        if rc == 0:
            assert (hdrs[i].width, hdrs[i].height, int(hdrs[i].color_type), int(hdrs[i].pixel_depth)) == (h.width, h.height, h.color_type, h.pixel_depth)
    oa, la = np.asarray(offs, np.uint64), np.asarray(lens, np.uint64)
    hd = (api._CHeader * 1)()
    st = (C.c_int * 1)()
    f = api.lib().felics_read_headers_device
    P = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint64))  # noqa: E731
    assert f(enc._h, 1, d.data_ptr(), None, P(la), hd, st) == E_INVALID_ARGUMENT
    assert f(enc._h, 1, d.data_ptr(), P(oa), None, hd, st) == E_INVALID_ARGUMENT
    assert f(enc._h, 1, d.data_ptr(), P(oa), P(la), None, st) == E_INVALID_ARGUMENT
    assert f(enc._h, 1, d.data_ptr(), P(oa), P(la), hd, None) == E_INVALID_ARGUMENT


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["0", "1", None])
def test_lane_form_inside_a_mixed_call(enc, form):
    """1 600 gray8 64x40, 200 RGB8 48x24 and 40 odd shapes: exact under FELICS_TEST_DECODE_LANES=0, =1 and the library's choice."""
    from felics_amd import synth

    rng = np.random.default_rng(41)
    imgs = [synth.gray8(64, 40, f % 50, "S1") for f in range(50)]
    imgs = [imgs[f % 50] for f in range(1600)]
    rgb = [_rand(rng, 24, 48, "rgb8") // 4 * 4 for _ in range(20)]
    imgs += [rgb[f % 20] for f in range(200)]
    imgs += [_rand(rng, int(rng.integers(1, 30)), int(rng.integers(1, 90)), ("gray8", "rgb8")[k % 2]) for k in range(40)]
    uniq = {}
    streams = []
    for im in imgs:  # (the same stream referenced many times)
        key = id(im)
        if key not in uniq:
            uniq[key] = _encode(enc, [im])[0]
        streams.append(uniq[key])
    old = os.environ.get("FELICS_TEST_DECODE_LANES")
    if form is not None:
        os.environ["FELICS_TEST_DECODE_LANES"] = form
    try:
        host, po, hdrs, st, rc, cap = _decode(enc, streams)
    finally:
        if old is None:
            os.environ.pop("FELICS_TEST_DECODE_LANES", None)
        else:
            os.environ["FELICS_TEST_DECODE_LANES"] = old
    assert rc == 0 and (st == 0).all()
    _check_frames(host, po, imgs, cap)


@pytest.mark.gpu
def test_host_fallback_rows(enc):
    """A gray8 40 000 x 3 and a gray16 17 000 x 2 stream (rows beyond the LDS) among small ones."""
    rng = np.random.default_rng(51)
    imgs = [_rand(rng, 3, 40000, "gray8"), _rand(rng, 5, 6, "gray8"), _rand(rng, 2, 17000, "gray16"), _rand(rng, 4, 4, "rgb16"),
            _rand(rng, 7, 9, "rgb8")]
    host, po, hdrs, st, rc, cap = _decode(enc, _encode(enc, imgs))
    assert rc == 0 and (st == 0).all()
    _check_frames(host, po, imgs, cap)


@pytest.mark.gpu
def test_capacity(enc):
    """needed - 1: -8, pix_offsets[0] = needed, d_pixels untouched; exactly needed: OK."""
    rng = np.random.default_rng(61)
    imgs = [_rand(rng, 13, 17, "gray8"), _rand(rng, 5, 9, "rgb16"), _rand(rng, 3, 3, "rgb8")]
    streams = _encode(enc, imgs)
    host, po, hdrs, st, rc, need = _decode(enc, streams)
    assert rc == 0
    host2, po2, hdrs2, st2, rc2, _ = _decode(enc, streams, cap=need - 1)
    assert rc2 == E_BUFFER_TOO_SMALL and int(po2[0]) == need and (st2 == E_BUFFER_TOO_SMALL).all()
    assert (host2 == 0xA5).all()
    assert hdrs2 == hdrs


@pytest.mark.gpu
def test_refusal_and_empty_call(enc):
    import torch

    from felics_amd import api

    po, hd, st = enc.decompress_images_device(0, [], [], 0, 0)
    assert len(po) == 0 and hd == [] and len(st) == 0
    frames = torch.zeros((2, 64, 64), dtype=torch.uint8, device="cuda")
    out = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    px = torch.zeros(1 << 14, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    offs, lens = enc.compress_batch_device(frames.data_ptr(), 2, 64, 64, 0, 0, out.data_ptr(), out.numel())
    sub = enc.submit_batch_device(frames.data_ptr(), 2, 64, 64, 0, 0, out.data_ptr() + (1 << 15), 1 << 15)
    try:
        oa, la = np.asarray(offs, np.uint64), np.asarray(lens, np.uint64)
        st = np.zeros(2, np.int32)
        pix = np.zeros(2, np.uint64)
        hd = (api._CHeader * 2)()
        rc = api.lib().felics_decompress_images_device(enc._h, 2, out.data_ptr(), oa.ctypes.data_as(C.POINTER(C.c_uint64)),
                                                       la.ctypes.data_as(C.POINTER(C.c_uint64)), px.data_ptr(), px.numel(),
                                                       pix.ctypes.data_as(C.POINTER(C.c_uint64)), hd, st.ctypes.data_as(C.POINTER(C.c_int)))
        assert rc == E_INVALID_ARGUMENT and (st == E_INVALID_ARGUMENT).all()
        hdrs = (api._CHeader * 2)()
        st[:] = 0
        rc = api.lib().felics_read_headers_device(enc._h, 2, out.data_ptr(), oa.ctypes.data_as(C.POINTER(C.c_uint64)),
                                                  la.ctypes.data_as(C.POINTER(C.c_uint64)), hdrs, st.ctypes.data_as(C.POINTER(C.c_int)))
        assert rc == E_INVALID_ARGUMENT and (st == E_INVALID_ARGUMENT).all()
    finally:
        enc.wait_batch(sub)
    po, hd, st = enc.decompress_images_device(out.data_ptr(), offs, lens, px.data_ptr(), px.numel())
    assert (st == 0).all() and (px[: 64 * 64].cpu().numpy() == 0).all()


@pytest.mark.gpu
def test_random_sweep(enc):
    """300 random shapes and types from a fixed seed: compress_images_device, then one decompress_images_device call."""
    import torch

    rng = np.random.default_rng(71)
    kinds = ("gray8", "rgb8", "gray16", "rgb16")
    imgs = [_rand(rng, int(rng.integers(0, 70)), int(rng.integers(0, 300)), kinds[int(rng.integers(0, 4))]) for _ in range(300)]
    frames = [torch.from_numpy(np.ascontiguousarray(im).view(np.uint8).reshape(-1)).cuda() for im in imgs]
    descs = [(f.data_ptr() if im.size else 0, im.shape[1], im.shape[0], int(im.ndim == 3), int(im.dtype == np.uint16)) for f, im in zip(frames, imgs)]
    cap = sum(im.nbytes * 2 + 96 for im in imgs) + (1 << 16)
    d_out = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    offs, lens = enc.compress_images_device(descs, d_out.data_ptr(), cap)
    need = sum((im.nbytes + 15) // 16 * 16 for im in imgs)
    px = torch.full((need + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    po, hd, st = enc.decompress_images_device(d_out.data_ptr(), offs, lens, px.data_ptr(), need)
    assert (st == 0).all()
    _check_frames(px.cpu().numpy(), po, imgs, need)
