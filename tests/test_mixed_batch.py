"""Mixed-shape batches (felics_compress_images / felics_compress_images_device): images of any shapes and types in one call.

Every stream must equal the CPU oracle's for that image alone and decode back.  The CPU test checks the ABI surface; the GPU
tests cover tiny and odd shapes, the golden corpus, the remedies inside a mixed call, placement in device memory, and that
8-bit images of different shapes really share submissions."""
import ctypes as C
import hashlib
import io
import json
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
E_BUFFER_TOO_SMALL = -8
E_INVALID_ARGUMENT = -11


def test_mixed_abi_surface():
    """Both entry points are exported, reject a NULL context and NULL images, and the Python API has the methods."""
    from felics_amd import api

    L = api.lib()
    for name in ("felics_compress_images", "felics_compress_images_device"):
        assert hasattr(L, name), name
        assert name in api.EXPORTS
    one = (api._CImage * 1)(api._CImage(None, 0, 0, 0, 0))
    outs = (C.c_void_p * 1)()
    caps = (C.c_size_t * 1)(64)
    lens = (C.c_size_t * 1)()
    assert L.felics_compress_images(None, 1, one, outs, caps, lens) == E_INVALID_ARGUMENT
    assert L.felics_compress_images(None, 1, None, outs, caps, lens) == E_INVALID_ARGUMENT
    offs = (C.c_uint64 * 1)()
    dl = (C.c_uint64 * 1)()
    assert L.felics_compress_images_device(None, 1, one, C.c_void_p(16), 64, offs, dl) == E_INVALID_ARGUMENT
    assert L.felics_compress_images_device(None, 1, None, C.c_void_p(16), 64, offs, dl) == E_INVALID_ARGUMENT
    assert callable(getattr(api.Encoder, "compress_images", None))
    assert callable(getattr(api.Encoder, "compress_images_device", None))


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


def _check_all(got, imgs, oracle, what=""):
    import felics_amd

    assert len(got) == len(imgs)
    for i, (g, img) in enumerate(zip(got, imgs)):
        want = oracle.compress(img)
        assert g == want, "%s image %d shape %s %s: %d vs %d bytes" % (what, i, img.shape, img.dtype, len(g), len(want))
        back = felics_amd.decompress_image(io.BytesIO(g))
        assert back.shape == img.shape and (back == img).all(), (what, i, img.shape)


def _rand(rng, h, w, kind):
    if kind == "gray8":
        return rng.integers(0, 256, size=(h, w), dtype=np.uint8)
    if kind == "rgb8":
        return rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
    if kind == "gray16":
        return rng.integers(0, 65536, size=(h, w), dtype=np.uint16)
    return rng.integers(0, 65536, size=(h, w, 3), dtype=np.uint16)


@pytest.mark.gpu
def test_every_tiny_shape_in_one_call(enc, oracle):
    """Every (w, h) with 1 <= w, h <= 19, gray8 and RGB8 random content: all 722 images in one call."""
    rng = np.random.default_rng(5)
    imgs = [_rand(rng, h, w, kind) for kind in ("gray8", "rgb8") for h in range(1, 20) for w in range(1, 20)]
    assert len(imgs) == 722
    _check_all(enc.compress_images(imgs), imgs, oracle, "tiny")


@pytest.mark.gpu
def test_golden_suite_in_one_call(enc, oracle):
    """All originals of tests/golden/suite/ (gray8, gray16, RGB8 at 512, 1000 and 1024 square) in ONE call: each stream equals its
    committed .felics file and pinned sha256."""
    from PIL import Image

    pins = json.load(open(os.path.join(GOLDEN, "pins.json")))["suite"]
    names = sorted(pins)
    imgs = [np.ascontiguousarray(np.array(Image.open(os.path.join(GOLDEN, "suite", n)))) for n in names]
    assert len({(im.shape, str(im.dtype)) for im in imgs}) >= 4
    got = enc.compress_images(imgs)
    for n, g in zip(names, got):
        want = open(os.path.join(GOLDEN, "suite", n + ".felics"), "rb").read()
        assert g == want, n
        assert hashlib.sha256(g).hexdigest() == pins[n]["sha256"], n
    _check_all(got, imgs, oracle, "suite")


@pytest.mark.gpu
def test_large_frame_with_odd_shapes(enc, oracle):
    """A 4096 x 2160 frame beside tiny, zero-sized, 1 x N, N x 1 images and widths 255/256/257, 4095/4096/4097."""
    from felics_amd import synth

    rng = np.random.default_rng(8)
    imgs = [synth.gray8(4096, 2160, 0, "S1")]
    imgs += [np.zeros((0, 7), np.uint8), np.zeros((5, 0, 3), np.uint8), np.zeros((0, 0), np.uint16)]
    imgs += [_rand(rng, 1, 1, "gray8"), _rand(rng, 2, 3, "rgb8"), _rand(rng, 1, 3000, "gray8"), _rand(rng, 3000, 1, "gray8"),
             _rand(rng, 1, 700, "rgb8"), _rand(rng, 700, 1, "rgb8")]
    for w in (255, 256, 257, 4095, 4096, 4097):
        imgs.append(_rand(rng, 3 + w % 5, w, "gray8"))
        imgs.append(_rand(rng, 2 + w % 3, w, "rgb8"))
    imgs.append(synth.rgb8(640, 360, 1))
    imgs.append(_rand(rng, 33, 47, "gray16"))
    order = rng.permutation(len(imgs))
    imgs = [imgs[i] for i in order]
    _check_all(enc.compress_images(imgs), imgs, oracle, "odd")


@pytest.mark.gpu
def test_mixed_shapes_share_submissions(oracle):
    """64 gray8 images, each of its own shape between 500 x 500 and 600 x 600, take at most two submissions (one per shape
    would be 64)."""
    e = _encoder()
    try:
        rng = np.random.default_rng(9)
        shapes = set()
        while len(shapes) < 64:
            shapes.add((int(rng.integers(500, 601)), int(rng.integers(500, 601))))
        imgs = [_rand(rng, h, w, "gray8") // 8 * 8 for h, w in sorted(shapes)]
        before = e.stats()["submissions"]
        got = e.compress_images(imgs)
        assert e.stats()["submissions"] - before <= 2, e.stats()
        _check_all(got, imgs, oracle, "share")
    finally:
        e.close()


@pytest.mark.gpu
@pytest.mark.parametrize("env", ["FELICS_TEST_TILE_CAP", "FELICS_TEST_LOOKBACK_FAIL", "FELICS_TEST_SCATTER_ORDER", "FELICS_TWO_PASS"])
def test_remedies_inside_a_mixed_call(oracle, env):
    """Each remedy of a sub-batch, inside a mixed call on a fresh context: the streams still equal the oracle's."""
    from felics_amd import synth

    e = _encoder(**{env: "1"})
    try:
        rng = np.random.default_rng(13)
        imgs = [synth.gray8(300 + 17 * i, 200 + 11 * i, i, "S1") for i in range(6)]
        imgs += [synth.rgb8(120 + 9 * i, 90 + 5 * i, i) for i in range(4)]
        imgs += [_rand(rng, 64, 64 + i, "gray8") for i in range(3)] + [_rand(rng, 20, 30, "gray16")]
        _check_all(e.compress_images(imgs), imgs, oracle, env)
        st = e.stats()
        if env == "FELICS_TEST_TILE_CAP":
            assert st["tile_overflows"] >= 1, st
        elif env == "FELICS_TEST_LOOKBACK_FAIL":
            assert st["lookback_fallbacks"] >= 1, st
        elif env == "FELICS_TEST_SCATTER_ORDER":
            assert st["scatter_fallbacks"] >= 1, st
        _check_all(e.compress_images(imgs[::-1]), imgs[::-1], oracle, env + " again")
    finally:
        e.close()


@pytest.mark.gpu
def test_device_entry_point_placement(enc, oracle):
    """Device tensors of different shapes: offsets 16-byte aligned, ascending, non-overlapping; a buffer of exactly the rounded
    stream sizes still works (exact placement), 16 bytes less reports the size needed.  Host entry point: a too-small buffer
    reports every size and gets nothing written."""
    import torch

    from felics_amd import api

    rng = np.random.default_rng(17)
    imgs = [_rand(rng, 37, 51, "gray8"), _rand(rng, 200, 300, "rgb8"), _rand(rng, 64, 64, "gray16"), np.zeros((0, 4), np.uint8),
            (rng.integers(0, 40, size=(513, 700), dtype=np.uint8)), _rand(rng, 9, 1, "rgb8")]
    want = [oracle.compress(im) for im in imgs]
    dev = [torch.from_numpy(im).cuda() if im.size else None for im in imgs]
    torch.cuda.synchronize()
    descs = []
    for im, t in zip(imgs, dev):
        _, w, h, color, depth = api._describe(im)
        descs.append((t.data_ptr() if t is not None else 0, w, h, int(color), int(depth)))

    def run(cap):
        out = torch.zeros(max(cap, 16), dtype=torch.uint8, device="cuda")
        offs, lens = enc.compress_images_device(descs, out.data_ptr(), cap)
        host = out.cpu().numpy()
        return offs, lens, [host[int(o):int(o) + int(n)].tobytes() for o, n in zip(offs, lens)]

    big = sum(len(w) for w in want) * 2 + 4096 * len(want)
    for cap in (big, sum((len(w) + 15) // 16 * 16 for w in want)):
        offs, lens, got = run(cap)
        assert got == want, cap
        assert all(int(o) % 16 == 0 for o in offs)
        for i in range(1, len(offs)):
            assert offs[i] >= offs[i - 1] + lens[i - 1]
    exact = sum((len(w) + 15) // 16 * 16 for w in want)
    with pytest.raises(api.FelicsError) as ei:
        run(exact - 16)
    assert ei.value.code == E_BUFFER_TOO_SMALL and ("need %d bytes" % exact) in str(ei.value)

    n = len(imgs)
    descr = [api._describe(im) for im in imgs]
    cimgs = (api._CImage * n)(*[api._CImage(d[0].ctypes.data if d[0].size else None, d[1], d[2], int(d[3]), int(d[4])) for d in descr])
    caps = [len(w) + 64 for w in want]
    caps[1] = len(want[1]) - 1
    caps[4] = 10
    bufs = [np.full(c, 0xEE, dtype=np.uint8) for c in caps]
    op = (C.c_void_p * n)(*[b.ctypes.data for b in bufs])
    lens = (C.c_size_t * n)()
    rc = api.lib().felics_compress_images(enc._h, n, cimgs, op, (C.c_size_t * n)(*caps), lens)
    assert rc == E_BUFFER_TOO_SMALL
    assert list(lens) == [len(w) for w in want]
    for i in range(n):
        if i in (1, 4):
            assert (bufs[i] == 0xEE).all(), i
        else:
            assert bufs[i][: len(want[i])].tobytes() == want[i], i


@pytest.mark.gpu
def test_refused_while_a_ticket_is_outstanding(enc):
    import torch

    from felics_amd import api

    frames = torch.zeros((2, 64, 64), dtype=torch.uint8, device="cuda")
    out = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    out2 = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    sub = enc.submit_batch_device(frames.data_ptr(), 2, 64, 64, 0, 0, out.data_ptr(), out.numel())
    try:
        with pytest.raises(api.FelicsError) as ei:
            enc.compress_images_device([(frames.data_ptr(), 64, 64, 0, 0)], out2.data_ptr(), out2.numel())
        assert ei.value.code == E_INVALID_ARGUMENT
        with pytest.raises(api.FelicsError) as ei:
            enc.compress_images([np.zeros((3, 3), np.uint8)])
        assert ei.value.code == E_INVALID_ARGUMENT
    finally:
        enc.wait_batch(sub)


@pytest.mark.gpu
def test_random_mixed_sweep(enc, oracle):
    """About 40 calls of 1-40 images each: shapes from 1 x 1 to ~1500 x 1500, gray8 / RGB8 / gray16, noise, flat content and
    crops of the golden images."""
    from PIL import Image

    rng = np.random.default_rng(2024)
    sources = []
    for name in ("suite/boat.tiff", "suite/lena_color_512.tif", "man.tiff", "suite/5.3.01.tiff"):
        sources.append(np.ascontiguousarray(np.array(Image.open(os.path.join(GOLDEN, name)))))
    for call in range(40):
        imgs = []
        for _ in range(int(rng.integers(1, 41))):
            side = int(rng.choice([4, 40, 400, 1500]))
            h, w = int(rng.integers(1, side + 1)), int(rng.integers(1, side + 1))
            kind = str(rng.choice(["gray8", "rgb8", "gray16"], p=[0.5, 0.35, 0.15]))
            if kind == "gray16":
                h, w = max(1, h // 4), max(1, w // 4)
            style = int(rng.integers(0, 3))
            if style == 0:
                img = _rand(rng, h, w, kind)
            elif style == 1:
                img = np.full((h, w, 3) if kind == "rgb8" else (h, w), int(rng.integers(0, 256)), np.uint16 if kind == "gray16" else np.uint8)
            else:
                src = [s for s in sources if (s.ndim == 3) == (kind == "rgb8")]
                src = src[int(rng.integers(0, len(src)))]
                y, x = int(rng.integers(0, src.shape[0])), int(rng.integers(0, src.shape[1]))
                img = np.ascontiguousarray(src[y:y + h, x:x + w])
                if kind == "gray16":
                    img = img.astype(np.uint16) * 257
                elif img.dtype != np.uint8:
                    img = (img >> 8).astype(np.uint8)
            imgs.append(img)
        _check_all(enc.compress_images(imgs), imgs, oracle, "call %d" % call)
