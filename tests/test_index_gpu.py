"""Restart index on the GPU: felics_decompress_batch_device_indexed (a wave per segment, k_decode8_seg) against the original pixels,
with host-built indexes over oracle streams and with the encoder's; its counters, its refusals (none may fault) and what it does not
support; felics_compress_batch_device_indexed's indexes byte for byte against felics_index_build's, on every pack variant."""
import glob
import os

import numpy as np
import pytest

from tests import index_common as ic

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture(scope="module")
def enc():
    import felics_amd

    e = felics_amd.Encoder(0)
    yield e
    e.close()


_decode_indexed = ic.decode_indexed  # (shared with test_index_large_gpu.py)


@pytest.mark.parametrize("rgb", (0, 1))
@pytest.mark.parametrize("w,h", ic.SHAPES)
def test_decode_with_host_built_index(enc, oracle, w, h, rgb):
    """Oracle streams, felics_index_build's indexes (no encoder involved): three frames of different content per shape, both segment
    sizes, the pixels of the originals; segments8 counts n * C * K."""
    from felics_amd import api

    imgs = ic.images(w, h, rgb, 3)
    streams = [oracle.compress(im) for im in imgs]
    for seg in ic.SEGMENTS:
        indexes = [api.index_build(s, seg) for s in streams]
        before = enc.decode_stats()
        status, frames = _decode_indexed(enc, streams, indexes, imgs[0].size, guard=256)
        assert (status == 0).all()
        for im, f in zip(imgs, frames):
            assert (f.reshape(im.shape) == im).all(), (w, h, rgb, seg)
        k = (w * h + seg - 1) // seg
        assert enc.decode_stats()["segments8"] - before["segments8"] == 3 * (3 if rgb else 1) * k


def test_suite_originals_at_65536(enc):
    """two 1024 x 1024 originals of tests/golden/suite/ (one gray, one RGB), their committed streams, 16 segments per plane"""
    from PIL import Image

    from felics_amd import api

    seen = set()
    for path in sorted(glob.glob(os.path.join(GOLDEN, "suite", "*.felics"))):
        stream = open(path, "rb").read()
        img = np.array(Image.open(path[:-len(".felics")]))
        if img.dtype != np.uint8 or img.shape[:2] != (1024, 1024) or img.ndim in seen:
            continue
        seen.add(img.ndim)
        index = api.index_build(stream, 65536)
        assert len(index) == ic.index_size(1024, 1024, int(img.ndim == 3), 65536)
        status, frames = _decode_indexed(enc, [stream], [index], img.size, guard=256)
        assert (status == 0).all() and (frames[0].reshape(img.shape) == img).all(), path
    assert seen == {2, 3}


@pytest.mark.parametrize("rgb", (0, 1))
def test_corrupt_index_of_one_stream(enc, oracle, rgb):
    """Four streams; stream 2's index carries one of the corruptions the host refuses: status[2] is FELICS_E_INVALID_INDEX, the other
    three decode exactly, nothing outside d_pixels changes."""
    from felics_amd import api

    imgs = ic.images(100, 100, rgb, 4)
    streams = [oracle.compress(im) for im in imgs]
    good = [api.index_build(s, 4096) for s in streams]
    for name, bad in ic.corruptions(good[2]).items():
        if len(bad) != len(good[2]):
            continue  # (the size is the stride's business on the device: below)
        status, frames = _decode_indexed(enc, streams, good[:2] + [bad] + good[3:], imgs[0].size, guard=4096, expect=ic.E_INVALID_INDEX)
        assert list(status) == [0, 0, ic.E_INVALID_INDEX, 0], (name, status)
        for i in (0, 1, 3):
            assert (frames[i].reshape(imgs[i].shape) == imgs[i]).all(), (name, i)
    # index 0 names how every index is cut: a stride that cannot hold it, or a corrupt header there, refuses the call
    import torch

    blob, offs, lens = ic.pack_streams(streams)
    d_in = torch.from_numpy(np.frombuffer(blob, dtype=np.uint8).copy()).cuda()
    d_idx = torch.from_numpy(np.frombuffer(good[0] + bytes(64), dtype=np.uint8).copy()).cuda()
    d_px = torch.zeros(imgs[0].size * 4, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    import felics_amd

    with pytest.raises(felics_amd.FelicsError) as ei:
        enc.decompress_batch_device_indexed(d_in.data_ptr(), offs, lens, d_idx.data_ptr(), 64, d_px.data_ptr(), d_px.numel())
    assert ei.value.code == ic.E_INVALID_INDEX and (ei.value.status == ic.E_INVALID_INDEX).all()
    with pytest.raises(felics_amd.FelicsError) as ei:  # an unaligned stride is an argument error
        enc.decompress_batch_device_indexed(d_in.data_ptr(), offs, lens, d_idx.data_ptr(), len(good[0]) + 8, d_px.data_ptr(), d_px.numel())
    assert ei.value.code == -11


def test_corrupt_stream_under_a_good_index(enc, oracle):
    """A truncated stream and one with a forged header, each beside the index of the good stream: an error status for them, exact
    pixels for the stream beside them."""
    from felics_amd import api

    imgs = ic.images(64, 65, 0, 2)
    streams = [oracle.compress(im) for im in imgs]
    indexes = [api.index_build(s, 4096) for s in streams]
    cut = streams[1][:len(streams[1]) // 2]
    status, frames = _decode_indexed(enc, [streams[0], cut], indexes, imgs[0].size, guard=4096, expect=ic.E_INVALID_INDEX)
    assert status[0] == 0 and status[1] == ic.E_INVALID_INDEX and (frames[0].reshape(imgs[0].shape) == imgs[0]).all()
    forged = streams[1][:6] + (65).to_bytes(4, "big") + (64).to_bytes(4, "big") + streams[1][14:]
    status, frames = _decode_indexed(enc, [streams[0], forged], indexes, imgs[0].size, guard=4096, expect=-4)
    assert status[0] == 0 and status[1] == -4 and (frames[0].reshape(imgs[0].shape) == imgs[0]).all()


def test_unsupported(enc, oracle):
    """Rows too wide for the LDS (the smallest such W, H = 1) and a 16-bit batch: FELICS_E_UNSUPPORTED everywhere, no host fallback."""
    from felics_amd import api

    w = next(w for w in range(39000, 41000) if 256 * 24 + 2 * 2 * ((w + 63) // 64 * 64) > 160 * 1024)
    assert 256 * 24 + 2 * 2 * ((w - 1 + 63) // 64 * 64) <= 160 * 1024
    img = (np.arange(w, dtype=np.uint32) // 3 % 256).astype(np.uint8).reshape(1, w)
    stream = oracle.compress(img)
    index = api.index_build(stream, 4096)
    assert (api.decompress_indexed(stream, index) == img).all()  # the host decodes it through its index
    status, _ = _decode_indexed(enc, [stream, stream], [index, index], img.size, guard=256, expect=ic.E_UNSUPPORTED)
    assert (status == ic.E_UNSUPPORTED).all()
    # one column narrower fits
    img2 = img[:, :w - 1].copy()
    s2 = oracle.compress(img2)
    status, frames = _decode_indexed(enc, [s2], [api.index_build(s2, 4096)], img2.size, guard=256)
    assert (status == 0).all() and (frames[0].reshape(img2.shape) == img2).all()
    s16 = oracle.compress(np.arange(64 * 65, dtype=np.uint16).reshape(65, 64))
    some = api.index_build(oracle.compress(np.zeros((65, 64), np.uint8)), 4096)
    status, _ = _decode_indexed(enc, [s16, s16], [some, some], 64 * 65 * 2, guard=256, expect=ic.E_UNSUPPORTED)
    assert (status == ic.E_UNSUPPORTED).all()


# ---- the encoder's index -------------------------------------------------------------------------------------------------------

_encode_indexed = ic.encode_indexed  # (shared with test_index_large_gpu.py)


def _first_difference(a, b):
    return next((i for i in range(min(len(a), len(b))) if a[i] != b[i]), min(len(a), len(b)))


@pytest.mark.parametrize("rgb", (0, 1))
@pytest.mark.parametrize("w,h", [s for s in ic.SHAPES if s[0] * s[1]])
def test_encoder_index_equals_index_build(enc, oracle, w, h, rgb):
    """The encoder's index equals felics_index_build of the same stream byte for byte, and the streams equal the oracle's: three
    frames of different content per shape, both segment sizes; the decoder takes the pair as it lies in device memory."""
    from felics_amd import api

    imgs = ic.images(w, h, rgb, 3)
    want = [oracle.compress(im) for im in imgs]
    for seg in ic.SEGMENTS:
        streams, indexes = _encode_indexed(enc, imgs, seg)
        assert streams == want, (w, h, rgb, seg)
        for s, got in zip(streams, indexes):
            ref = api.index_build(s, seg)
            assert len(got) == len(ref) and got == ref, (w, h, rgb, seg, _first_difference(got, ref))
        status, frames = _decode_indexed(enc, streams, indexes, imgs[0].size, guard=256)
        assert (status == 0).all()
        for im, f in zip(imgs, frames):
            assert (f.reshape(im.shape) == im).all(), (w, h, rgb, seg)


def test_encoder_index_of_empty_images(enc, oracle):
    from felics_amd import api

    for w, h in ((0, 5), (5, 0)):
        for rgb in (0, 1):
            imgs = ic.images(w, h, rgb, 2)
            streams, indexes = _encode_indexed(enc, imgs, 4096, d_out_cap=4096)
            assert streams == [oracle.compress(im) for im in imgs]
            assert indexes == [api.index_build(s, 4096) for s in streams] and len(indexes[0]) == 64


VARIANTS = [{"FELICS_TEST_LOOKBACK_FAIL": "1"}, {"FELICS_TEST_SCATTER_ORDER": "1"}, {"FELICS_TEST_TILE_CAP": "1"}, {"exact": "1"},
            {"FELICS_TEST_PASS_IMAGES": "1"}]


@pytest.mark.parametrize("variant", VARIANTS, ids=lambda v: next(iter(v)))
def test_encoder_index_under_forced_variants(oracle, variant):
    """The 512 x 256 S1 batch under each forced variant, one at a time, with FELICS_POISON on: a pass that is redone by a remedy
    rewrites its index, exact placement and several passes leave the same bytes."""
    import felics_amd
    from felics_amd import api

    env = {k: v for k, v in variant.items() if k.startswith("FELICS_")}
    imgs = [ic.images(512, 256, rgb, 3) for rgb in (0, 1)]
    os.environ.update(env)
    os.environ["FELICS_POISON"] = "1"
    try:
        e = felics_amd.Encoder(0)
        try:
            for batch in imgs:
                want = [oracle.compress(im) for im in batch]
                exact_cap = sum((len(s) + 15) // 16 * 16 for s in want) if "exact" in variant else None  # too small for slots
                for seg in ic.SEGMENTS:
                    streams, indexes = _encode_indexed(e, batch, seg, d_out_cap=exact_cap)
                    assert streams == want, (variant, seg)
                    for s, got in zip(streams, indexes):
                        ref = api.index_build(s, seg)
                        assert got == ref, (variant, seg, _first_difference(got, ref))
            st = e.stats()
            if "FELICS_TEST_LOOKBACK_FAIL" in env:
                assert st["lookback_fallbacks"] >= 1
            if "FELICS_TEST_SCATTER_ORDER" in env:
                assert st["scatter_fallbacks"] >= 1
            if "FELICS_TEST_TILE_CAP" in env:
                assert st["tile_overflows"] >= 1
            if "FELICS_TEST_PASS_IMAGES" in env:
                assert st["submissions"] >= 2 * 2 * 3
        finally:
            e.close()
    finally:
        for k in list(env) + ["FELICS_POISON"]:
            del os.environ[k]


def test_encoder_index_refusals(enc):
    import torch

    import felics_amd
    from felics_amd import api

    img = ic.images(64, 65, 0, 1)[0]
    d_in = torch.from_numpy(img).cuda()
    d_out = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    isize = api.index_size(64, 65, 0, 0, 4096)
    d_idx = torch.full((isize + 64,), 0x5A, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()

    def call(seg=4096, depth=0, cap=isize, at=0):
        return api.lib().felics_compress_batch_device_indexed(enc._h, 1, d_in.data_ptr(), 64, 65, 0, depth, d_out.data_ptr(), d_out.numel(), seg,
                                                              d_idx.data_ptr() + at, cap, None, None)

    import ctypes as C

    offs, lens = (C.c_uint64 * 1)(), (C.c_uint64 * 1)()

    def call2(seg=4096, depth=0, cap=isize, at=0):
        return api.lib().felics_compress_batch_device_indexed(enc._h, 1, d_in.data_ptr(), 64, 65, 0, depth, d_out.data_ptr(), d_out.numel(), seg,
                                                              d_idx.data_ptr() + at, cap, offs, lens)

    assert call() == -11  # NULL offsets / lens
    assert call2(cap=isize - 1) == -8  # before anything is launched: the buffer is untouched
    assert call2(seg=6000) == -11 and call2(at=8) == -11
    assert call2(depth=1) == ic.E_UNSUPPORTED
    assert (d_idx.cpu().numpy() == 0x5A).all()
    assert call2() == 0
    # refused like the other synchronous entry points while a ticket is outstanding
    t = enc.submit_batch_device(d_in.data_ptr(), 1, 64, 65, 0, 0, d_out.data_ptr(), d_out.numel())
    assert call2() == -11
    enc.wait_batch(t)
    assert call2() == 0
