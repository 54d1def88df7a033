"""Restart index of 16-bit streams on the GPU: felics_decompress_batch_device_indexed16 (a wave per segment, k_decode16_seg) on every
case of index16_common.py against the original pixels and the unindexed decoder; several streams, passes, the table buffer and epoch
counter it shares with the unindexed forms; the corruption list (status against the host model's; none may fault); the refusals."""
import glob
import os

import numpy as np
import pytest

from tests import index16_common as ic

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture(scope="module")
def enc():
    import felics_amd

    e = felics_amd.Encoder(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def cases(oracle):
    """name -> (frame, oracle stream, index at 4096): computed once, read by every test"""
    from felics_amd import api

    out = {}
    for name, (img, _) in ic.cases().items():
        stream = oracle.compress(img)
        out[name] = (img, stream, api.index16_build(stream, 4096))
    return out


def _decode(enc, streams, indexes, frame_bytes, guard=256, expect=None, indexed=True, idx_shift=0, cap_short=0):
    """streams + their indexes -> (status, frames as uint16 arrays); checks the guard bytes around d_pixels and that d_index is
    byte-identical afterwards.  expect: the code the call must raise.  indexed=False: felics_decompress_batch_device."""
    import torch

    import felics_amd

    n = len(streams)
    blob, offs, lens = ic.pack(streams, 16)
    iblob, ioffs, ilens = ic.pack(indexes, 64)
    d_in = torch.from_numpy(np.frombuffer(blob, dtype=np.uint8).copy()).cuda()
    d_idx = torch.from_numpy(np.frombuffer(iblob, dtype=np.uint8).copy()).cuda()
    total = frame_bytes * n
    d_px = torch.full((guard + max(total, 16) + guard,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert d_idx.data_ptr() % 64 == 0 and (d_px.data_ptr() + guard) % 2 == 0
    if indexed:
        def call():
            return enc.decompress_batch_device_indexed16(d_in.data_ptr(), offs, lens, d_idx.data_ptr(), [o + idx_shift for o in ioffs], ilens,
                                                         d_px.data_ptr() + guard, total - cap_short)
    else:
        def call():
            return enc.decompress_batch_device(d_in.data_ptr(), offs, lens, d_px.data_ptr() + guard, total)
    if expect is None:
        _, status = call()
    else:
        with pytest.raises((felics_amd.FelicsError, felics_amd.DecompressionError)) as ei:
            call()
        assert ei.value.code == expect
        status = getattr(ei.value, "status", None)
    host = d_px.cpu().numpy()
    assert (host[:guard] == 0xA5).all() and (host[guard + max(total, 16):] == 0xA5).all()
    assert d_idx.cpu().numpy().tobytes() == iblob
    return status, [host[guard + i * frame_bytes:guard + (i + 1) * frame_bytes].view(np.uint16) for i in range(n)]


@pytest.mark.parametrize("name", list(ic.cases()))
def test_every_case(enc, cases, name):
    """pixels equal the original and the unindexed decoder's, every status 0, d_index and the guard bytes untouched, the counters add
    up: one wave per (plane, segment), one loaded row per row of the index"""
    img, stream, index = cases[name]
    lay = ic.Layout16(index)
    before = enc.index16_stats()
    status, frames = _decode(enc, [stream], [index], img.nbytes)
    after = enc.index16_stats()
    assert (status == 0).all() and (frames[0].reshape(img.shape) == img).all(), name
    assert after["streams"] - before["streams"] == 1
    assert after["segments16"] - before["segments16"] == lay.planes * max(lay.k, 1)
    assert after["rows_loaded"] - before["rows_loaded"] == sum(lay.n_rows())
    assert after["passes"] - before["passes"] >= 1 and after["table_bytes"] % (131071 * 64) == 0 and after["table_bytes"] > 0
    if img.size:
        status, plain = _decode(enc, [stream], [index], img.nbytes, indexed=False)
        assert (status == 0).all() and (plain[0] == frames[0]).all(), name


@pytest.mark.parametrize("seg", ic.SEGMENTS[1:])
def test_other_segment_sizes(enc, cases, seg):
    from felics_amd import api

    for name in ("100x100_rgb", "4100x3", "alias", "banded"):
        img, stream, _ = cases[name]
        status, frames = _decode(enc, [stream], [api.index16_build(stream, seg)], img.nbytes)
        assert (status == 0).all() and (frames[0].reshape(img.shape) == img).all(), (name, seg)


@pytest.mark.parametrize("rgb", (0, 1))
def test_several_streams(enc, oracle, rgb):
    """n = 1, 2, 5 streams of one shape and different content: indexes of different lengths at different offsets; one stream twice"""
    from felics_amd import api

    imgs = [ic.noise(64, 130, rgb, bits, 100 + bits) for bits in (12, 10, 8, 6)] + [ic.ramp(64, 130, rgb)]
    streams = [oracle.compress(im) for im in imgs]
    indexes = [api.index16_build(s, 4096) for s in streams]
    assert len(set(len(i) for i in indexes)) >= 4
    for n in (1, 2, 5):
        before = enc.index16_stats()
        status, frames = _decode(enc, streams[:n], indexes[:n], imgs[0].nbytes)
        assert (status == 0).all()
        for im, f in zip(imgs, frames):
            assert (f.reshape(im.shape) == im).all(), (rgb, n)
        after = enc.index16_stats()
        assert after["segments16"] - before["segments16"] == n * (3 if rgb else 1) * 3
        assert after["rows_loaded"] - before["rows_loaded"] == sum(sum(ic.Layout16(i).n_rows()) for i in indexes[:n])
    twice = [0, 3, 0]
    status, frames = _decode(enc, [streams[i] for i in twice], [indexes[i] for i in twice], imgs[0].nbytes)
    assert (status == 0).all() and all((f.reshape(imgs[i].shape) == imgs[i]).all() for i, f in zip(twice, frames))


@pytest.mark.parametrize("k", (1, 3))
def test_passes(enc, oracle, k):
    """FELICS_TEST_INDEX16_PASS = 1 and 3 on a 5-stream RGB16 call of 45 items: the same pixels, passes = ceil(items / k)"""
    from felics_amd import api

    imgs = [ic.noise(64, 130, 1, bits, 200 + bits) for bits in (12, 11, 10, 9, 8)]
    streams = [oracle.compress(im) for im in imgs]
    indexes = [api.index16_build(s, 4096) for s in streams]
    items = 5 * 3 * 3
    os.environ["FELICS_TEST_INDEX16_PASS"] = str(k)
    try:
        before = enc.index16_stats()
        status, frames = _decode(enc, streams, indexes, imgs[0].nbytes)
        after = enc.index16_stats()
    finally:
        del os.environ["FELICS_TEST_INDEX16_PASS"]
    assert (status == 0).all()
    for im, f in zip(imgs, frames):
        assert (f.reshape(im.shape) == im).all(), k
    assert after["passes"] - before["passes"] == (items + k - 1) // k
    assert after["table_bytes"] == k * 131071 * 64


def test_shared_table_and_epochs(oracle):
    """On one context: an unindexed 16-bit call (the wave form: the same table buffer, the same epoch counter), the indexed call, a
    16-bit lane-form call, the indexed call again -- all pixels right"""
    import felics_amd
    from felics_amd import api

    imgs = [ic.noise(64, 130, 0, bits, 300 + bits) for bits in (12, 9)]
    streams = [oracle.compress(im) for im in imgs]
    indexes = [api.index16_build(s, 4096) for s in streams]
    e = felics_amd.Encoder(0)
    try:
        def check(indexed, lanes=None):
            if lanes is not None:
                os.environ["FELICS_TEST_DECODE16_LANES"] = lanes
            try:
                status, frames = _decode(e, streams, indexes, imgs[0].nbytes, indexed=indexed)
            finally:
                os.environ.pop("FELICS_TEST_DECODE16_LANES", None)
            assert (status == 0).all() and all((f.reshape(im.shape) == im).all() for im, f in zip(imgs, frames)), (indexed, lanes)

        check(False, "0")
        check(True)
        check(False, "1")
        check(True)
        check(False, "0")
    finally:
        e.close()


# corruptions whose damage is one segment's own: every other segment of the stream must hold the right pixels
LOCAL = {"contexts_swapped": (0, 1), "contexts_equal": (0, 1), "context_out_of_range": (0, 1), "n_rows_plus_1": (0, 1), "n_rows_minus_1": (0, 1),
         "n_rows_at_j0": (0, 0)}


@pytest.mark.parametrize("rgb", (0, 1))
def test_corruptions(enc, cases, rgb):
    """Three streams; stream 1's index carries one of the corruptions: its status is the host model's code, the streams beside it
    decode, and (gray) where the damage is one segment's own the other segments hold the right pixels.  Every corruption is caught by
    a check the kernel makes before the read it guards."""
    import felics_amd
    from felics_amd import api

    img, stream, index = cases["100x100_rgb" if rgb else "100x100"]
    other = cases["ramp_100x100_rgb"] if rgb else (img[::-1].copy(), None, None)
    if not rgb:
        from tests import oracle_lib

        s2 = oracle_lib.load().compress(other[0])
        other = (other[0], s2, api.index16_build(s2, 4096))
    for what, bad in ic.corruptions(index).items():
        s = np.frombuffer(stream, np.uint8)
        b = np.frombuffer(bad, np.uint8)
        out = np.zeros(img.nbytes, np.uint8)
        want = api.lib().felics_decompress_indexed_wide(s.ctypes.data, len(s), b.ctypes.data, len(b), out.ctypes.data, out.nbytes, None)
        assert want == ic.E_INVALID_INDEX, what
        status, frames = _decode(enc, [other[1], stream, other[1]], [other[2], bad, other[2]], img.nbytes, guard=4096, expect=want)
        assert list(status) == [0, want, 0], (what, status)
        for i in (0, 2):
            assert (frames[i].reshape(img.shape) == other[0]).all(), (what, i)
        if not rgb and what in LOCAL:
            c, j = LOCAL[what]
            got, ref = frames[1], img.ravel()
            keep = np.ones(img.size, bool)
            keep[j * 4096:(j + 1) * 4096] = False
            assert (got[keep] == ref[keep]).all(), what


def test_header_mismatch_between_streams(enc, cases, oracle):
    """index 0 names segment_pixels and K, stream 0 the shape: a stream of another shape gets FELICS_E_INVALID_DIMENSIONS, an index cut at
    another segment size FELICS_E_INVALID_INDEX, the stream beside them decodes"""
    from felics_amd import api

    img, stream, index = cases["100x100"]
    _, s2, i2 = cases["64x65"]
    status, frames = _decode(enc, [stream, s2], [index, i2], img.nbytes, expect=-4)
    assert list(status) == [0, -4] and (frames[0].reshape(img.shape) == img).all()
    status, frames = _decode(enc, [stream, stream], [index, api.index16_build(stream, 8192)], img.nbytes, expect=ic.E_INVALID_INDEX)
    assert list(status) == [0, ic.E_INVALID_INDEX] and (frames[0].reshape(img.shape) == img).all()


def test_refusals(enc, cases, oracle):
    """before anything is launched: an 8-bit batch, the smallest row past the LDS limit, an index offset that is no multiple of 64, a
    short d_pixels_cap, an outstanding ticket"""
    import torch

    from felics_amd import api

    img, stream, index = cases["100x100"]
    img8 = (img >> 8).astype(np.uint8)
    s8 = oracle.compress(img8)
    status, _ = _decode(enc, [s8, s8], [index, index], img.nbytes, expect=ic.E_UNSUPPORTED)
    assert (status == ic.E_UNSUPPORTED).all()
    # 512 rows of 16 words, 512 tags, two rows of int32 padded to whole blocks of 64: W = 16128 fits 160 KiB, 16129 does not
    lds = lambda w: 512 * 64 + 512 * 4 + 2 * 4 * ((w + 63) // 64 * 64)
    assert lds(16128) <= 160 * 1024 < lds(16129)
    wide = (np.arange(16129, dtype=np.uint32) * 5 % 65536).astype(np.uint16).reshape(1, 16129)
    sw = oracle.compress(wide)
    iw = api.index16_build(sw, 4096)
    assert (api.decompress_indexed16(sw, iw) == wide).all()  # the host decodes it through its index
    status, _ = _decode(enc, [sw, sw], [iw, iw], wide.nbytes, expect=ic.E_UNSUPPORTED)
    assert (status == ic.E_UNSUPPORTED).all()
    _decode(enc, [stream, stream], [index, index], img.nbytes, expect=-11, idx_shift=16)
    status, _ = _decode(enc, [stream, stream], [index, index], img.nbytes, expect=-8, cap_short=2)
    assert (status == -8).all()
    # refused like the other synchronous entry points while a ticket is outstanding
    d_in = torch.from_numpy(img8).cuda()
    d_out = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    t = enc.submit_batch_device(d_in.data_ptr(), 1, 100, 100, 0, 0, d_out.data_ptr(), d_out.numel())
    try:
        _decode(enc, [stream], [index], img.nbytes, expect=-11)
    finally:
        enc.wait_batch(t)
    status, frames = _decode(enc, [stream], [index], img.nbytes)
    assert (status == 0).all() and (frames[0].reshape(img.shape) == img).all()


def test_suite_original_at_65536(enc):
    """one gray16 original of tests/golden/suite/ through its committed stream, segments of 65 536 pixels"""
    from PIL import Image

    from felics_amd import api

    for path in sorted(glob.glob(os.path.join(GOLDEN, "suite", "*.felics"))):
        stream = open(path, "rb").read()
        if stream[4] != 0 or stream[5] != 1:
            continue
        img = np.array(Image.open(path[:-len(".felics")]))
        index = api.index16_build(stream, 65536)
        status, frames = _decode(enc, [stream], [index], img.nbytes)
        assert img.dtype == np.uint16 and (status == 0).all() and (frames[0].reshape(img.shape) == img).all(), path
        return
    raise AssertionError("no gray16 original under tests/golden/suite/")
