"""Restart index on the GPU, lane form: felics_decompress_batch_device_indexed with 64 segments per wave (k_decode8_seg_lanes, a lane
per stream) and the rest of the batch a wave per segment beside it -- the original pixels at every shape that starts, ends or reads
the row above differently, the counters, the passes, the fallbacks, the refusals (none may fault) and the wave form's results."""
import os

import numpy as np
import pytest

from tests import index_common as ic

pytestmark = pytest.mark.gpu

GUARD = 256

# (W, H): what each covers is in the comment behind it
SHAPES = [
    (64, 65),     # K = 2, last segment 64 pixels
    (99, 130),    # x0 = 37, 74, 12: starts and ends inside a group of four, x0 & 3 = 1, 2, 0
    (9, 1000),    # W just above the limit, a one-sample tail group, x0 = 1, 2
    (8, 600),     # W = 8, x0 = 0
    (4097, 1),    # segments starting in row 0, window mostly in front of the plane
    (5000, 3),
    (8200, 2),    # rows wider than a segment
    (4096, 3),    # x0 = 0 on every boundary: (0, y0 - 2) out of the window
    (512, 256),   # S1 first: halvings before the later checkpoints
]


@pytest.fixture(scope="module")
def enc():
    import felics_amd

    e = felics_amd.Encoder(0)
    yield e
    e.close()


@pytest.fixture()
def switch():
    """sets FELICS_TEST_INDEX_LANES / _PASS for one test (read per call by the library)"""
    names = ("FELICS_TEST_INDEX_LANES", "FELICS_TEST_INDEX_LANES_PASS")
    saved = {k: os.environ.pop(k, None) for k in names}

    def set_(lanes=None, per_pass=None):
        for k, v in zip(names, (lanes, per_pass)):
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = str(v)

    yield set_
    for k, v in saved.items():
        os.environ.pop(k, None)
        if v is not None:
            os.environ[k] = v


def frames(w, h, rgb, n):
    """n frames of one shape, every one of its own content: noise with a per-stream seed (cold contexts: the table rows loaded from
    the checkpoint), the ramp shifted per stream, synth S1 frames (512 x 256: S1 first)"""
    from felics_amd import synth

    shape = (h, w, 3) if rgb else (h, w)
    order = (2, 0, 1) if (w, h) == (512, 256) else (0, 1, 2)
    out = []
    for i in range(n):
        kind = order[i % 3]
        if kind == 0:
            out.append(np.random.default_rng(1000003 * i + w * 7919 + h * 31 + rgb).integers(0, 256, size=shape, dtype=np.uint8))
        elif kind == 1:
            smooth = ((np.add.outer(np.arange(h), np.arange(w)) // 2 + 5 * i) % 256).astype(np.uint8)
            out.append(np.stack([smooth, smooth[::-1], 255 - smooth], -1).copy() if rgb else smooth)
        else:
            out.append(synth.rgb8(w, h, i) if rgb else synth.gray8(w, h, i, "S1"))
    return out


_cache = {}


def batch(oracle, w, h, rgb, n):
    """(frames, oracle streams): computed once per (shape, colour), shared and left unchanged"""
    key = (w, h, rgb)
    if key not in _cache or len(_cache[key][0]) < n:
        imgs = frames(w, h, rgb, n)
        _cache[key] = (imgs, [oracle.compress(im) for im in imgs])
    imgs, streams = _cache[key]
    return imgs[:n], streams[:n]


def decode(enc, streams, indexes, frame_bytes, expect=None):
    """streams + their indexes -> (status, frames as uint8 rows); asserts the 0xA5 guard of GUARD bytes around d_pixels"""
    import torch

    import felics_amd

    n = len(streams)
    blob, offs, lens = ic.pack_streams(streams)
    stride = max((max(len(i) for i in indexes) + 15) // 16 * 16, 64)
    iblob = b"".join(i + bytes(stride - len(i)) for i in indexes)
    d_in = torch.from_numpy(np.frombuffer(blob, dtype=np.uint8).copy()).cuda()
    d_idx = torch.from_numpy(np.frombuffer(iblob, dtype=np.uint8).copy()).cuda()
    total = frame_bytes * n
    d_px = torch.full((GUARD + total + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    args = (d_in.data_ptr(), offs, lens, d_idx.data_ptr(), stride, d_px.data_ptr() + GUARD, total)
    if expect is None:
        _, status = enc.decompress_batch_device_indexed(*args)
    else:
        with pytest.raises(felics_amd.FelicsError) as ei:
            enc.decompress_batch_device_indexed(*args)
        assert ei.value.code == expect
        status = ei.value.status
    host = d_px.cpu().numpy()
    assert (host[:GUARD] == 0xA5).all() and (host[GUARD + total:] == 0xA5).all()
    assert (d_idx.cpu().numpy() == np.frombuffer(iblob, dtype=np.uint8)).all()  # the checkpoints are read, never written
    return status, [host[GUARD + i * frame_bytes:GUARD + (i + 1) * frame_bytes] for i in range(n)]


def delta(enc, before):
    now = enc.decode_stats()
    return {k: now[k] - before[k] for k in ("segments8", "lane_segments8", "lane_passes")}


def exact(imgs, out, which=None):
    for i, (im, f) in enumerate(zip(imgs, out)):
        if which is None or i in which:
            assert (f.reshape(im.shape) == im).all(), (i, int(np.argmax(f != im.reshape(-1))))


@pytest.mark.parametrize("rgb", (0, 1))
@pytest.mark.parametrize("w,h", SHAPES)
def test_exact_pixels(enc, oracle, switch, w, h, rgb):
    """n = 67: one wave of 64 lanes and three streams a wave per segment, both segment sizes: the originals' pixels, all statuses 0,
    lane_segments8 grows by 64 C K and segments8 by 3 C K."""
    from felics_amd import api

    switch(lanes=1)
    imgs, streams = batch(oracle, w, h, rgb, 67)
    c = 3 if rgb else 1
    for seg in ic.SEGMENTS:
        indexes = [api.index_build(s, seg) for s in streams]
        before = enc.decode_stats()
        status, out = decode(enc, streams, indexes, imgs[0].size)
        k = (w * h + seg - 1) // seg
        d = delta(enc, before)
        assert (status == 0).all(), (seg, status)
        exact(imgs, out)
        assert d["lane_segments8"] == 64 * c * k and d["segments8"] == 3 * c * k and d["lane_passes"] == 1, (seg, d)


@pytest.mark.parametrize("rgb", (0, 1))
@pytest.mark.parametrize("n", (64, 130))
def test_whole_waves_and_a_tail(enc, oracle, switch, n, rgb):
    """100 x 100: exactly one wave with no wave-form tail, then two waves plus two streams"""
    from felics_amd import api

    switch(lanes=1)
    imgs, streams = batch(oracle, 100, 100, rgb, 130)
    imgs, streams = imgs[:n], streams[:n]
    indexes = [api.index_build(s, 4096) for s in streams]
    before = enc.decode_stats()
    status, out = decode(enc, streams, indexes, imgs[0].size)
    assert (status == 0).all()
    exact(imgs, out)
    c, k = (3 if rgb else 1), 3
    assert delta(enc, before) == {"lane_segments8": n // 64 * 64 * c * k, "segments8": n % 64 * c * k, "lane_passes": 1}


@pytest.mark.parametrize("rgb", (0, 1))
def test_encoder_indexes_as_they_lie(enc, switch, rgb):
    """compress_batch_device_indexed on 64 frames of 99 x 130: streams and indexes decode where the encoder left them"""
    import torch

    from felics_amd import api

    switch(lanes=1)
    w, h, n, seg = 99, 130, 64, 4096
    imgs = frames(w, h, rgb, n)
    isize = api.index_size(w, h, rgb, 0, seg)
    d_in = torch.from_numpy(np.stack(imgs)).cuda()
    cap = n * ((imgs[0].size * 5 // 4 + 64 + 15) // 16 * 16)
    d_out = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    d_idx = torch.zeros(n * isize, dtype=torch.uint8, device="cuda")
    total = imgs[0].size * n
    d_px = torch.full((GUARD + total + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    offs, lens = enc.compress_batch_device_indexed(d_in.data_ptr(), n, w, h, rgb, 0, d_out.data_ptr(), cap, seg, d_idx.data_ptr(), n * isize)
    before = enc.decode_stats()
    _, status = enc.decompress_batch_device_indexed(d_out.data_ptr(), offs, lens, d_idx.data_ptr(), isize, d_px.data_ptr() + GUARD, total)
    host = d_px.cpu().numpy()
    assert (status == 0).all() and (host[:GUARD] == 0xA5).all() and (host[GUARD + total:] == 0xA5).all()
    assert (host[GUARD:GUARD + total] == np.stack(imgs).reshape(-1)).all()
    assert delta(enc, before)["lane_segments8"] == 64 * (3 if rgb else 1) * 4


def test_fallbacks(enc, oracle, switch):
    """what keeps a wave per segment: W < 8 and n < 64 under the switch, n = 67 with the switch at 0, n = 3 without the switch"""
    from felics_amd import api

    def run(w, h, n, lanes):
        switch(lanes=lanes)
        imgs, streams = batch(oracle, w, h, 0, max(n, 64))
        imgs, streams = imgs[:n], streams[:n]
        indexes = [api.index_build(s, 4096) for s in streams]
        before = enc.decode_stats()
        status, out = decode(enc, streams, indexes, imgs[0].size)
        assert (status == 0).all()
        exact(imgs, out)
        k = (w * h + 4095) // 4096
        assert delta(enc, before) == {"lane_segments8": 0, "segments8": n * k, "lane_passes": 0}, (w, h, n, lanes)

    run(2, 5000, 64, 1)
    run(100, 100, 63, 1)
    run(100, 100, 67, 0)
    run(100, 100, 3, None)


def test_passes(enc, oracle, switch):
    """FELICS_TEST_INDEX_LANES_PASS=64 on n = 130, 100 x 100 RGB: a pass per wave, C K 2 of them, the same pixels"""
    from felics_amd import api

    switch(lanes=1, per_pass=64)
    imgs, streams = batch(oracle, 100, 100, 1, 130)
    indexes = [api.index_build(s, 4096) for s in streams]
    before = enc.decode_stats()
    status, out = decode(enc, streams, indexes, imgs[0].size)
    assert (status == 0).all()
    exact(imgs, out)
    assert delta(enc, before) == {"lane_segments8": 128 * 3 * 3, "segments8": 2 * 3 * 3, "lane_passes": 3 * 3 * 2}


@pytest.mark.parametrize("rgb", (0, 1))
@pytest.mark.parametrize("bad_at", (5, 65))
def test_corrupt_index_of_one_stream(enc, oracle, switch, bad_at, rgb):
    """n = 67 of 100 x 100; one stream (a lane of the wave, or one of the wave-form tail) carries each same-size corruption of
    index_common.corruptions -- offset_plus_1, which only the end check catches, and co_300 among them: FELICS_E_INVALID_INDEX for it,
    exact pixels for every other stream, the guard intact."""
    from felics_amd import api

    switch(lanes=1)
    imgs, streams = batch(oracle, 100, 100, rgb, 130)
    imgs, streams = imgs[:67], streams[:67]
    good = [api.index_build(s, 4096) for s in streams]
    seen = set()
    for name, bad in ic.corruptions(good[bad_at]).items():
        if len(bad) != len(good[bad_at]):
            continue
        seen.add(name)
        status, out = decode(enc, streams, good[:bad_at] + [bad] + good[bad_at + 1:], imgs[0].size, expect=ic.E_INVALID_INDEX)
        want = [0] * 67
        want[bad_at] = ic.E_INVALID_INDEX
        assert list(status) == want, (name, status)
        exact(imgs, out, set(range(67)) - {bad_at})
    assert {"offset_plus_1", "offset_beyond", "magic"} <= seen and (not rgb or "co_300" in seen)


def test_corrupt_stream_under_a_good_index(enc, oracle, switch):
    """A truncated stream and one with a forged header in lane 1, each beside the index of the good stream: an error status for
    them, exact pixels for lane 0 and every other stream (refusals with bounded reads)."""
    from felics_amd import api

    switch(lanes=1)
    imgs, streams = batch(oracle, 64, 65, 0, 67)
    streams = list(streams[:64])
    imgs = imgs[:64]
    indexes = [api.index_build(s, 4096) for s in streams]
    good1 = streams[1]
    streams[1] = good1[:len(good1) // 2]
    status, out = decode(enc, streams, indexes, imgs[0].size, expect=ic.E_INVALID_INDEX)
    assert status[1] == ic.E_INVALID_INDEX and (np.delete(status, 1) == 0).all()
    exact(imgs, out, set(range(64)) - {1})
    streams[1] = good1[:6] + (65).to_bytes(4, "big") + (64).to_bytes(4, "big") + good1[14:]
    status, out = decode(enc, streams, indexes, imgs[0].size, expect=-4)
    assert status[1] == -4 and (np.delete(status, 1) == 0).all()
    exact(imgs, out, set(range(64)) - {1})


def test_both_forms_agree(enc, oracle, switch):
    """one noise batch, 67 x 512 x 256 gray: the status arrays and the pixels under =1 and =0 are identical"""
    from felics_amd import api

    w, h, n = 512, 256, 67
    imgs = [np.random.default_rng(77 + i).integers(0, 256, size=(h, w), dtype=np.uint8) for i in range(n)]
    streams = [oracle.compress(im) for im in imgs]
    indexes = [api.index_build(s, 4096) for s in streams]
    got = {}
    for lanes in (1, 0):
        switch(lanes=lanes)
        before = enc.decode_stats()
        got[lanes] = decode(enc, streams, indexes, imgs[0].size)
        assert (delta(enc, before)["lane_segments8"] > 0) == bool(lanes)
    assert (got[1][0] == got[0][0]).all() and (got[0][0] == 0).all()
    for a, b, im in zip(got[1][1], got[0][1], imgs):
        assert (a == b).all() and (a.reshape(im.shape) == im).all()
