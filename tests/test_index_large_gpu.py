"""The encoder's restart index (felics_index.hip) past 64 checkpoints and 8 tiles per segment: k_index_states' chunk loop makes
several trips (the carried find, finds in lanes 0 and 63, chunks without any) and its tile loop reads more than one group of eight
(the tail of a short last interval included), on banded frames whose contexts fall silent for many checkpoints.  Every stream
against the oracle, every index byte for byte against felics_index_build (which test_index_cpu.py holds against the format's model
at these sizes), guard bytes around both; then the three indexed decoders on what the encoder wrote, as it lies in device memory."""
import os

import numpy as np
import pytest

from tests import index_common as ic
from tests import region_common as rc

pytestmark = pytest.mark.gpu

GUARD = 256
_ROWS = [(w, h, st) for w, h, seg_tiles, _ in ic.LARGE for st in seg_tiles]


@pytest.fixture(scope="module")
def enc():
    import felics_amd

    e = felics_amd.Encoder(0)
    yield e
    e.close()


_frames, _refs = {}, {}


def batch(oracle, w, h, rgb):
    """(frames, oracle streams) of a shape: a banded frame per plan of ic.LARGE, one all-noise frame and the ramp, so that chains of
    differently planned frames lie side by side in one launch.  Computed once, shared and left unchanged."""
    key = (w, h, rgb)
    if key not in _frames:
        plans = []
        for ww, hh, _, ps in ic.LARGE:
            plans += [p for p in ps if (ww, hh) == (w, h) and p not in plans]
        tiles = (w * h + ic.GRANULE - 1) // ic.GRANULE
        imgs = [ic.banded(w, h, rgb, p) for p in plans] + [ic.banded(w, h, rgb, range(tiles), seed=6), ic.ramp(w, h, rgb)]
        _frames[key] = (imgs, [oracle.compress(im) for im in imgs])
    return _frames[key]


def reference(oracle, w, h, rgb, seg):
    """felics_index_build of the batch's oracle streams at a segment size"""
    from felics_amd import api

    key = (w, h, rgb, seg)
    if key not in _refs:
        _refs[key] = [api.index_build(s, seg) for s in batch(oracle, w, h, rgb)[1]]
    return _refs[key]


def check(got, oracle, w, h, rgb, seg, what=""):
    """streams equal the oracle's, every index equals felics_index_build's in length and bytes (the guards: ic.encode_indexed)"""
    _, want = batch(oracle, w, h, rgb)
    assert got.streams == want, (w, h, rgb, seg, what)
    for i, (idx, ref) in enumerate(zip(got.indexes, reference(oracle, w, h, rgb, seg))):
        d = ic.first_difference(idx, ref)
        assert len(idx) == len(ref) and d is None, "%s%d x %d rgb=%d segment %d, frame %d: index differs at byte %s: %s" % (
            what, w, h, rgb, seg, i, d, ic.where_in_index(ref, d))


def pixels_as_they_lie(enc, got, imgs):
    """felics_decompress_batch_device_indexed on the encoder's buffers: (status, frames)"""
    import torch

    total = imgs[0].size * len(imgs)
    d_px = torch.full((GUARD + total + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    _, status = enc.decompress_batch_device_indexed(got.d_out.data_ptr() + got.guard, got.offs, got.lens, got.d_idx.data_ptr() + got.guard,
                                                    got.isize, d_px.data_ptr() + GUARD, total)
    host = d_px.cpu().numpy()
    assert (host[:GUARD] == 0xA5).all() and (host[GUARD + total:] == 0xA5).all()
    return status, host[GUARD:GUARD + total].reshape((len(imgs),) + imgs[0].shape)


def regions_as_they_lie(enc, got, imgs, seg, windows):
    """One felics_decompress_regions_device_indexed call on the encoder's buffers, the windows dealt out over the frames: numpy crops,
    and segments_walked against felics_region_segments."""
    import torch

    from felics_amd import api

    h, w = imgs[0].shape[:2]
    planes = 3 if imgs[0].ndim == 3 else 1
    requests = [(k % len(imgs),) + win for k, win in enumerate(windows)]
    total = sum(r[3] * r[4] * planes for r in requests)
    d_px = torch.full((GUARD + total + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    before = enc.region_stats()
    _, status, offs = enc.decompress_regions_device_indexed(got.d_out.data_ptr() + got.guard, got.offs, got.lens, got.d_idx.data_ptr() + got.guard,
                                                            got.isize, requests, d_px.data_ptr() + GUARD, total)
    walked = enc.region_stats()["segments_walked"] - before["segments_walked"]
    host = d_px.cpu().numpy()
    assert (status == 0).all(), status
    assert (host[:GUARD] == 0xA5).all() and (host[GUARD + total:] == 0xA5).all()
    for r, o in zip(requests, offs):
        want = rc.crop(imgs[r[0]], r[1:])
        assert (host[GUARD + int(o):GUARD + int(o) + want.size].reshape(want.shape) == want).all(), (w, h, planes, seg, r)
    needed = [api.region_segments(w, h, seg, *r[1:]) for r in requests]
    assert walked == planes * sum(len(s) for s in needed)
    return needed


@pytest.mark.parametrize("rgb", (0, 1))
@pytest.mark.parametrize("w,h,seg_tiles", _ROWS)
def test_encoder_index_equals_index_build(enc, oracle, w, h, seg_tiles, rgb):
    """One felics_compress_batch_device_indexed call per row of ic.LARGE and colour.  At 4096 pixels per segment the wave-per-segment
    decoder then takes streams and indexes as they lie (statuses 0, the originals' pixels, segments8 grown by n C K), and at
    1000 x 541 and 1000 x 1100 (65536) the region decoder takes windows of them."""
    seg = seg_tiles * ic.GRANULE
    imgs, _ = batch(oracle, w, h, rgb)
    got = ic.encode_indexed(enc, imgs, seg, full=True)
    check(got, oracle, w, h, rgb, seg)
    k = (w * h + seg - 1) // seg
    planes = 3 if rgb else 1
    if seg_tiles == 1:
        before = enc.decode_stats()
        status, frames = pixels_as_they_lie(enc, got, imgs)
        assert (status == 0).all(), status
        for i, im in enumerate(imgs):
            assert (frames[i] == im).all(), (w, h, rgb, i)
        assert enc.decode_stats()["segments8"] - before["segments8"] == len(imgs) * planes * k
    if (w, h, seg_tiles) == (1000, 541, 1):
        # segments 64 and later only: rows 263 and below
        some = [win for win in rc.all_regions(w, h, 40, seed=3) if win[2] * win[3] and win[1] * w >= 64 * seg][:4]
        assert len(some) == 4
        needed = regions_as_they_lie(enc, got, imgs, seg, [(0, 300, 1000, 4), (990, 270, 10, 271), (500, 540, 1, 1)] + some)
        assert all(s and min(s) >= 64 for s in needed) and max(max(s) for s in needed) == k - 1
    if (w, h, seg_tiles) == (1000, 1100, 16):
        needed = regions_as_they_lie(enc, got, imgs, seg, [(0, 700, 1000, 3), (990, 500, 10, 600), (999, 1099, 1, 1)])
        assert needed[0] == [10] and needed[1] == list(range(7, 17)) and needed[2] == [16]


VARIANTS = [{"FELICS_TEST_PASS_IMAGES": "1"}, {"FELICS_TEST_TILE_CAP": "1"}, {"exact": "1"}]


@pytest.mark.parametrize("variant", VARIANTS, ids=lambda v: next(iter(v)))
def test_three_chunks_under_forced_variants(oracle, variant):
    """The 4096 x 132 batches (K = 132) on a fresh context under each variant, with FELICS_POISON on: a pass per image, a pass that
    is redone by a remedy and so rewrites an index of three chunks, exact placement -- the same bytes."""
    import felics_amd

    env = {k: v for k, v in variant.items() if k.startswith("FELICS_")}
    w, h, seg = 4096, 132, 4096
    os.environ.update(env)
    os.environ["FELICS_POISON"] = "1"
    try:
        e = felics_amd.Encoder(0)
        try:
            for rgb in (0, 1):
                imgs, want = batch(oracle, w, h, rgb)
                exact_cap = sum((len(s) + 15) // 16 * 16 for s in want) if "exact" in variant else None  # too small for slots
                before = e.stats()
                got = ic.encode_indexed(e, imgs, seg, d_out_cap=exact_cap, full=True)
                check(got, oracle, w, h, rgb, seg, "%s: " % next(iter(variant)))
                if "FELICS_TEST_PASS_IMAGES" in env:
                    assert e.stats()["submissions"] - before["submissions"] == len(imgs)
            if "FELICS_TEST_TILE_CAP" in env:
                assert e.stats()["tile_overflows"] >= 1
        finally:
            e.close()
    finally:
        for k in list(env) + ["FELICS_POISON"]:
            del os.environ[k]


@pytest.mark.parametrize("rgb", (0, 1))
def test_lane_form_at_the_default_segment(enc, oracle, rgb):
    """64 banded frames of 300 x 300 (22 tiles, plans and content from a fixed seed) at 65536 pixels per segment, K = 2, with
    FELICS_TEST_INDEX_LANES=1: the encoder's indexes equal felics_index_build's, k_decode8_seg_lanes takes them as they lie and
    gives the originals' pixels; lane_segments8 grows by 64 C 2."""
    from felics_amd import api

    w, h, n, seg = 300, 300, 64, 65536
    rng = np.random.default_rng(300)
    imgs = [ic.banded(w, h, rgb, np.flatnonzero(rng.random(22) < 0.3).tolist(), seed=100 + i) for i in range(n)]
    got = ic.encode_indexed(enc, imgs, seg, full=True)
    for i, (im, s, idx) in enumerate(zip(imgs, got.streams, got.indexes)):
        assert s == oracle.compress(im), i
        ref = api.index_build(s, seg)
        d = ic.first_difference(idx, ref)
        assert len(idx) == len(ref) and d is None, (i, d, ic.where_in_index(ref, d))
    saved = os.environ.get("FELICS_TEST_INDEX_LANES")
    os.environ["FELICS_TEST_INDEX_LANES"] = "1"
    try:
        before = enc.decode_stats()
        status, frames = pixels_as_they_lie(enc, got, imgs)
        after = enc.decode_stats()
    finally:
        del os.environ["FELICS_TEST_INDEX_LANES"]
        if saved is not None:
            os.environ["FELICS_TEST_INDEX_LANES"] = saved
    assert (status == 0).all(), status
    assert (frames == np.stack(imgs)).all()
    assert after["lane_segments8"] - before["lane_segments8"] == 64 * (3 if rgb else 1) * 2
