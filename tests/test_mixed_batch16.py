"""16-bit images of different shapes in one submission (felics_compress_images*, felics_compress_views_device).

16-bit images are bucketed like 8-bit ones (T = ceil(w h / 4096), a bucket holds T_min .. ceil(1.25 T_min)); a bucket of more than
one shape is ONE mixed 16-bit sub-batch: the 16-bit pipeline with a per-plane geometry table, frames read in place, streams
written straight into their slots.  Every stream must equal the CPU oracle's for that image alone and decode back; felics_stats'
`submissions` shows that shapes really share sub-batches.  Every context is fresh and runs with FELICS_POISON=1."""
import io
import os

import numpy as np
import pytest

E_BUFFER_TOO_SMALL = -8
GRAY, RGB, D8, D16 = 0, 1, 0, 1


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


_WANT = {}  # the oracle's stream of an image of a shared corpus, by (corpus, index): computed once


def _want(oracle, img, key=None):
    if key is None:
        return oracle.compress(img)
    if key not in _WANT:
        _WANT[key] = oracle.compress(img)
    return _WANT[key]


def _check_all(got, imgs, oracle, what="", corpus=None):
    import felics_amd

    assert len(got) == len(imgs)
    for i, (g, img) in enumerate(zip(got, imgs)):
        want = _want(oracle, img, (corpus, i) if corpus else None)
        assert g == want, "%s image %d shape %s %s: %d vs %d bytes" % (what, i, img.shape, img.dtype, len(g), len(want))
        back = felics_amd.decompress_image(io.BytesIO(g))
        assert back.shape == img.shape and (back == img).all(), (what, i, img.shape)


def _noise(rng, h, w, rgb=False):
    return rng.integers(0, 65536, size=(h, w, 3) if rgb else (h, w), dtype=np.uint16)


def _content(rng, h, w, i, rgb=False):
    """Cycles through synth.gray16, full noise, 12-bit noise on an offset and flat."""
    from felics_amd import synth

    style = i % 4
    if style == 0:
        if rgb:
            return np.ascontiguousarray(np.stack([synth.gray16(w, h, 3 * i + c) for c in range(3)], axis=-1))
        return synth.gray16(w, h, i)
    if style == 1:
        return _noise(rng, h, w, rgb)
    if style == 2:
        return (rng.integers(0, 4096, size=(h, w, 3) if rgb else (h, w)) + 30000).astype(np.uint16)
    return np.full((h, w, 3) if rgb else (h, w), 777 + i, np.uint16)


def _spiky(rng, h, w, rgb=False, spikes=1):
    """Quiet data (samples 0 / 1: the events of context 0 are tiny, so its Rice parameter settles at 0) with full-scale spikes in the
    lower half where both neighbours are equal: the first spike of a plane is coded in unary, ~2^16 bits."""
    img = rng.integers(0, 2, size=(h, w), dtype=np.uint16)
    put = 0
    for y in range(h - 1, h // 2, -1):
        for x in range(w - 2, 0, -3):
            if put < spikes and img[y, x - 1] == img[y - 1, x]:
                img[y, x] = 65535
                put += 1
    assert put == spikes
    return np.ascontiguousarray(np.stack([img] * 3, axis=-1)) if rgb else img


def _distinct_shapes(rng, n, lo, hi):
    shapes = set()
    while len(shapes) < n:
        shapes.add((int(rng.integers(lo, hi + 1)), int(rng.integers(lo, hi + 1))))
    return sorted(shapes)


def _tiles(img):
    return -(-(img.shape[0] * img.shape[1]) // 4096)


def _one_bucket(imgs):
    t = [_tiles(im) for im in imgs]
    return max(t) <= -(-5 * min(t) // 4)


@pytest.mark.gpu
def test_every_tiny_shape_in_one_call16(oracle):
    """Every (w, h) with 1 <= w, h <= 19, gray16 and RGB16 random content: 722 images, two submissions (one per colour)."""
    rng = np.random.default_rng(105)
    imgs = [_noise(rng, h, w, rgb) for rgb in (False, True) for h in range(1, 20) for w in range(1, 20)]
    assert len(imgs) == 722
    e = _encoder()
    try:
        before = e.stats()["submissions"]
        got = e.compress_images(imgs)
        assert e.stats()["submissions"] - before <= 2, e.stats()
        _check_all(got, imgs, oracle, "tiny16")
    finally:
        e.close()


def _share_corpus(rgb):
    rng = np.random.default_rng(109 + rgb)
    if rgb:
        shapes = _distinct_shapes(rng, 16, 250, 280)
    else:
        shapes = _distinct_shapes(rng, 32, 500, 560)
    return [_content(rng, h, w, i, rgb) for i, (h, w) in enumerate(shapes)]


@pytest.mark.gpu
@pytest.mark.parametrize("wide_lane", [None, "0", "1", "7", "64"])
def test_shapes_share_submissions16(oracle, wide_lane):
    """32 gray16 images of distinct shapes in [500, 560]^2 (T = 62 .. 77 <= ceil(1.25 * 62) = 78) and 16 RGB16 ones in [250, 280]^2
    (T = 16 .. 20 = ceil(1.25 * 16)) are one bucket each: at most two submissions per call (one per shape would be 32 and 16).
    FELICS_WIDE_LANE: the wave-wide chain kernel alone, the four-lane kernel handing every chain over after 1 / 7 / 64 events."""
    e = _encoder(**({} if wide_lane is None else {"FELICS_WIDE_LANE": wide_lane}))
    old = os.environ.get("FELICS_WIDE_LANE")
    try:
        if wide_lane is not None:
            os.environ["FELICS_WIDE_LANE"] = wide_lane  # (read per sub-batch)
        for rgb in (False, True):
            imgs = _share_corpus(rgb)
            assert _one_bucket(imgs) and len({im.shape for im in imgs}) == len(imgs)
            before = e.stats()["submissions"]
            got = e.compress_images(imgs)
            assert e.stats()["submissions"] - before <= 2, (rgb, e.stats())
            _check_all(got, imgs, oracle, "share16 rgb=%d lane=%s" % (rgb, wide_lane), corpus="share%d" % rgb)
    finally:
        if wide_lane is not None:
            if old is None:
                del os.environ["FELICS_WIDE_LANE"]
            else:
                os.environ["FELICS_WIDE_LANE"] = old
        e.close()


@pytest.mark.gpu
def test_edges_in_one_call16(oracle):
    """Beside a 60 x 60 image: 1 x 1, 1 x 2, 2 x 1, 1 x 3000, 3000 x 1, widths 15 / 16 / 17 and 4095 / 4096 / 4097 with 1-3 rows, planes of
    exactly 4096 k - 1, 4096 k, 4096 k + 1 pixels for k = 1, 2 (planes with fewer tiles than their bucket's T_max, a last tile of one
    pixel), gray and RGB, zero-sized 16-bit images among them, order shuffled."""
    rng = np.random.default_rng(113)
    shapes = [(60, 60), (1, 1), (2, 1), (1, 2), (1, 3000), (3000, 1)]
    shapes += [(1 + w % 3, w) for w in (15, 16, 17, 4095, 4096, 4097)]
    shapes += [(63, 65), (64, 64), (17, 241), (1, 8191), (8191, 1), (64, 128), (3, 2731), (2731, 3)]
    assert {h * w for h, w in shapes} >= {4095, 4096, 4097, 8191, 8192, 8193}
    imgs = [_noise(rng, h, w, rgb) for rgb in (False, True) for h, w in shapes]
    imgs += [np.zeros((0, 7), np.uint16), np.zeros((5, 0, 3), np.uint16), np.zeros((0, 0), np.uint16)]
    imgs = [imgs[i] for i in rng.permutation(len(imgs))]
    e = _encoder()
    try:
        _check_all(e.compress_images(imgs), imgs, oracle, "edges16")
    finally:
        e.close()


@pytest.mark.gpu
def test_long_codes_in_a_mixed_sub_batch(oracle):
    """A quiet frame with full-scale spikes (a code of ~2^16 bits: more than one pack window in its tile) beside ordinary frames of
    other shapes in the same bucket, gray and RGB."""
    rng = np.random.default_rng(117)
    gray = [_spiky(rng, 200, 210, False, 3), _content(rng, 205, 207, 0), _content(rng, 199, 215, 1), _spiky(rng, 211, 202, False, 1),
            _content(rng, 208, 208, 2)]
    rgb = [_spiky(rng, 120, 130, True, 2), _content(rng, 125, 127, 0, True), _content(rng, 119, 133, 1, True)]
    assert _one_bucket(gray) and _one_bucket(rgb)
    assert len(oracle.compress(gray[0])) > 65536 // 8 and len(oracle.compress(rgb[0])) > 65536 // 8
    imgs = gray + rgb
    e = _encoder()
    try:
        before = e.stats()["slot_overflows"]
        got = e.compress_images(imgs)
        assert e.stats()["slot_overflows"] == before, e.stats()  # (long codes, but every stream inside its slot)
        _check_all(got, imgs, oracle, "long16")
    finally:
        e.close()


@pytest.mark.gpu
def test_slot_overflow_inside_a_mixed_sub_batch16(oracle):
    """One image of the bucket outgrows its slot (frame + frame / 4 + 64 bytes): the sub-batch is noted and redone, and every stream
    of the call is right -- the other images of that sub-batch too."""
    rng = np.random.default_rng(121)
    big = _spiky(rng, 40, 41, False, 1)
    assert len(oracle.compress(big)) > big.nbytes + big.nbytes // 4 + 64
    imgs = [_noise(rng, 39, 43), big, _content(rng, 44, 40, 0), _content(rng, 41, 41, 2), _noise(rng, 30, 31, True), _noise(rng, 33, 29, True)]
    e = _encoder()
    try:
        before = e.stats()["slot_overflows"]
        got = e.compress_images(imgs)
        assert e.stats()["slot_overflows"] - before >= 1, e.stats()
        _check_all(got, imgs, oracle, "overflow16")
    finally:
        e.close()


@pytest.mark.gpu
def test_device_placement16(oracle):
    """compress_images_device into a buffer full of a sentinel.  Room for the slots: offsets 16-byte aligned and ascending, streams at
    their slots, nothing outside the slots touched.  One slot short: exact placement, the same streams, nothing touched behind the
    last stream rounded to 16.  Less than the rounded sizes: FELICS_E_BUFFER_TOO_SMALL and the capacity needed."""
    import torch

    from felics_amd import api, synth

    rng = np.random.default_rng(125)
    imgs = [synth.gray16(150 + 3 * i, 140 - 2 * i, i) for i in range(5)]
    imgs += [np.ascontiguousarray(np.stack([synth.gray16(70 + i, 66 - i, 10 + 3 * i + c) for c in range(3)], axis=-1)) for i in range(3)]
    imgs = [imgs[i] for i in rng.permutation(len(imgs))]
    want = [oracle.compress(im) for im in imgs]
    dev = [torch.from_numpy(im).cuda() for im in imgs]
    torch.cuda.synchronize()
    descs = [(t.data_ptr(), im.shape[1], im.shape[0], RGB if im.ndim == 3 else GRAY, D16) for im, t in zip(imgs, dev)]
    slots = [(im.nbytes + im.nbytes // 4 + 64 + 15) // 16 * 16 for im in imgs]
    need = sum((len(w) + 15) // 16 * 16 for w in want)
    total = sum(slots)
    assert need <= total - slots[-1]
    SENT = 0xEE
    e = _encoder()
    try:
        def run(cap):
            out = torch.full((total + 4096,), SENT, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            offs, lens = e.compress_images_device(descs, out.data_ptr(), cap)
            return [int(o) for o in offs], [int(n) for n in lens], out.cpu().numpy()

        offs, lens, host = run(total)
        assert offs == [sum(slots[:i]) for i in range(len(slots))]
        assert all(o % 16 == 0 for o in offs)
        assert [host[o:o + n].tobytes() for o, n in zip(offs, lens)] == want
        assert (host[total:] == SENT).all()

        offs, lens, host = run(total - slots[-1])  # (the sizes first, then every stream at its place)
        assert all(o % 16 == 0 for o in offs) and offs[0] == 0
        assert all(offs[i] == offs[i - 1] + (lens[i - 1] + 15) // 16 * 16 for i in range(1, len(offs)))
        assert [host[o:o + n].tobytes() for o, n in zip(offs, lens)] == want
        assert offs[-1] + (lens[-1] + 15) // 16 * 16 == need
        assert (host[need:] == SENT).all()

        with pytest.raises(api.FelicsError) as ei:
            run(need - 16)
        assert ei.value.code == E_BUFFER_TOO_SMALL and ("need %d bytes" % need) in str(ei.value)
    finally:
        e.close()


@pytest.mark.gpu
def test_passes_of_a_mixed_bucket16(oracle):
    """FELICS_TEST_PASS_IMAGES=5: 12 images of one bucket are three sub-batches."""
    rng = np.random.default_rng(129)
    imgs = [_content(rng, 100 + i, 110 - i, i) for i in range(12)]
    assert _one_bucket(imgs)
    old = os.environ.get("FELICS_TEST_PASS_IMAGES")
    os.environ["FELICS_TEST_PASS_IMAGES"] = "5"  # (read when the call cuts its buckets into passes)
    e = _encoder()
    try:
        before = e.stats()["submissions"]
        got = e.compress_images(imgs)
        assert e.stats()["submissions"] - before == 3, e.stats()
        _check_all(got, imgs, oracle, "passes16")
    finally:
        if old is None:
            del os.environ["FELICS_TEST_PASS_IMAGES"]
        else:
            os.environ["FELICS_TEST_PASS_IMAGES"] = old
        e.close()


@pytest.mark.gpu
def test_views_and_company16(oracle):
    """One compress_views_device call: 12 gray16 crops of distinct shapes from one pitched surface, RGBA16 surfaces read as RGB, a
    pitched gray8 view and a dense RGB8 image.  The 16-bit views are gathered, as before, and then share submissions: one per
    depth and colour."""
    import torch

    rng = np.random.default_rng(133)
    surf16 = _noise(rng, 300, 700) // 16 * 16
    rgba16 = rng.integers(0, 65536, size=(64, 200, 4), dtype=np.uint16)
    surf8 = rng.integers(0, 256, size=(128, 256), dtype=np.uint8)
    rgb8 = rng.integers(0, 256, size=(50, 60, 3), dtype=np.uint8)
    host = [surf16, rgba16, surf8, rgb8]
    dev = [torch.from_numpy(a).cuda() for a in host]
    torch.cuda.synchronize()

    def view(k, v):
        a = host[k]
        off = v.__array_interface__["data"][0] - a.__array_interface__["data"][0]
        h, w = v.shape[:2]
        return (dev[k].data_ptr() + off, w, h, RGB if v.ndim == 3 else GRAY, D16 if v.dtype == np.uint16 else D8, v.strides[0], v.strides[1],
                v.strides[2] if v.ndim == 3 else 0)

    crops = []
    for i in range(12):
        h, w = 120 + i % 11, 130 - (3 * i) % 11 - i // 11
        y, x = int(rng.integers(0, 300 - h)), int(rng.integers(0, 700 - w))
        crops.append(surf16[y:y + h, x:x + w])
    assert len({c.shape for c in crops}) == 12 and all(120 <= s <= 130 for c in crops for s in c.shape)
    as_rgb = [rgba16[0:60, 0:90, :3], rgba16[3:64, 100:195, :3], rgba16[1:62, 5:99, :3]]
    pairs = [(0, c) for c in crops] + [(1, v) for v in as_rgb] + [(2, surf8[7:100, 13:200]), (3, rgb8)]
    pairs = [pairs[i] for i in rng.permutation(len(pairs))]
    dense = [np.ascontiguousarray(v) for _, v in pairs]
    cap = sum(a.nbytes * 5 // 4 + 96 for a in dense) + 4096
    e = _encoder()
    try:
        out = torch.zeros(cap, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        st0, vs0 = e.stats(), e.view_stats()
        offs, lens = e.compress_views_device([view(k, v) for k, v in pairs], out.data_ptr(), cap)
        st1, vs1 = e.stats(), e.view_stats()
        got = out.cpu().numpy()
        _check_all([got[int(o):int(o) + int(n)].tobytes() for o, n in zip(offs, lens)], dense, oracle, "views16")
        assert vs1["views"] - vs0["views"] == len(pairs)
        assert vs1["gathered"] - vs0["gathered"] == len(crops) + len(as_rgb), (vs0, vs1)
        assert vs1["in_place"] - vs0["in_place"] == 1 and vs1["dense"] - vs0["dense"] == 1, (vs0, vs1)
        assert vs1["bytes_staged"] - vs0["bytes_staged"] == sum(v.size * 2 for v in crops + as_rgb), (vs0, vs1)
        assert st1["submissions"] - st0["submissions"] <= 4, (st0, st1)
    finally:
        e.close()


@pytest.mark.gpu
def test_one_shape_keeps_its_path16(oracle):
    """6 gray16 images of one shape and 2 of a shape far outside their bucket: two submissions, through the uniform path."""
    rng = np.random.default_rng(137)
    imgs = [_content(rng, 90, 100, i) for i in range(6)] + [_content(rng, 300, 310, i) for i in range(2)]
    imgs = [imgs[i] for i in rng.permutation(len(imgs))]
    e = _encoder()
    try:
        before = e.stats()["submissions"]
        got = e.compress_images(imgs)
        assert e.stats()["submissions"] - before == 2, e.stats()
        _check_all(got, imgs, oracle, "oneshape16")
    finally:
        e.close()


@pytest.mark.gpu
def test_stage_timers_in_a_mixed_sub_batch16(oracle):
    """With profiling on, a mixed 16-bit sub-batch reports its span and the 16-bit stages' times, and the streams are right."""
    rng = np.random.default_rng(141)
    imgs = [_content(rng, 70 + i, 80 - i, i, True) for i in range(5)]
    assert _one_bucket(imgs)
    e = _encoder()
    try:
        e.set_profiling(True)
        before = e.stats()["submissions"]
        got = e.compress_images(imgs)
        assert e.stats()["submissions"] - before == 1, e.stats()
        ms = e.stage_ms()
        assert e.span_ms() > 0 and all(ms[k] > 0 for k in ("planes", "wide_keys", "wide_sort", "wide_chains", "lengths", "pack")), (e.span_ms(), ms)
        _check_all(got, imgs, oracle, "timers16")
    finally:
        e.close()
