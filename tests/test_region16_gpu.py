"""Regions of 16-bit streams through the version-2 restart index on the GPU: felics_decompress_regions_device_indexed16 (a wave per
needed segment, k_decode16_region) against numpy crops of the originals, its counters against the planner and the index's directory,
the full-frame region against felics_decompress_batch_device_indexed16 on the same buffers, the device against the host model under
corruption, passes, the epoch wrap it shares with the full call, empty regions, a plan with a hole, the refusals before a launch."""
import contextlib
import os
import re
import struct

import numpy as np
import pytest

from tests import index16_common as ic
from tests import region_common as rc

pytestmark = pytest.mark.gpu

POISON = 0xA5
SHAPES = ((100, 100), (4096, 3), (8200, 2), (1, 9000), (4097, 1), (64, 64))
DEC16_EPOCH_LAST = 0xFFFFFFF0  # felics_epochs.h: the dense tables are cleared once the counter has passed this


@pytest.fixture(scope="module")
def enc():
    import felics_amd

    e = felics_amd.Encoder(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def cases(oracle):
    """name -> (frame, oracle stream, index at 4096) of the index16_common cases these tests use: computed once"""
    from felics_amd import api

    out = {}
    for name in ("alias", "spikes", "chroma", "100x100_rgb"):
        img = ic.cases()[name][0]
        stream = oracle.compress(img)
        out[name] = (img, stream, api.index16_build(stream, 4096))
    return out


@contextlib.contextmanager
def _env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    try:
        os.environ.update({k: str(v) for k, v in kv.items()})
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


class Device:
    """16-bit streams of one shape and their version-2 indexes in device memory"""

    def __init__(self, streams, indexes):
        import torch

        self.blob, self.offs, self.lens = ic.pack(streams, 16)
        self.iblob, self.ioffs, self.ilens = ic.pack(indexes, 64)
        self.d_in = torch.from_numpy(np.frombuffer(self.blob, dtype=np.uint8).copy()).cuda()
        self.d_idx = torch.from_numpy(np.frombuffer(self.iblob, dtype=np.uint8).copy()).cuda()
        torch.cuda.synchronize()
        assert self.d_idx.data_ptr() % 64 == 0

    def regions(self, enc, requests, planes, guard=256, expect=None, cap=None, idx_shift=0, px_shift=0):
        """requests: (stream, x, y, w, h) each -> (status, crops as flat uint16 arrays, out_offsets); the poisoned bands in front of
        the first crop and behind the last one must be intact and d_index unchanged.  expect: the code the call must raise."""
        import torch

        import felics_amd

        sizes = [r[3] * r[4] * planes * 2 for r in requests]
        total = sum(sizes)
        d_px = torch.full((guard + max(total, 16) + guard,), POISON, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        assert (d_px.data_ptr() + guard) % 2 == 0
        args = (self.d_in.data_ptr(), self.offs, self.lens, self.d_idx.data_ptr(), [o + idx_shift for o in self.ioffs], self.ilens, requests,
                d_px.data_ptr() + guard + px_shift, total if cap is None else cap)
        out_offsets = None
        if expect is None:
            _, status, out_offsets = enc.decompress_regions_device_indexed16(*args)
        else:
            with pytest.raises(felics_amd.FelicsError) as ei:
                enc.decompress_regions_device_indexed16(*args)
            assert ei.value.code == expect
            status = ei.value.status
        host = d_px.cpu().numpy()
        assert (host[:guard] == POISON).all() and (host[guard + total:] == POISON).all()
        assert self.d_idx.cpu().numpy().tobytes() == self.iblob
        starts = [0] + list(np.cumsum(sizes))
        crops = [host[guard + a:guard + a + n].view(np.uint16) for a, n in zip(starts, sizes)]
        if out_offsets is not None:  # in bytes, back to back in request order
            assert list(out_offsets) == starts[:-1]
        return status, crops, out_offsets

    def frames(self, enc, frame_bytes, guard=256, expect=None):
        """felics_decompress_batch_device_indexed16 over the same device streams and indexes -> (status, frames as flat uint16 arrays)"""
        import torch

        import felics_amd

        n = len(self.offs)
        d_px = torch.full((guard + frame_bytes * n + guard,), POISON, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        args = (self.d_in.data_ptr(), self.offs, self.lens, self.d_idx.data_ptr(), self.ioffs, self.ilens, d_px.data_ptr() + guard, frame_bytes * n)
        if expect is None:
            _, status = enc.decompress_batch_device_indexed16(*args)
        else:
            with pytest.raises(felics_amd.FelicsError) as ei:
                enc.decompress_batch_device_indexed16(*args)
            assert ei.value.code == expect
            status = ei.value.status
        host = d_px.cpu().numpy()
        assert (host[:guard] == POISON).all() and (host[guard + frame_bytes * n:] == POISON).all()
        return status, [host[guard + i * frame_bytes:guard + (i + 1) * frame_bytes].view(np.uint16) for i in range(n)]


def _plan(w, h, seg, planes, requests, indexes=None):
    """What the format and the planner's rule say a call does, by marking pixels: the four counters of felics_region16_stats, the
    items per request and (with the indexes) the state rows its waves load -- a wave loads its checkpoint's rows, all of them."""
    k = (w * h + seg - 1) // seg
    walked = pixels = rows = 0
    items = []
    for r in requests:
        segs = rc.needed_by_marking(w, h, seg, r[1:]) if r[3] * r[4] else []
        items.append(planes * len(segs) if segs else 1)
        walked += planes * len(segs)
        last = (r[2] + r[4] - 1) * w + r[1] + r[3]
        pixels += planes * sum(min(w * h, (j + 1) * seg, last) - j * seg for j in segs)
        if indexes is not None:
            lay = ic.Layout16(indexes[r[0]])
            rows += sum(lay.get(c, j)[2] for c in range(planes) for j in segs)
    return {"regions": len(requests), "segments_walked": walked, "segments_skipped": len(requests) * planes * k - walked, "pixels_walked": pixels,
            "rows_loaded": rows}, items


def _delta(before, after):
    return {k: after[k] - before[k] for k in after}


def _shape_cases():
    for w, h in SHAPES:
        for rgb in (0, 1):
            for seg in (ic.SEGMENTS if (w, h) in ((100, 100), (8200, 2)) else ic.SEGMENTS[:1]):
                yield w, h, rgb, seg


@pytest.mark.parametrize("w,h,rgb,seg", list(_shape_cases()))
def test_regions_of_three_streams(enc, oracle, w, h, rgb, seg):
    """One call per (shape, colour, segment size): three streams of different content, all of the shape's windows (fixed, edge,
    empty and six random ones) spread over them.  Every crop is the numpy crop of the original, the offsets are back to back, the
    statuses 0, the counters those of the planner and of the indexes' directories.  Then every fixed window in a call of its own: a
    poisoned band right behind that crop."""
    from felics_amd import api

    imgs = [ic.noise(w, h, rgb, 10, 2000 + 10 * k + w) for k in range(3)]
    streams = [oracle.compress(im) for im in imgs]
    indexes = [api.index16_build(s, seg) for s in streams]
    dev = Device(streams, indexes)
    planes = 3 if rgb else 1
    windows = rc.all_regions(w, h, 6, seed=3)
    requests = [(k % 3,) + win for k, win in enumerate(windows)] + [((k + 1) % 3,) + win for k, win in enumerate(rc.FIXED.get((w, h), []))]
    before = enc.region16_stats()
    others = (enc.region_stats(), enc.index16_stats())
    status, crops, _ = dev.regions(enc, requests, planes)
    d = _delta(before, enc.region16_stats())
    assert (status == 0).all(), status
    for r, got in zip(requests, crops):
        want = rc.crop(imgs[r[0]], r[1:])
        assert (got.reshape(want.shape) == want).all(), (w, h, rgb, seg, r)
    want, _ = _plan(w, h, seg, planes, requests, indexes)
    print("counters:", d)
    assert d.pop("passes") >= 1 and d == want
    assert want["segments_walked"] == planes * sum(len(api.region_segments(w, h, seg, *r[1:])) for r in requests)
    assert others == (enc.region_stats(), enc.index16_stats())  # the 8-bit region call's and the full call's counters are theirs alone
    for win in rc.FIXED.get((w, h), []):
        status, crops, _ = dev.regions(enc, [(2,) + win], planes)
        want = rc.crop(imgs[2], win)
        assert status[0] == 0 and (crops[0].reshape(want.shape) == want).all(), (w, h, rgb, seg, win)


def _three(cases, name, oracle):
    """the case's stream between two streams of its own shape and other content (the frame upside down)"""
    from felics_amd import api

    img, stream, index = cases[name]
    other = img[::-1].copy()
    s2 = oracle.compress(other)
    i2 = api.index16_build(s2, 4096)
    return [other, img, other], [s2, stream, s2], [i2, index, i2]


@pytest.mark.parametrize("name", ("alias", "spikes", "chroma", "100x100_rgb"))
def test_full_frame_region_equals_indexed_decode(enc, oracle, cases, name):
    """k_decode16_region and k_decode16_seg are two sinks of one walk (decode16_from_checkpoint), so the full-frame region of every
    stream is felics_decompress_batch_device_indexed16's frame: both calls on the same device streams and indexes -- the same words,
    the same statuses, both the original frames.  Once more with stream 1's index carrying bit_offset_plus_1 (segment (0, 0) no
    longer ends on checkpoint (0, 1)): both calls raise FELICS_E_INVALID_INDEX with statuses [0, E_INVALID_INDEX, 0], and streams 0
    and 2 are exact in both."""
    imgs, streams, indexes = _three(cases, name, oracle)
    h, w = imgs[0].shape[:2]
    planes = 3 if imgs[0].ndim == 3 else 1
    for corrupt in (False, True):
        idx = list(indexes)
        if corrupt:  # (ic.corruptions()' bit_offset_plus_1, written out: `spikes` has too few rows for that list's other entries)
            lay = ic.Layout16(indexes[1])
            assert lay.k >= 2
            at = lay.entry(0, 1)
            idx[1] = indexes[1][:at] + struct.pack("<Q", lay.get(0, 1)[0] + 1) + indexes[1][at + 8:]
        dev = Device(streams, idx)
        expect = ic.E_INVALID_INDEX if corrupt else None
        want = [0, ic.E_INVALID_INDEX, 0] if corrupt else [0, 0, 0]
        rstatus, crops, _ = dev.regions(enc, [(s, 0, 0, w, h) for s in range(3)], planes, expect=expect)
        fstatus, frames = dev.frames(enc, imgs[0].nbytes, expect=expect)
        assert list(rstatus) == want and list(fstatus) == want, (name, corrupt)
        for s in range(3):
            if want[s] == 0:
                assert (crops[s] == frames[s]).all() and (crops[s] == imgs[s].reshape(-1)).all(), (name, corrupt, s)


@pytest.mark.parametrize("what", ("bit_offset_plus_1", "n_rows_plus_1", "contexts_swapped", "co_sample_70000"))
def test_device_equals_host_model_under_corruption(enc, oracle, cases, what):
    """Three 100 x 100 RGB16 streams, stream 1 beside a corrupted index: every request's status is
    felics_decompress_region_indexed16's on the same pair, both outcomes occur on stream 1, streams 0 and 2 are all clean, and every
    request with status 0 is exact."""
    import felics_amd
    from felics_amd import api

    img, stream, index = cases["100x100_rgb"]
    imgs = [ic.noise(100, 100, 1, 10, 61), img, ic.noise(100, 100, 1, 10, 62)]
    streams = [oracle.compress(imgs[0]), stream, oracle.compress(imgs[2])]
    indexes = [api.index16_build(streams[0], 4096), ic.corruptions(index)[what], api.index16_build(streams[2], 4096)]
    dev = Device(streams, indexes)
    requests = [(s,) + win for win in rc.all_regions(100, 100, 8) for s in range(3)]

    def host_code(r):
        try:
            api.decompress_region_indexed16(streams[r[0]], indexes[r[0]], *r[1:])
        except (felics_amd.FelicsError, felics_amd.DecompressionError) as e:
            return e.code
        return 0

    want = [host_code(r) for r in requests]
    assert ic.E_INVALID_INDEX in want and any(c == 0 and r[0] == 1 and r[3] * r[4] for c, r in zip(want, requests))
    assert all(c == 0 for c, r in zip(want, requests) if r[0] != 1)
    first = next(c for c in want if c)
    status, crops, _ = dev.regions(enc, requests, 3, expect=first)
    print("stream 1, host:", [c for c, r in zip(want, requests) if r[0] == 1], "device:", [int(c) for c, r in zip(status, requests) if r[0] == 1])
    assert list(status) == want
    for r, got, code in zip(requests, crops, want):
        if code == 0:
            assert (got.reshape(rc.crop(imgs[r[0]], r[1:]).shape) == rc.crop(imgs[r[0]], r[1:])).all(), r


def test_passes(enc, oracle):
    """FELICS_TEST_INDEX16_PASS = 5 on the 8200 x 2 RGB16 case: the item list runs in ceil(items / 5) passes, a pass boundary falls
    inside a region, and every word is what the call gives in one pass"""
    from felics_amd import api

    w, h, seg = 8200, 2, 4096
    imgs = [ic.noise(w, h, 1, 10, 2000 + 10 * k + w) for k in range(3)]
    streams = [oracle.compress(im) for im in imgs]
    indexes = [api.index16_build(s, seg) for s in streams]
    dev = Device(streams, indexes)
    requests = [(k % 3,) + win for k, win in enumerate(rc.all_regions(w, h, 6, seed=3))]
    want, items = _plan(w, h, seg, 3, requests, indexes)
    starts = np.cumsum([0] + items)
    assert any(a // 5 != (b - 1) // 5 for a, b in zip(starts[:-1], starts[1:]))  # a region whose items lie in two passes
    before = enc.region16_stats()
    status1, crops1, _ = dev.regions(enc, requests, 3)
    middle = enc.region16_stats()
    with _env(FELICS_TEST_INDEX16_PASS=5):
        status5, crops5, _ = dev.regions(enc, requests, 3)
    after = enc.region16_stats()
    assert (status1 == 0).all() and (status5 == 0).all()
    for r, a, b in zip(requests, crops1, crops5):
        assert (a == b).all() and (a.reshape(rc.crop(imgs[r[0]], r[1:]).shape) == rc.crop(imgs[r[0]], r[1:])).all(), r
    total = int(starts[-1])
    assert total > 10 and after["passes"] - middle["passes"] == (total + 4) // 5
    assert 1 <= middle["passes"] - before["passes"] < (total + 4) // 5
    d1, d5 = _delta(before, middle), _delta(middle, after)
    d1.pop("passes"), d5.pop("passes")
    assert d1 == want and d5 == want


def test_epoch_wrap_shared_with_the_full_call(oracle, cases, capfd):
    """A context whose dense-table counter starts two passes short of 0xFFFFFFF0: full indexed16 calls and region calls take turns
    on `alias` (three items a call at most, one pass each; the first call is the full one, so the table buffer never grows again).
    Both draw their epochs from the one counter -- last + 1, + 4, + 7, then a clear and 1, 4, 7 -- and every call is exact."""
    import felics_amd

    imgs, streams, indexes = _three(cases, "alias", oracle)
    imgs, streams, indexes = imgs[1:2], streams[1:2], indexes[1:2]
    img = imgs[0]
    h, w = img.shape
    last = DEC16_EPOCH_LAST - 6
    with _env(FELICS_TEST_DECODE16_EPOCH=hex(last), FELICS_TRACE_EPOCHS="1"):
        e = felics_amd.Encoder(0)
    try:
        dev = Device(streams, indexes)
        windows = [(0, 0, w, h), (3, 60, 40, 30), (0, 0, w, h)]  # all three segments; segments 0 and 1; all three
        capfd.readouterr()
        for win in windows:
            status, frames = dev.frames(e, img.nbytes)
            assert status[0] == 0 and (frames[0].reshape(img.shape) == img).all()
            status, crops, _ = dev.regions(e, [(0,) + win], 1)
            assert status[0] == 0 and (crops[0].reshape(rc.crop(img, win).shape) == rc.crop(img, win)).all(), win
    finally:
        e.close()
    got = [(int(m.group(1), 16), m.group(2) == "1") for m in
           (re.fullmatch(r"\[felics\] decode16 epoch 0x([0-9a-f]+) clear ([01])", line) for line in capfd.readouterr().err.splitlines()) if m]
    assert got == [(last + 1, False), (last + 4, False), (last + 7, False), (1, True), (4, False), (7, False)]


def test_empty_regions_write_nothing(enc, oracle):
    """empty images have empty regions only, and an image with pixels may be asked for none: status 0, not a byte written, no
    segment walked"""
    from felics_amd import api

    for w, h in ((0, 5), (5, 0), (64, 65)):
        for rgb in (0, 1):
            imgs = [np.zeros((h, w, 3) if rgb else (h, w), np.uint16) + 7, ic.noise(w, h, rgb, 10, 5)]
            streams = [oracle.compress(im) for im in imgs]
            dev = Device(streams, [api.index16_build(s, 4096) for s in streams])
            requests = [(k % 2,) + win for k, win in enumerate(rc.edges(w, h)) if win[2] * win[3] == 0]
            assert len(requests) >= 3
            before = enc.region16_stats()
            status, _, offs = dev.regions(enc, requests, 3 if rgb else 1)  # (total = 0: the whole buffer is guard)
            d = _delta(before, enc.region16_stats())
            assert (status == 0).all() and (offs == 0).all()
            assert (d["regions"], d["segments_walked"], d["pixels_walked"], d["rows_loaded"]) == (len(requests), 0, 0, 0)


def test_plan_with_a_hole_counts(enc, oracle):
    """(5000, 0, 100, 2) of an 8200 x 2 gray16 frame alone: segments 1 and 3 are walked, 0, 2 and 4 are not"""
    from felics_amd import api

    img = ic.noise(8200, 2, 0, 10, 77)
    stream = oracle.compress(img)
    dev = Device([stream], [api.index16_build(stream, 4096)])
    before = enc.region16_stats()
    status, crops, _ = dev.regions(enc, [(0, 5000, 0, 100, 2)], 1)
    d = _delta(before, enc.region16_stats())
    assert status[0] == 0 and (crops[0].reshape(2, 100) == img[:, 5000:5100]).all()
    # segment 1 from pixel 4096 to its end 8192, segment 3 from 12288 to the pixel behind the region's last one, 8200 + 5100
    assert (d["regions"], d["segments_walked"], d["segments_skipped"], d["pixels_walked"]) == (1, 2, 3, 4096 + (13300 - 12288))
    assert d["passes"] == 1


def test_refusals_before_launch(enc, oracle):
    import torch

    from felics_amd import api

    imgs = [ic.noise(64, 65, 0, 10, 90 + k) for k in range(2)]
    streams = [oracle.compress(im) for im in imgs]
    indexes = [api.index16_build(s, 4096) for s in streams]
    dev = Device(streams, indexes)
    good = (1, 3, 3, 10, 10)
    before = enc.region16_stats()
    for bad in ((0, 60, 0, 5, 1), (0, 0, 64, 1, 2), (0, 0xFFFFFFFF, 0, 2, 1), (2, 0, 0, 1, 1), (0xFFFFFFFF, 0, 0, 0, 0)):
        status, _, _ = dev.regions(enc, [good, bad], 1, expect=rc.E_INVALID_ARGUMENT)  # (not a byte written: the guards are everything)
        assert (status == rc.E_INVALID_ARGUMENT).all(), bad
    status, _, _ = dev.regions(enc, [good, good], 1, expect=rc.E_BUFFER_TOO_SMALL, cap=399)
    assert (status == rc.E_BUFFER_TOO_SMALL).all()
    status, _, _ = dev.regions(enc, [good], 1, expect=rc.E_INVALID_ARGUMENT, idx_shift=16)  # index offsets that are no multiple of 64
    assert (status == rc.E_INVALID_ARGUMENT).all()
    status, _, _ = dev.regions(enc, [good], 1, expect=rc.E_INVALID_ARGUMENT, px_shift=1, cap=200)  # d_pixels at an odd address
    assert (status == rc.E_INVALID_ARGUMENT).all()
    # an 8-bit batch: felics_decompress_regions_device_indexed's business
    s8 = oracle.compress((imgs[0] >> 2).astype(np.uint8))
    status, _, _ = Device([s8, s8], indexes).regions(enc, [good, (0, 0, 0, 0, 0)], 1, expect=ic.E_UNSUPPORTED)
    assert (status == ic.E_UNSUPPORTED).all()
    # the smallest width past the LDS limit (512 rows of 16 words, 512 tags, two int32 rows padded to whole blocks of 64), H = 1: no
    # host fallback in this call, while the host model decodes it
    lds = lambda w: 512 * 64 + 512 * 4 + 2 * 4 * ((w + 63) // 64 * 64)
    assert lds(16128) <= 160 * 1024 < lds(16129)
    wide = (np.arange(16129, dtype=np.uint32) * 5 % 65536).astype(np.uint16).reshape(1, 16129)
    sw = oracle.compress(wide)
    iw = api.index16_build(sw, 4096)
    assert (api.decompress_region_indexed16(sw, iw, 16120, 0, 9, 1) == wide[:, 16120:]).all()
    status, _, _ = Device([sw], [iw]).regions(enc, [(0, 16120, 0, 9, 1)], 1, expect=ic.E_UNSUPPORTED)
    assert (status == ic.E_UNSUPPORTED).all()
    assert enc.region16_stats() == before  # refused calls count nothing
    status, crops, _ = dev.regions(enc, [good], 1)
    assert status[0] == 0 and (crops[0].reshape(10, 10) == imgs[1][3:13, 3:13]).all()
    # refused like the other synchronous entry points while a ticket is outstanding
    d_in = torch.from_numpy((imgs[0] >> 2).astype(np.uint8)).cuda()
    d_out = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    t = enc.submit_batch_device(d_in.data_ptr(), 1, 64, 65, 0, 0, d_out.data_ptr(), d_out.numel())
    try:
        status, _, _ = dev.regions(enc, [good], 1, expect=rc.E_INVALID_ARGUMENT)
    finally:
        enc.wait_batch(t)
    status, _, _ = dev.regions(enc, [good], 1)
    assert status[0] == 0
