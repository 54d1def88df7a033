"""Regions through the restart index on the GPU: felics_decompress_regions_device_indexed (a wave per needed segment,
k_decode8_region) against numpy crops of the originals, its counters, the device against the host model under corruption, its
refusals before the launch, and cfelics --index against felics_index_build."""
import os
import subprocess

import numpy as np
import pytest

from tests import index_common as ic
from tests import region_common as rc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
BUILD = os.path.join(ROOT, "felics_amd", "_build")
POISON = 0xA5


@pytest.fixture(scope="module")
def enc():
    import felics_amd

    e = felics_amd.Encoder(0)
    yield e
    e.close()


class Device:
    """streams and their indexes of one shape in device memory"""

    def __init__(self, streams, indexes):
        import torch

        blob, self.offs, self.lens = ic.pack_streams(streams)
        self.stride = max((max(len(i) for i in indexes) + 15) // 16 * 16, 64)
        iblob = b"".join(i + bytes(self.stride - len(i)) for i in indexes)
        self.d_in = torch.from_numpy(np.frombuffer(blob, dtype=np.uint8).copy()).cuda()
        self.d_idx = torch.from_numpy(np.frombuffer(iblob, dtype=np.uint8).copy()).cuda()
        torch.cuda.synchronize()

    def regions(self, enc, requests, planes, guard=256, expect=None, cap=None, stride=None):
        """requests: (stream, x, y, w, h) each -> (status, crops as flat uint8 arrays, out_offsets); the poisoned bands in front of
        the first crop and behind the last one must be intact.  expect: the code the call must raise."""
        import torch

        import felics_amd

        total = sum(r[3] * r[4] * planes for r in requests)
        d_px = torch.full((guard + max(total, 16) + guard,), POISON, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        args = (self.d_in.data_ptr(), self.offs, self.lens, self.d_idx.data_ptr(), self.stride if stride is None else stride, requests,
                d_px.data_ptr() + guard, total if cap is None else cap)
        out_offsets = None
        if expect is None:
            _, status, out_offsets = enc.decompress_regions_device_indexed(*args)
        else:
            with pytest.raises(felics_amd.FelicsError) as ei:
                enc.decompress_regions_device_indexed(*args)
            assert ei.value.code == expect
            status = ei.value.status
        host = d_px.cpu().numpy()
        assert (host[:guard] == POISON).all() and (host[guard + total:] == POISON).all()
        at, crops = 0, []
        for r in requests:
            crops.append(host[guard + at:guard + at + r[3] * r[4] * planes])
            at += r[3] * r[4] * planes
        if out_offsets is not None:  # back to back in request order
            assert list(out_offsets) == list(np.cumsum([0] + [r[3] * r[4] * planes for r in requests[:-1]]))
        return status, crops, out_offsets

    def frames(self, enc, frame_bytes, guard=256, expect=None):
        """felics_decompress_batch_device_indexed over the same device streams and indexes -> (status, frames as flat uint8
        arrays); the poisoned bands in front of the first frame and behind the last one must be intact."""
        import torch

        import felics_amd

        n = len(self.offs)
        d_px = torch.full((guard + frame_bytes * n + guard,), POISON, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        args = (self.d_in.data_ptr(), self.offs, self.lens, self.d_idx.data_ptr(), self.stride, d_px.data_ptr() + guard, frame_bytes * n)
        if expect is None:
            _, status = enc.decompress_batch_device_indexed(*args)
        else:
            with pytest.raises(felics_amd.FelicsError) as ei:
                enc.decompress_batch_device_indexed(*args)
            assert ei.value.code == expect
            status = ei.value.status
        host = d_px.cpu().numpy()
        assert (host[:guard] == POISON).all() and (host[guard + frame_bytes * n:] == POISON).all()
        return status, [host[guard + i * frame_bytes:guard + (i + 1) * frame_bytes] for i in range(n)]


def _shape_cases():
    for w, h in ic.SHAPES:
        for rgb in (0, 1):
            segs = ic.SEGMENTS if (w, h) in ((512, 256), (100, 100), (8200, 2)) else ic.SEGMENTS[:1]
            for seg in segs:
                yield w, h, rgb, seg


@pytest.mark.parametrize("w,h,rgb,seg", list(_shape_cases()))
def test_regions_of_three_streams(enc, oracle, w, h, rgb, seg):
    """One call per (shape, colour, segment size): three streams of different content, all of the shape's windows (fixed, edge,
    empty and six random ones) spread over them, so that several requests of different sizes go to one stream.  Every crop is the
    numpy crop of the original, the offsets are back to back, the statuses 0, the counters those of the planner.  Then every fixed
    window in a call of its own: a poisoned band right behind that crop."""
    from felics_amd import api

    imgs = ic.images(w, h, rgb, 3)
    streams = [oracle.compress(im) for im in imgs]
    dev = Device(streams, [api.index_build(s, seg) for s in streams])
    planes = 3 if rgb else 1
    windows = rc.all_regions(w, h, 6, seed=3)
    requests = [(k % 3,) + win for k, win in enumerate(windows)] + [((k + 1) % 3,) + win for k, win in enumerate(rc.FIXED.get((w, h), []))]
    before = enc.region_stats()
    status, crops, _ = dev.regions(enc, requests, planes)
    assert (status == 0).all(), status
    for r, got in zip(requests, crops):
        want = rc.crop(imgs[r[0]], r[1:])
        assert (got.reshape(want.shape) == want).all(), (w, h, rgb, seg, r)
    after = enc.region_stats()
    k = (w * h + seg - 1) // seg
    walked = planes * sum(len(api.region_segments(w, h, seg, *r[1:])) for r in requests)
    assert after["regions"] - before["regions"] == len(requests)
    assert after["segments_walked"] - before["segments_walked"] == walked
    assert after["segments_skipped"] - before["segments_skipped"] == len(requests) * planes * k - walked
    for win in rc.FIXED.get((w, h), []):
        status, crops, _ = dev.regions(enc, [(2,) + win], planes)
        want = rc.crop(imgs[2], win)
        assert status[0] == 0 and (crops[0].reshape(want.shape) == want).all(), (w, h, rgb, seg, win)


@pytest.mark.parametrize("w,h,rgb,corrupt", [(100, 100, 1, None), (4096, 3, 0, None), (100, 100, 1, "offset_plus_1")])
def test_full_frame_region_equals_indexed_decode(enc, oracle, w, h, rgb, corrupt):
    """k_decode8_region and k_decode8_seg are two sinks of one walk (decode8_from_checkpoint), so the full-frame region of every
    stream is felics_decompress_batch_device_indexed's frame: three streams at segment 4096, both calls on the same device streams
    and indexes -- the same bytes, the same per-stream statuses, both the original frames, the guard bands intact on both.  With
    stream 1's index corrupted (the end check of segment (0, 0)) both calls raise FELICS_E_INVALID_INDEX with statuses
    [0, E_INVALID_INDEX, 0], and streams 0 and 2 are exact in both."""
    from felics_amd import api

    imgs = ic.images(w, h, rgb, 3)
    streams = [oracle.compress(im) for im in imgs]
    indexes = [api.index_build(s, 4096) for s in streams]
    if corrupt:
        indexes[1] = ic.corruptions(indexes[1])[corrupt]
    dev = Device(streams, indexes)
    planes = 3 if rgb else 1
    expect = ic.E_INVALID_INDEX if corrupt else None
    want = [0, ic.E_INVALID_INDEX, 0] if corrupt else [0, 0, 0]
    rstatus, crops, _ = dev.regions(enc, [(s, 0, 0, w, h) for s in range(3)], planes, expect=expect)
    fstatus, frames = dev.frames(enc, w * h * planes, expect=expect)
    assert list(rstatus) == want and list(fstatus) == want
    for s in range(3):
        if want[s] == 0:
            assert (crops[s] == frames[s]).all(), s
            assert (crops[s] == imgs[s].reshape(-1)).all() and (frames[s] == imgs[s].reshape(-1)).all(), s


def test_empty_regions_write_nothing(enc, oracle):
    """empty images have empty regions only, and an image with pixels may be asked for none: status 0, not a byte written"""
    from felics_amd import api

    for w, h in ((0, 5), (5, 0), (64, 65)):
        for rgb in (0, 1):
            imgs = ic.images(w, h, rgb, 2)
            streams = [oracle.compress(im) for im in imgs]
            dev = Device(streams, [api.index_build(s, 4096) for s in streams])
            requests = [(k % 2,) + win for k, win in enumerate(rc.edges(w, h)) if win[2] * win[3] == 0]
            assert len(requests) >= 3
            status, _, offs = dev.regions(enc, requests, 3 if rgb else 1)  # (total = 0: the whole buffer is guard)
            assert (status == 0).all() and (offs == 0).all()


def test_plan_with_a_hole_counts(enc, oracle):
    """(5000, 0, 100, 2) of an 8200 x 2 gray frame alone: segments 1 and 3 are walked, 0, 2 and 4 are not"""
    from felics_amd import api

    img = ic.images(8200, 2, 0, 1)[0]
    stream = oracle.compress(img)
    dev = Device([stream], [api.index_build(stream, 4096)])
    before = enc.region_stats()
    status, crops, _ = dev.regions(enc, [(0, 5000, 0, 100, 2)], 1)
    after = enc.region_stats()
    assert status[0] == 0 and (crops[0].reshape(2, 100) == img[:, 5000:5100]).all()
    delta = {k: after[k] - before[k] for k in after}
    # segment 1 from pixel 4096 to its end 8192, segment 3 from 12288 to the pixel behind the region's last one, 8200 + 5100
    assert delta == {"regions": 1, "segments_walked": 2, "segments_skipped": 3, "pixels_walked": 4096 + (13300 - 12288)}


@pytest.mark.parametrize("name", ("co_300", "offset_plus_1"))
def test_device_equals_host_model_under_corruption(enc, oracle, name):
    """Three 100 x 100 RGB streams, stream 1 beside a corrupted index: every request's status is felics_decompress_region_indexed's
    on the same pair (refused iff the region needs the damaged segment or walks segment (0, 0) to its end), every request with
    status 0 is exact -- those on the clean streams all are."""
    import felics_amd
    from felics_amd import api

    imgs = ic.images(100, 100, 1, 3)
    streams = [oracle.compress(im) for im in imgs]
    indexes = [api.index_build(s, 4096) for s in streams]
    indexes[1] = ic.corruptions(indexes[1])[name]
    dev = Device(streams, indexes)
    windows = rc.all_regions(100, 100, 8, seed=4)
    requests = [(s,) + win for win in windows for s in range(3)]

    def host_code(r):
        try:
            api.decompress_region_indexed(streams[r[0]], indexes[r[0]], *r[1:])
        except felics_amd.FelicsError as e:
            return e.code
        return 0

    want = [host_code(r) for r in requests]
    assert ic.E_INVALID_INDEX in want and any(c == 0 and r[0] == 1 and r[3] * r[4] for c, r in zip(want, requests))
    assert all(c == 0 for c, r in zip(want, requests) if r[0] != 1)
    status, crops, _ = dev.regions(enc, requests, 3, expect=ic.E_INVALID_INDEX)
    assert list(status) == want
    for r, got, code in zip(requests, crops, want):
        if code == 0:
            assert (got.reshape(rc.crop(imgs[r[0]], r[1:]).shape) == rc.crop(imgs[r[0]], r[1:])).all(), r


def test_refusals_before_launch(enc, oracle):
    from felics_amd import api

    imgs = ic.images(64, 65, 0, 2)
    streams = [oracle.compress(im) for im in imgs]
    indexes = [api.index_build(s, 4096) for s in streams]
    dev = Device(streams, indexes)
    good = (1, 3, 3, 10, 10)
    before = enc.region_stats()
    for bad in ((0, 60, 0, 5, 1), (0, 0, 64, 1, 2), (0, 0xFFFFFFFF, 0, 2, 1), (2, 0, 0, 1, 1), (0xFFFFFFFF, 0, 0, 0, 0)):
        status, _, _ = dev.regions(enc, [good, bad], 1, expect=rc.E_INVALID_ARGUMENT)  # (not a byte written: the guards are everything)
        assert (status == rc.E_INVALID_ARGUMENT).all(), bad
    status, _, _ = dev.regions(enc, [good, good], 1, expect=rc.E_BUFFER_TOO_SMALL, cap=199)
    assert (status == rc.E_BUFFER_TOO_SMALL).all()
    status, _, _ = dev.regions(enc, [good], 1, expect=rc.E_INVALID_ARGUMENT, stride=dev.stride + 8)
    assert (status == rc.E_INVALID_ARGUMENT).all()
    assert enc.region_stats() == before  # refused calls count nothing
    status, crops, _ = dev.regions(enc, [good], 1)
    assert status[0] == 0 and (crops[0].reshape(10, 10) == imgs[1][3:13, 3:13]).all()
    # 16-bit streams have no index
    s16 = oracle.compress(np.arange(64 * 65, dtype=np.uint16).reshape(65, 64))
    status, _, _ = Device([s16, s16], indexes).regions(enc, [good, (0, 0, 0, 0, 0)], 1, expect=ic.E_UNSUPPORTED)
    assert (status == ic.E_UNSUPPORTED).all()
    # the smallest width past the LDS limit, H = 1: no host fallback in this call
    w = next(w for w in range(39000, 41000) if 256 * 24 + 2 * 2 * ((w + 63) // 64 * 64) > 160 * 1024)
    wide = (np.arange(w, dtype=np.uint32) // 3 % 256).astype(np.uint8).reshape(1, w)
    sw = oracle.compress(wide)
    iw = api.index_build(sw, 4096)
    assert (api.decompress_region_indexed(sw, iw, w - 9, 0, 9, 1) == wide[:, w - 9:]).all()  # the host model takes it
    status, _, _ = Device([sw], [iw]).regions(enc, [(0, w - 9, 0, 9, 1)], 1, expect=ic.E_UNSUPPORTED)
    assert (status == ic.E_UNSUPPORTED).all()
    # refused like the other synchronous entry points while a ticket is outstanding
    import torch

    d_in = torch.from_numpy(imgs[0]).cuda()
    d_out = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    t = enc.submit_batch_device(d_in.data_ptr(), 1, 64, 65, 0, 0, d_out.data_ptr(), d_out.numel())
    status, _, _ = dev.regions(enc, [good], 1, expect=rc.E_INVALID_ARGUMENT)
    enc.wait_batch(t)
    status, _, _ = dev.regions(enc, [good], 1)
    assert status[0] == 0


def test_cfelics_index(tmp_path, oracle):
    """cfelics --index writes felics_index_build's bytes of the stream it wrote (64 x 65 gray8, --segment 4096; 65536 by default)
    and refuses a 16-bit input with the library's message; at its default on a 1024 x 1024 gray original of tests/golden/suite/ (K = 16,
    16 tiles per interval) the stream is the committed one and the index felics_index_build's."""
    import glob

    from PIL import Image

    from felics_amd import api

    img = ic.images(64, 65, 0, 1)[0]
    src = str(tmp_path / "in.tiff")
    Image.fromarray(img).save(src)
    out, idx = tmp_path / "out.felics", tmp_path / "out.idx"
    cfelics = os.path.join(BUILD, "cfelics")
    r = subprocess.run([cfelics, "-i", src, "-o", str(out), "--index", str(idx), "--segment", "4096"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "Compressing 8-bit grayscale image...", r.stdout + r.stderr
    assert out.read_bytes() == oracle.compress(img)
    assert idx.read_bytes() == api.index_build(out.read_bytes(), 4096)
    r = subprocess.run([cfelics, "-i", src, "-o", str(out), "--index", str(idx)], capture_output=True, text=True)
    assert r.returncode == 0 and idx.read_bytes() == api.index_build(out.read_bytes(), 65536)
    r = subprocess.run([cfelics, "-i", src, "-o", str(out), "--index", str(idx), "--segment", "5000"], capture_output=True, text=True)
    assert r.returncode == 1 and api.lib().felics_strerror(rc.E_INVALID_ARGUMENT).decode() in r.stdout
    out16, idx16 = tmp_path / "a.felics", tmp_path / "a.idx"
    r = subprocess.run([cfelics, "-i", os.path.join(GOLDEN, "aerial.tiff"), "-o", str(out16), "--index", str(idx16)], capture_output=True, text=True)
    assert r.returncode == 1 and r.stdout.splitlines()[0] == "Compressing 16-bit grayscale image..."
    assert r.stdout.splitlines()[1].startswith("Cannot compress image: " + api.lib().felics_strerror(ic.E_UNSUPPORTED).decode())
    assert not out16.exists() and not idx16.exists()
    r = subprocess.run([cfelics, "-i", src, "-o", str(out), "--segment", "4096"], capture_output=True, text=True)
    assert r.returncode == 2  # a usage error: no index named
    # the first 1024 x 1024 gray original of the suite, chosen the way test_index_gpu.py::test_suite_originals_at_65536 does
    for path in sorted(glob.glob(os.path.join(GOLDEN, "suite", "*.felics"))):
        real = np.array(Image.open(path[:-len(".felics")]))
        if real.dtype == np.uint8 and real.shape == (1024, 1024):
            break
    else:
        pytest.fail("no 1024 x 1024 gray original in tests/golden/suite")
    big, bigidx = tmp_path / "big.felics", tmp_path / "big.idx"
    r = subprocess.run([cfelics, "-i", path[:-len(".felics")], "-o", str(big), "--index", str(bigidx)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert big.read_bytes() == open(path, "rb").read(), path
    got, ref = bigidx.read_bytes(), api.index_build(big.read_bytes(), 65536)
    assert ic.Layout(ref).k == 16 and ic.Layout(ref).seg == 65536
    d = ic.first_difference(got, ref)
    assert len(got) == len(ref) and d is None, (path, d, ic.where_in_index(ref, d))
