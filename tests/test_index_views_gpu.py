"""Indexed decode into device surfaces (felics_decompress_views_device_indexed), on the GPU.

Streams come from the CPU oracle and indexes from felics_index_build, so nothing here needs the GPU encoder.  Streams and indexes lie
between guard bytes in device memory and are compared unchanged after every call; every target is a surface of 0xA5 compared WHOLE
afterwards: the samples must be the images, every other byte must still hold 0xA5."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import index_common as ic
from tests import index_views_common as vc

pytestmark = pytest.mark.gpu
GUARD = 256


@pytest.fixture(scope="module")
def enc():
    import felics_amd

    e = felics_amd.Encoder(0)
    yield e
    e.close()


@pytest.fixture(scope="module")
def api():
    from felics_amd import api as a

    return a


@pytest.fixture(scope="module")
def cases(oracle, api):
    """(w, h, rgb) -> (image, oracle stream, {segment size: index}): computed once, read by every test"""
    out = {}
    for w, h in ic.SHAPES:
        for rgb in (0, 1):
            im = ic.images(w, h, rgb, 1)[0]
            stream = oracle.compress(im)
            out[(w, h, rgb)] = (im, stream, {seg: api.index_build(stream, seg) for seg in ic.SEGMENTS})
    return out


class Inputs:
    """Streams (at odd offsets too) and indexes (at multiples of 16, 0x5A between them) in device memory, each blob between GUARD
    bytes of 0x5A.  idx_lens may be overridden per stream (an entry of `ilens`).  check(): both buffers are what was uploaded."""

    def __init__(self, streams, indexes, ilens=None):
        import torch

        blob, self.offs = bytearray(b"\x5a" * GUARD), []
        for i, s in enumerate(streams):
            blob += b"\x5a" * (i % 3)
            self.offs.append(len(blob) - GUARD)
            blob += s
        blob += b"\x5a" * GUARD
        iblob, self.ioffs = bytearray(b"\x5a" * GUARD), []
        for i, x in enumerate(indexes):
            iblob += b"\x5a" * ((-len(iblob)) % 16 + 16 * (i % 2))
            self.ioffs.append(len(iblob) - GUARD)
            iblob += x
        iblob += b"\x5a" * GUARD
        self.host_s, self.host_i = np.frombuffer(bytes(blob), np.uint8).copy(), np.frombuffer(bytes(iblob), np.uint8).copy()
        self.d_s, self.d_i = torch.from_numpy(self.host_s).cuda(), torch.from_numpy(self.host_i).cuda()
        torch.cuda.synchronize()
        self.offs = np.asarray(self.offs, np.uint64)
        self.lens = np.asarray([len(s) for s in streams], np.uint64)
        self.ioffs = np.asarray(self.ioffs, np.uint64)
        self.ilens = np.asarray([len(x) for x in indexes] if ilens is None else ilens, np.uint64)

    @property
    def streams_ptr(self):
        return self.d_s.data_ptr() + GUARD

    @property
    def index_ptr(self):
        return self.d_i.data_ptr() + GUARD

    def check(self):
        assert (self.d_s.cpu().numpy() == self.host_s).all() and (self.d_i.cpu().numpy() == self.host_i).all()


def _u64(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint64)) if a is not None else None


def _call(api, enc, p, views, ready_event=None, d_streams=True, d_index=True, ioffs=True, ilens=True):
    """One felics_decompress_views_device_indexed call: (rc, headers as tuples, status); status is 77 where the call wrote none."""
    n = len(views)
    st = np.full(max(n, 1), 77, np.int32)
    hd = (api._CHeader * max(n, 1))()
    cv = (api._CView * max(n, 1))(*[api._cview(v) for v in views])
    rc = api.lib().felics_decompress_views_device_indexed(
        enc._h, n, p.streams_ptr if d_streams else None, _u64(p.offs), _u64(p.lens), p.index_ptr if d_index else None,
        _u64(p.ioffs if ioffs is True else ioffs), _u64(p.ilens if ilens else None), cv, int(ready_event) if ready_event else None, hd,
        st.ctypes.data_as(C.POINTER(C.c_int)))
    return rc, [(h.color_type, h.pixel_depth, h.width, h.height) for h in hd[:n]], st[:n].copy()


def _hdr(im):
    return (int(im.ndim == 3), 0, im.shape[1], im.shape[0])


def _items(index):
    lay = ic.Layout(index)
    return lay.planes * max(lay.k, 1)


def _delta(after, before):
    return {k: after[k] - before[k] for k in after}


class _Env:
    """Sets environment variables the library reads per call and restores them."""

    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        os.environ.update(self.kv)

    def __exit__(self, *exc):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def test_mixed_call(api, enc, cases):
    """Every shape, gray and RGB, in ONE call, the segment size alternating from stream to stream, into dense frames that lie 7 bytes
    apart in one surface: byte-equal to the images, every status OK, a wave per (stream, plane, segment)."""
    keys = [(w, h, rgb) for w, h in ic.SHAPES for rgb in (0, 1)]
    imgs = [cases[k][0] for k in keys]
    streams = [cases[k][1] for k in keys]
    indexes = [cases[k][2][ic.SEGMENTS[i % 2]] for i, k in enumerate(keys)]
    at, where = 5, []
    for im in imgs:
        where.append(at)
        at += im.size + 7
    m = vc.Surface((at,))
    views = [m.view(lambda a, o=o, im=im: a[o:o + im.size].reshape(im.shape), im) for o, im in zip(where, imgs)]
    p = Inputs(streams, indexes)
    s0 = enc.index_view_stats()
    i0 = enc.decode_stats()
    rc, hdrs, st = _call(api, enc, p, views)
    assert rc == vc.OK and (st == vc.OK).all(), st
    assert hdrs == [_hdr(im) for im in imgs]
    m.check("mixed call")
    p.check()
    d = _delta(enc.index_view_stats(), s0)
    assert d["streams"] == len(keys) and d["undecoded"] == 0 and d["items"] == sum(_items(x) for x in indexes)
    assert d["passes"] >= 1 and 1 <= d["launches"] <= 4 * d["passes"]
    assert enc.index_view_stats()["plane_bytes"] == sum(6 * im.shape[0] * im.shape[1] for im in imgs if im.ndim == 3)  # (one pass holds them all)
    assert enc.decode_stats() == i0  # (felics_decode_stats and felics_index_stats count the other calls)
    # the getter writes min(out_size, sizeof) bytes
    part = api._CIndexViewStats(7, 7, 7, 7, 7, 7)
    assert api.lib().felics_get_index_view_stats(enc._h, C.byref(part), 16) == 0
    now = enc.index_view_stats()
    assert (part.streams, part.undecoded, part.items, part.launches) == (now["streams"], now["undecoded"], 7, 7)
    # n = 0
    hd, st = enc.decompress_views_device_indexed(0, [], [], 0, [], [], [])
    assert hd == [] and len(st) == 0


@pytest.mark.parametrize("shape", [(100, 100), (64, 65), (4096, 3), (1, 9000), (512, 256)])
def test_layouts(api, enc, cases, shape):
    """Every layout of the host test, gray and RGB, in one call per shape: the gaps keep their pattern."""
    w, h = shape
    surfaces, views, streams, indexes = [], [], [], []
    for rgb in (0, 1):
        img, stream, idx = cases[(w, h, rgb)]
        for name, sshape, fs in vc.layouts(h, w, rgb):
            m = vc.Surface(sshape)
            surfaces.append((name, rgb, m))
            for f in fs:
                views.append(m.view(f, img))
                streams.append(stream)
                indexes.append(idx[ic.SEGMENTS[len(views) % 2]])
    p = Inputs(streams, indexes)
    rc, hdrs, st = _call(api, enc, p, views)
    assert rc == vc.OK and (st == vc.OK).all(), st
    for name, rgb, m in surfaces:
        m.check("%s, rgb %d" % (name, rgb))
    p.check()


@pytest.mark.parametrize("rgb", [0, 1])
def test_equal_to_the_dense_call(api, enc, cases, oracle, rgb):
    """Three streams of one shape into dense views: byte for byte what felics_decompress_batch_device_indexed writes."""
    import torch

    w, h = 100, 100
    imgs = ic.images(w, h, rgb, 3)
    streams = [oracle.compress(im) for im in imgs]
    indexes = [api.index_build(s, 4096) for s in streams]
    frame = imgs[0].size
    status, frames = ic.decode_indexed(enc, streams, indexes, frame, guard=256)
    assert (status == 0).all()
    m = vc.Surface((3,) + imgs[0].shape)
    views = [m.view(lambda a, k=k: a[k]) for k in range(3)]
    p = Inputs(streams, indexes)
    rc, hdrs, st = _call(api, enc, p, views)
    assert rc == vc.OK and (st == vc.OK).all()
    torch.cuda.synchronize()
    got = m.dev.cpu().numpy()
    for k in range(3):
        assert (got[k].reshape(-1) == frames[k]).all() and (got[k] == imgs[k]).all()
    p.check()


def test_errors_among_valid_streams(api, enc, cases, oracle):
    """Bad pairs between good ones, in one call: each gets the code of felics.h's list, every other stream decodes, and a failing
    stream touches nothing but its own samples (a pair the host refuses: not even those)."""
    gimg, gstream, gidx = cases[(64, 65, 0)]
    cimg, cstream, cidx = cases[(100, 100, 1)]
    entries = []  # (stream, index, idx_len or None, image the view is made for, expected code, whether its samples may be written)

    def good():
        entries.append((gstream, gidx[4096], None, gimg, vc.OK, False))
        entries.append((cstream, cidx[12288], None, cimg, vc.OK, False))

    good()
    on_device = ("offset_beyond", "offset_plus_1", "co_300")  # (what only the walk finds: the others fail the header's checks on the host)
    for stream, index, img in ((gstream, gidx[4096], gimg), (cstream, cidx[4096], cimg)):
        for name, bad in ic.corruptions(index).items():
            entries.append((stream, bad, None, img, vc.E_INVALID_INDEX, name in on_device))
        good()
    entries.append((cstream[:len(cstream) // 16], cidx[4096], None, cimg, vc.E_IO, False))  # cannot hold what its header claims
    entries.append((gstream[:-5], gidx[4096], None, gimg, vc.E_INVALID_INDEX, False))       # the index names another last byte
    entries.append((gstream[:9], gidx[4096], None, gimg, vc.E_IO, False))
    good()
    entries.append((gstream, gidx[4096] + b"\x5a" * 16, len(gidx[4096]) + 16, gimg, vc.E_INVALID_INDEX, False))
    entries.append((gstream, gidx[4096], len(gidx[4096]) - 16, gimg, vc.E_INVALID_INDEX, False))
    entries.append((gstream, gidx[4096], 48, gimg, vc.E_INVALID_INDEX, False))
    s16 = oracle.compress(np.arange(64 * 65, dtype=np.uint16).reshape(65, 64))
    entries.append((s16, gidx[4096], None, gimg, vc.E_UNSUPPORTED, False))
    entries.append((gstream, gidx[4096], None, gimg[:, :63].copy(), vc.E_INVALID_DIMENSIONS, False))  # a view of another shape
    wide = np.zeros((1, 40000), np.uint8)  # one row too wide for the wave form's LDS
    swide = oracle.compress(wide)
    entries.append((swide, api.index_build(swide, 4096), None, wide, vc.E_UNSUPPORTED, False))
    good()
    surfaces, views = [], []
    for stream, index, ilen, img, code, loose in entries:
        m = vc.Surface((img.shape[0] + 2, img.shape[1] + 5) + img.shape[2:])
        f = lambda a, img=img: a[1:1 + img.shape[0], 2:2 + img.shape[1]]  # noqa: E731
        views.append(m.view(f, img if code == vc.OK else None, loose=loose))
        surfaces.append(m)
    p = Inputs([e[0] for e in entries], [e[1] for e in entries], [len(e[1]) if e[2] is None else e[2] for e in entries])
    s0 = enc.index_view_stats()
    rc, hdrs, st = _call(api, enc, p, views)
    want = [e[4] for e in entries]
    assert list(st) == want, [(i, int(a), b) for i, (a, b) in enumerate(zip(st, want)) if a != b]
    assert rc == next(c for c in want if c != vc.OK)
    for i, m in enumerate(surfaces):
        m.check("entry %d" % i)
    p.check()
    d = _delta(enc.index_view_stats(), s0)
    assert d["streams"] == len(entries)
    assert d["undecoded"] == sum(1 for e in entries if e[4] != vc.OK and not e[5])
    assert d["items"] == sum(_items(e[1]) for e in entries if e[4] == vc.OK or e[5])
    assert hdrs[-3] == (0, 0, 40000, 1) and hdrs[-4] == (0, 0, 64, 65) and hdrs[-5] == (0, 1, 64, 65)  # (the header the stream has)


def test_prelaunch_refusals(api, enc, cases):
    """A misaligned index, a view that aliases itself, NULL pointers, a ticket outstanding: the code in every status, stats and
    targets as they were."""
    import torch

    img, stream, idx = cases[(64, 65, 0)]
    m = vc.Surface((3, 65, 70))
    views = [m.view(lambda a, k=k: a[k, :, 3:67]) for k in range(3)]
    p = Inputs([stream] * 3, [idx[4096]] * 3)
    s0 = enc.index_view_stats()

    def refused(**kw):
        rc, hdrs, st = _call(api, enc, p, kw.pop("views", views), **kw)
        assert rc == vc.E_INVALID_ARGUMENT and (st == vc.E_INVALID_ARGUMENT).all() and hdrs == [(0, 0, 0, 0)] * 3
        m.check()
        assert enc.index_view_stats() == s0

    odd = p.ioffs.copy()
    odd[2] += 8
    refused(ioffs=odd)
    alias = list(views)
    alias[1] = alias[1][:5] + (0, 1, 0)  # row_stride = 0 with 65 rows
    refused(views=alias)
    refused(d_index=False)
    refused(d_streams=False)
    refused(ilens=False)
    frames = torch.zeros((2, 64, 64), dtype=torch.uint8, device="cuda")
    out = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    sub = enc.submit_batch_device(frames.data_ptr(), 2, 64, 64, 0, 0, out.data_ptr(), 1 << 15)
    try:
        refused()
    finally:
        enc.wait_batch(sub)
    # and the same call decodes once nothing stands in the way
    for k in range(3):
        m.view(lambda a, k=k: a[k, :, 3:67], img)
    rc, hdrs, st = _call(api, enc, p, views)
    assert rc == vc.OK and (st == vc.OK).all()
    m.check()
    p.check()


def test_ready_event(api, cases):
    """As tests/test_decode_views.py::test_ready_event: a side stream stalls for tens of milliseconds, then copies streams and indexes
    to the device and writes the fill over the surfaces; the call gets the event recorded behind that work and no host
    synchronisation.  Had a library stream started early it would have read zeros for a stream or an index (a status) or been
    overwritten by the fill.  (A race test in the one direction that cannot fail falsely; run once.)"""
    import torch

    import felics_amd

    e = felics_amd.Encoder(0)
    try:
        keys = [(100, 100, 0), (64, 65, 1), (512, 256, 0), (1, 9000, 1)]
        specs = [lambda a: a[:, :100], lambda a: a[..., :3], lambda a: a[::-1], lambda a: a.transpose(1, 2, 0)]
        shapes = [(100, 113), (65, 64, 4), (256, 512), (3, 9000, 1)]
        surfs, views = [], []
        for k, f, shape in zip(keys, specs, shapes):
            m = vc.Surface(shape)
            views.append(m.view(f, cases[k][0]))
            surfs.append(m)
        p = Inputs([cases[k][1] for k in keys], [cases[k][2][4096] for k in keys])
        final_s, final_i = p.d_s, p.d_i
        p.d_s, p.d_i = torch.zeros_like(final_s), torch.zeros_like(final_i)
        fills = [m.dev.clone() for m in surfs]
        for m in surfs:
            m.dev.zero_()
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            big = torch.zeros(1 << 26, dtype=torch.float32, device="cuda")
            for _ in range(600):
                big.add_(1.0)
            p.d_s.copy_(final_s, non_blocking=True)
            p.d_i.copy_(final_i, non_blocking=True)
            for m, f in zip(surfs, fills):
                m.dev.copy_(f, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(side)
        rc, hdrs, st = _call(api, e, p, views, ready_event=ev.cuda_event)
        assert rc == vc.OK and (st == vc.OK).all(), "a stream or an index was read before the producer had written it"
        for m in surfs:
            m.check()
        p.check()
        del big
    finally:
        e.close()


def test_passes(api, enc, oracle):
    """Five RGB streams whose planes are capped at two streams a pass: three passes at least, the same output as uncapped."""
    w, h = 64, 65
    imgs = (ic.images(w, h, 1, 3) + ic.images(w, h, 1, 2))[:5]
    streams = [oracle.compress(im) for im in imgs]
    indexes = [api.index_build(s, 4096) for s in streams]
    p = Inputs(streams, indexes)
    out = []
    for cap in (None, str(2 * 6 * w * h)):
        m = vc.Surface((5, h, w, 4))
        views = [m.view(lambda a, k=k: a[k, :, :, :3], imgs[k]) for k in range(5)]
        s0 = enc.index_view_stats()
        with _Env(**({"FELICS_TEST_INDEX_VIEWS_PASS": cap} if cap else {})):
            rc, hdrs, st = _call(api, enc, p, views)
        assert rc == vc.OK and (st == vc.OK).all()
        m.check()
        d = _delta(enc.index_view_stats(), s0)
        if cap:
            assert d["passes"] >= 3 and enc.index_view_stats()["plane_bytes"] == 2 * 6 * w * h
        else:
            assert d["passes"] == 1 and enc.index_view_stats()["plane_bytes"] == 5 * 6 * w * h
        out.append(m.dev.cpu().numpy())
    assert (out[0] == out[1]).all()
    p.check()


def test_torch_targets(api, enc, oracle):
    """decompress_arrays_device_indexed into the images of an N x 3 x H x W uint8 tensor and into rgba[..., :3]."""
    import torch

    N, H, W = 3, 65, 64
    imgs = ic.images(W, H, 1, 3)
    extra = ic.images(100, 100, 1, 1)[0]
    streams = [oracle.compress(im) for im in imgs + [extra]]
    indexes = [api.index_build(s, 4096) for s in streams]
    p = Inputs(streams, indexes)
    batch = torch.full((N, 3, H, W), 0x5A, dtype=torch.uint8, device="cuda")
    rgba = torch.full((100, 100, 4), 0x5A, dtype=torch.uint8, device="cuda")
    arrays = [batch[i].permute(1, 2, 0) for i in range(N)] + [rgba[..., :3]]
    torch.cuda.synchronize()
    hd, st = enc.decompress_arrays_device_indexed(p.streams_ptr, p.offs, p.lens, p.index_ptr, p.ioffs, p.ilens, arrays)
    assert (st == vc.OK).all() and [(h.width, h.height) for h in hd] == [(W, H)] * N + [(100, 100)]
    assert torch.equal(batch, torch.from_numpy(np.stack([im.transpose(2, 0, 1) for im in imgs])).cuda())
    want = np.full((100, 100, 4), 0x5A, np.uint8)
    want[..., :3] = extra
    assert torch.equal(rgba, torch.from_numpy(want).cuda())
    p.check()
