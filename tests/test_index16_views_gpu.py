"""Indexed decode of 16-bit streams into device surfaces (felics_decompress_views_device_indexed16), on the GPU.

Frames are index16_common.cases(), streams come from the CPU oracle and indexes from felics_index16_build, so nothing here needs the
GPU encoder.  Streams and indexes lie between guard bytes in device memory and are compared unchanged after every call; every target
is a uint16 surface of 0xA5 bytes compared WHOLE afterwards: the samples must be the images, every other byte must still hold 0xA5."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import index16_common as ic
from tests import index16_views_common as vc

pytestmark = pytest.mark.gpu
GUARD = 256
TABLE = 131071 * 64  # bytes of one wave's estimator table


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
    """name -> (frame, oracle stream, {segment size: index}): computed once, read by every test"""
    out = {}
    for name, (img, _) in ic.cases().items():
        stream = oracle.compress(img)
        out[name] = (img, stream, {seg: api.index16_build(stream, seg) for seg in ic.SEGMENTS})
    return out


class Inputs:
    """Streams (at odd offsets too) and indexes (at multiples of 64, 0x5A between them) in device memory, each blob between GUARD
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
            iblob += b"\x5a" * ((-len(iblob)) % 64 + 64 * (i % 2))
            self.ioffs.append(len(iblob) - GUARD)
            iblob += x
        iblob += b"\x5a" * GUARD
        self.host_s, self.host_i = np.frombuffer(bytes(blob), np.uint8).copy(), np.frombuffer(bytes(iblob), np.uint8).copy()
        self.d_s, self.d_i = torch.from_numpy(self.host_s).cuda(), torch.from_numpy(self.host_i).cuda()
        torch.cuda.synchronize()
        assert (self.d_i.data_ptr() + GUARD) % 64 == 0
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
    """One felics_decompress_views_device_indexed16 call: (rc, headers as tuples, status); status is 77 where the call wrote none."""
    n = len(views)
    st = np.full(max(n, 1), 77, np.int32)
    hd = (api._CHeader * max(n, 1))()
    cv = (api._CView * max(n, 1))(*[api._cview(v) for v in views])
    rc = api.lib().felics_decompress_views_device_indexed_wide(
        enc._h, n, p.streams_ptr if d_streams else None, _u64(p.offs), _u64(p.lens), p.index_ptr if d_index else None,
        _u64(p.ioffs if ioffs is True else ioffs), _u64(p.ilens if ilens else None), cv, int(ready_event) if ready_event else None, hd,
        st.ctypes.data_as(C.POINTER(C.c_int)))
    return rc, [(h.color_type, h.pixel_depth, h.width, h.height) for h in hd[:n]], st[:n].copy()


def _hdr(im):
    return (int(im.ndim == 3), 1, im.shape[1], im.shape[0])


def _items(index):
    lay = ic.Layout16(index)
    return lay.planes * max(lay.k, 1)


def _delta(after, before):
    return {k: after[k] - before[k] for k in after}


def _pitched(img, pad=5):
    """a surface with a margin around a frame of img's shape, and the function that cuts the frame out of it"""
    return vc.Surface((img.shape[0] + 2, img.shape[1] + pad) + img.shape[2:]), lambda a, img=img: a[1:1 + img.shape[0], 2:2 + img.shape[1]]


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
    """Every case, gray16 and RGB16, in ONE call, the segment size alternating from stream to stream, into dense frames that lie 6
    bytes apart in one surface: byte-equal to the images, every status OK, a wave per (stream, plane, segment), a loaded row per row of
    the indexes."""
    names = list(cases)
    imgs = [cases[k][0] for k in names]
    streams = [cases[k][1] for k in names]
    indexes = [cases[k][2][ic.SEGMENTS[i % 3]] for i, k in enumerate(names)]
    at, where = 2, []
    for im in imgs:
        where.append(at)
        at += im.size + 3
    m = vc.Surface((at,))
    views = [m.view(lambda a, o=o, im=im: a[o:o + im.size].reshape(im.shape), im) for o, im in zip(where, imgs)]
    p = Inputs(streams, indexes)
    s0, i0, d0, v0 = enc.index16_view_stats(), enc.index16_stats(), enc.decode_stats(), enc.index_view_stats()
    rc, hdrs, st = _call(api, enc, p, views)
    assert rc == vc.OK and (st == vc.OK).all(), st
    assert hdrs == [_hdr(im) for im in imgs]
    m.check("mixed call")
    p.check()
    d = _delta(enc.index16_view_stats(), s0)
    assert d["streams"] == len(names) and d["undecoded"] == 0 and d["items"] == sum(_items(x) for x in indexes)
    assert d["rows_loaded"] == sum(sum(ic.Layout16(x).n_rows()) for x in indexes)
    assert d["passes"] == 1 and 1 <= d["launches"] <= 4
    now = enc.index16_view_stats()
    assert now["plane_bytes"] == sum(12 * im.shape[0] * im.shape[1] for im in imgs if im.ndim == 3)  # (one pass holds them all)
    assert now["table_bytes"] > 0 and now["table_bytes"] % TABLE == 0
    assert (enc.index16_stats(), enc.decode_stats(), enc.index_view_stats()) == (i0, d0, v0)  # (those count the other calls)
    # the getter writes min(out_size, sizeof) bytes
    part = api._CIndex16ViewStats(*([7] * 8))
    assert api.lib().felics_get_index_view_wide_stats(enc._h, C.byref(part), 16) == 0
    assert (part.streams, part.undecoded, part.items, part.table_bytes) == (now["streams"], now["undecoded"], 7, 7)
    # n = 0
    hd, st = enc.decompress_views_device_indexed16(0, [], [], 0, [], [], [])
    assert hd == [] and len(st) == 0


def test_layouts(api, enc, cases):
    """Every layout of the host test for 100 x 100 gray16 and RGB16 at K = 3 and K = 2, in one call: the gaps keep their pattern."""
    surfaces, views, streams, indexes = [], [], [], []
    for name in ("100x100", "100x100_rgb"):
        img, stream, idx = cases[name]
        for lname, sshape, fs in vc.layouts(100, 100, img.ndim == 3):
            m = vc.Surface(sshape)
            surfaces.append((lname, name, m))
            for f in fs:
                views.append(m.view(f, img))
                streams.append(stream)
                indexes.append(idx[ic.SEGMENTS[len(views) % 2]])
                assert ic.Layout16(indexes[-1]).k >= 2
    p = Inputs(streams, indexes)
    rc, hdrs, st = _call(api, enc, p, views)
    assert rc == vc.OK and (st == vc.OK).all(), st
    for lname, name, m in surfaces:
        m.check("%s, %s" % (lname, name))
    p.check()


def test_errors_among_valid_streams(api, enc, cases, oracle):
    """Bad pairs between good ones, in one call: each gets the code of felics.h's list, every other stream decodes, and a failing
    stream touches nothing but its own samples (a pair the host refuses, and every RGB one: not even those)."""
    gimg, gstream, gidx = cases["100x100"]
    cimg, cstream, cidx = cases["100x100_rgb"]
    # (stream, index, idx_len or None, image the view is made for, depth of the view, expected code, whether waves are launched for it)
    entries = []

    def good():
        entries.append((gstream, gidx[8192], None, gimg, 1, vc.OK, True))
        entries.append((cstream, cidx[4096], None, cimg, 1, vc.OK, True))

    good()
    # (what the host's look at the 64-byte header finds fails before a wave is launched; the rest is the walk's to find)
    on_host = ("magic", "version_1", "depth_0", "width", "height", "segment_pixels", "K", "total_plus_64", "total_minus_64", "reserved",
               "truncated", "appended")
    for stream, index, img in ((gstream, gidx[4096], gimg), (cstream, cidx[4096], cimg)):
        bad = ic.corruptions(index)
        assert set(on_host) < set(bad)
        for name, x in bad.items():
            entries.append((stream, x, None, img, 1, vc.E_INVALID_INDEX, name not in on_host))
        good()
    entries.append((cstream[:len(cstream) // 16], cidx[4096], None, cimg, 1, vc.E_IO, False))  # cannot hold what its header claims
    entries.append((gstream[:-5], gidx[4096], None, gimg, 1, vc.E_INVALID_INDEX, False))       # the index names another last byte
    entries.append((gstream[:9], gidx[4096], None, gimg, 1, vc.E_IO, False))
    good()
    entries.append((gstream, gidx[4096] + b"\x5a" * 64, len(gidx[4096]) + 64, gimg, 1, vc.E_INVALID_INDEX, False))
    entries.append((gstream, gidx[4096], len(gidx[4096]) - 64, gimg, 1, vc.E_INVALID_INDEX, False))
    entries.append((gstream, gidx[4096], 48, gimg, 1, vc.E_INVALID_INDEX, False))
    s8 = oracle.compress(np.arange(100 * 100, dtype=np.uint32).reshape(100, 100).astype(np.uint8))
    entries.append((s8, gidx[4096], None, gimg, 1, vc.E_UNSUPPORTED, False))
    entries.append((gstream, gidx[4096], None, gimg[:, :99].copy(), 1, vc.E_INVALID_DIMENSIONS, False))  # a view of another shape
    entries.append((gstream, gidx[4096], None, gimg, 0, vc.E_INVALID_DIMENSIONS, False))                 # a view of another depth
    wide = np.zeros((1, vc.WIDEST + 1), np.uint16)  # one row too wide for the wave form's LDS
    swide = oracle.compress(wide)
    entries.append((swide, api.index16_build(swide, 4096), None, wide, 1, vc.E_UNSUPPORTED, False))
    good()
    surfaces, views = [], []
    for stream, index, ilen, img, depth, code, launched in entries:
        m, f = _pitched(img)
        # (a gray stream that fails in the walk may have written samples of its own view; an RGB one is not converted)
        v = m.view(f, img if code == vc.OK else None, loose=launched and code != vc.OK and img.ndim == 2)
        views.append(v[:4] + (depth,) + v[5:])
        surfaces.append(m)
    p = Inputs([e[0] for e in entries], [e[1] for e in entries], [len(e[1]) if e[2] is None else e[2] for e in entries])
    s0 = enc.index16_view_stats()
    rc, hdrs, st = _call(api, enc, p, views)
    want = [e[5] for e in entries]
    assert list(st) == want, [(i, int(a), b) for i, (a, b) in enumerate(zip(st, want)) if a != b]
    assert rc == next(c for c in want if c != vc.OK)
    for i, m in enumerate(surfaces):
        m.check("entry %d" % i)
    p.check()
    d = _delta(enc.index16_view_stats(), s0)
    assert d["streams"] == len(entries)
    assert d["undecoded"] == sum(1 for e in entries if not e[6])
    assert d["items"] == sum(3 * (3 if e[3].ndim == 3 else 1) if e[5] else _items(e[1]) for e in entries if e[6])  # (K = 3 at 4096)
    assert hdrs[-3] == (0, 1, vc.WIDEST + 1, 1) and hdrs[-4] == (0, 1, 100, 100) and hdrs[-6] == (0, 0, 100, 100)  # (the header the stream has)


def test_prelaunch_refusals(api, enc, cases):
    """An index at 48 modulo 64, a view whose rows share bytes, NULL pointers, a ticket outstanding: the code in every status, stats
    and targets as they were."""
    import torch

    img, stream, idx = cases["64x65"]
    m = vc.Surface((3, 65, 70))
    views = [m.view(lambda a, k=k: a[k, :, 3:67]) for k in range(3)]
    p = Inputs([stream] * 3, [idx[4096]] * 3)
    s0 = enc.index16_view_stats()

    def refused(**kw):
        rc, hdrs, st = _call(api, enc, p, kw.pop("views", views), **kw)
        assert rc == vc.E_INVALID_ARGUMENT and (st == vc.E_INVALID_ARGUMENT).all() and hdrs == [(0, 0, 0, 0)] * 3
        m.check()
        assert enc.index16_view_stats() == s0

    odd = p.ioffs.copy()
    odd[2] += 48
    refused(ioffs=odd)
    alias = list(views)
    alias[1] = alias[1][:5] + (0, 2, 0)  # row_stride = 0 with 65 rows
    refused(views=alias)
    odd_stride = list(views)
    odd_stride[2] = odd_stride[2][:5] + (141, 2, 0)
    refused(views=odd_stride)
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


def test_forced_passes(api, enc, cases):
    """FELICS_TEST_INDEX16_PASS = 1, 2, 3 cuts launches inside a stream and inside a plane (K = 3 and K = 2 streams, one and three
    planes, two LDS classes); FELICS_TEST_INDEX_VIEWS_PASS = the smallest RGB stream's planes makes every RGB stream a pass of its own.
    Surfaces and statuses are those of the uncapped call; launches and passes are what the rules in index16_views_common give."""
    names = ["noise12", "100x100_rgb", "33x130_rgb", "4100x3", "64x64", "chroma"]
    imgs = [cases[k][0] for k in names]
    indexes = [cases[k][2][4096] for k in names]
    items = [_items(x) for x in indexes]
    assert items == [3, 9, 6, 4, 1, 6] and len({vc.lds_class(im.shape[1]) for im in imgs}) == 2
    p = Inputs([cases[k][1] for k in names], indexes)
    least = min(12 * im.shape[0] * im.shape[1] for im in imgs if im.ndim == 3)
    out = []
    for k, cap in ((None, None), (1, None), (2, None), (3, None), (None, least), (2, least)):
        surfaces, views = [], []
        for im in imgs:
            m, f = _pitched(im)
            views.append(m.view(f, im))
            surfaces.append(m)
        env = {}
        if k:
            env["FELICS_TEST_INDEX16_PASS"] = str(k)
        if cap:
            env["FELICS_TEST_INDEX_VIEWS_PASS"] = str(cap)
        s0 = enc.index16_view_stats()
        with _Env(**env):
            rc, hdrs, st = _call(api, enc, p, views)
        assert rc == vc.OK and (st == vc.OK).all(), (k, cap, st)
        for m in surfaces:
            m.check("k %s cap %s" % (k, cap))
        d = _delta(enc.index16_view_stats(), s0)
        passes = vc.stream_passes(imgs, cap or (1 << 62))
        assert len(passes) == (3 if cap else 1) and all(sum(imgs[i].ndim == 3 for i in ps) == 1 for ps in passes if cap)
        assert d["passes"] == len(passes) and d["items"] == sum(items)
        now = enc.index16_view_stats()
        assert now["plane_bytes"] == max(sum(12 * imgs[i].shape[0] * imgs[i].shape[1] for i in ps if imgs[i].ndim == 3) for ps in passes)
        if k:
            assert d["launches"] == vc.launches(imgs, items, passes, k) and now["table_bytes"] == k * TABLE
        else:
            assert d["launches"] == vc.launches(imgs, items, passes, 1 << 30)
        out.append([m.got() for m in surfaces])
    for other in out[1:]:
        assert all((a == b).all() for a, b in zip(out[0], other))
    p.check()


def test_same_stream_twice(api, enc, cases):
    """the same stream and index referenced twice (one blob each in device memory), into two views of different layouts"""
    img, stream, idx = cases["100x100_rgb"]
    p = Inputs([stream], [idx[8192]])
    p.offs, p.lens, p.ioffs, p.ilens = (np.repeat(a, 2) for a in (p.offs, p.lens, p.ioffs, p.ilens))
    m1, m2 = vc.Surface((100, 100, 4)), vc.Surface((3, 100, 100))
    views = [m1.view(lambda a: a[..., :3], img), m2.view(lambda a: a.transpose(1, 2, 0), img)]
    rc, hdrs, st = _call(api, enc, p, views)
    assert rc == vc.OK and (st == vc.OK).all()
    m1.check()
    m2.check()
    p.check()


def test_ready_event(api, cases):
    """As tests/test_index_views_gpu.py::test_ready_event: a side stream stalls for tens of milliseconds, then copies streams and
    indexes to the device and writes the fill over the surfaces; the call gets the event recorded behind that work and no host
    synchronisation.  Had a library stream started early it would have read zeros for a stream or an index (a status) or been
    overwritten by the fill.  (A race test in the one direction that cannot fail falsely; run once.)"""
    import torch

    import felics_amd

    e = felics_amd.Encoder(0)
    try:
        names = ["100x100", "33x130_rgb", "noise12", "chroma"]
        specs = [lambda a: a[:, :100], lambda a: a[..., :3], lambda a: a[::-1], lambda a: a.transpose(1, 2, 0)]
        shapes = [(100, 113), (130, 33, 4), (130, 64), (3, 130, 33)]
        surfs, views = [], []
        for k, f, shape in zip(names, specs, shapes):
            m = vc.Surface(shape)
            views.append(m.view(f, cases[k][0]))
            surfs.append(m)
        p = Inputs([cases[k][1] for k in names], [cases[k][2][4096] for k in names])
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


def test_interleaved_on_one_context(api, cases):
    """This call, the unindexed felics_decompress_batch_device on 16-bit streams, felics_decompress_batch_device_indexed16, this call
    again, on one context: the four share the table buffer and its epochs, and all are correct."""
    import torch

    import felics_amd

    names = ["noise12", "alias", "noise11"]  # three gray 64 x 130 frames: one shape for the same-shape calls
    imgs = [cases[k][0] for k in names]
    streams = [cases[k][1] for k in names]
    indexes = [cases[k][2][4096] for k in names]
    mixed = names + ["100x100_rgb", "chroma"]
    e = felics_amd.Encoder(0)
    try:
        p = Inputs([cases[k][1] for k in mixed], [cases[k][2][4096] for k in mixed])

        def views_call():
            surfaces, views = [], []
            for k in mixed:
                m, f = _pitched(cases[k][0])
                views.append(m.view(f, cases[k][0]))
                surfaces.append(m)
            rc, hdrs, st = _call(api, e, p, views)
            assert rc == vc.OK and (st == vc.OK).all(), st
            for m in surfaces:
                m.check()

        def dense_call(indexed):
            blob, offs, lens = ic.pack(streams, 16)
            iblob, ioffs, ilens = ic.pack(indexes, 64)
            d_in = torch.from_numpy(np.frombuffer(blob, np.uint8).copy()).cuda()
            d_idx = torch.from_numpy(np.frombuffer(iblob, np.uint8).copy()).cuda()
            frame = imgs[0].nbytes
            d_px = torch.zeros(3 * frame, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            if indexed:
                _, status = e.decompress_batch_device_indexed16(d_in.data_ptr(), offs, lens, d_idx.data_ptr(), ioffs, ilens, d_px.data_ptr(), 3 * frame)
            else:
                _, status = e.decompress_batch_device(d_in.data_ptr(), offs, lens, d_px.data_ptr(), 3 * frame)
            got = d_px.cpu().numpy().view(np.uint16).reshape((3,) + imgs[0].shape)
            assert (np.asarray(status) == 0).all() and all((got[i] == imgs[i]).all() for i in range(3))

        views_call()
        dense_call(False)
        dense_call(True)
        views_call()
        p.check()
    finally:
        e.close()


def test_agreement_with_the_host_model(api, enc, cases):
    """For every case, and for failing pairs of every kind, the statuses are felics_decompress_indexed16_view's and so are the
    surfaces -- whole, where the stream decodes or is RGB (a failing RGB stream leaves its view untouched in both); of a failing gray
    stream both may have written samples of the view, the model those in front of the failing segment, and neither anything else."""
    gimg, gstream, gidx = cases["100x100"]
    cimg, cstream, cidx = cases["100x100_rgb"]
    entries = [(cases[k][1], cases[k][2][ic.SEGMENTS[i % 3]], cases[k][0]) for i, k in enumerate(cases)]
    for stream, index, img in ((gstream, gidx[4096], gimg), (cstream, cidx[4096], cimg)):
        entries += [(stream, x, img) for x in ic.corruptions(index).values()]
    entries += [(gstream[:-5], gidx[4096], gimg), (cstream[:len(cstream) // 16], cidx[4096], cimg), (gstream, cidx[4096], gimg),
                (gstream, gidx[4096], gimg[:, :99].copy())]
    surfaces, views, codes = [], [], []
    for stream, index, img in entries:
        host = vc.Surface((img.shape[0] + 2, img.shape[1] + 5) + img.shape[2:], device=False)
        f = lambda a, img=img: a[1:1 + img.shape[0], 2:2 + img.shape[1]]  # noqa: E731
        s = np.frombuffer(stream, np.uint8)
        x = np.frombuffer(index, np.uint8)
        cv = api._cview(host.view(f))
        codes.append(api.lib().felics_decompress_indexed_view_wide(s.ctypes.data, len(s), x.ctypes.data, len(x), C.byref(cv), None))
        m, f = _pitched(img)
        views.append(m.view(f, loose=codes[-1] != vc.OK and img.ndim == 2))
        m.want = host.host  # what the model left: the image in its place, or the fill
        surfaces.append(m)
    assert codes[:len(cases)] == [vc.OK] * len(cases) and all(c != vc.OK for c in codes[len(cases):])
    p = Inputs([e[0] for e in entries], [e[1] for e in entries])
    rc, hdrs, st = _call(api, enc, p, views)
    assert list(st) == codes, [(i, int(a), b) for i, (a, b) in enumerate(zip(st, codes)) if a != b]
    for i, m in enumerate(surfaces):
        m.check("entry %d" % i)
    p.check()


def test_torch_targets(api, enc, cases):
    """decompress_arrays_device_indexed16 into the images of an N x 3 x H x W int16 tensor and into rgba[..., :3]."""
    import torch

    img, stream, idx = cases["33x130_rgb"]
    extra, xstream, xidx = cases["100x100_rgb"]
    p = Inputs([stream, stream, xstream], [idx[4096], idx[8192], xidx[4096]])

    class U16:  # (uint16 samples in an int16 tensor: not every torch build has a uint16 dtype on the device)
        def __init__(self, t):
            self.__cuda_array_interface__ = {"shape": tuple(t.shape), "typestr": "<u2", "data": (t.data_ptr(), False), "version": 2,
                                             "strides": tuple(2 * v for v in t.stride())}

    batch = torch.full((2, 3, 130, 33), 0x5A5A, dtype=torch.int16, device="cuda")
    rgba = torch.full((100, 100, 4), 0x5A5A, dtype=torch.int16, device="cuda")
    arrays = [U16(batch[i].permute(1, 2, 0)) for i in range(2)] + [U16(rgba[..., :3])]
    torch.cuda.synchronize()
    hd, st = enc.decompress_arrays_device_indexed16(p.streams_ptr, p.offs, p.lens, p.index_ptr, p.ioffs, p.ilens, arrays)
    assert (st == vc.OK).all() and [(h.width, h.height) for h in hd] == [(33, 130)] * 2 + [(100, 100)]
    got = batch.cpu().numpy().view(np.uint16)
    assert all((got[i].transpose(1, 2, 0) == img).all() for i in range(2))
    want = np.full((100, 100, 4), 0x5A5A, np.uint16)
    want[..., :3] = extra
    assert (rgba.cpu().numpy().view(np.uint16) == want).all()
    p.check()
