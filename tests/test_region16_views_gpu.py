"""Regions of 16-bit streams into device views, mixed shapes in one call (felics_decompress_region_views_device_indexed16), on the GPU.

Streams come from the CPU oracle and version-2 indexes from felics_index16_build.  Streams and indexes lie between guard bytes in
device memory and are compared unchanged after every call; every target is a uint16 surface whose every byte is 0xA5, compared WHOLE
afterwards: the samples must be the window's, every other byte must still hold 0xA5."""
import ctypes as C

import numpy as np
import pytest

from tests import index16_common as ic
from tests import index16_views_common as vc
from tests import region_common as rc
from tests import region_views_common as rv

pytestmark = pytest.mark.gpu
NAMES = ("alias", "spikes", "chroma", "100x100_rgb")


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
    """[(w, h, rgb, image, oracle stream, index, its layout)] of the mixed call, segments of 4096 pixels: computed once"""
    out = []
    for name in NAMES:
        im = ic.cases()[name][0]
        stream = oracle.compress(im)
        index = api.index16_build(stream, 4096)
        out.append((im.shape[1], im.shape[0], int(im.ndim == 3), im, stream, index, ic.Layout16(index)))
    return out


def _hdr(im):
    return (int(im.ndim == 3), 1, im.shape[1], im.shape[0])


def _rows_loaded(lay, need):
    return sum(lay.get(c, j)[2] for c in range(lay.planes) for j in need)


def _targets(cases, windows_of):
    """every window windows_of(w, h) of every stream into every layout: (regions, views, surfaces, plan rows)"""
    regions, views, surfaces, rows = [], [], [], []
    for s, (w, h, rgb, im, stream, index, lay) in enumerate(cases):
        for window in windows_of(w, h):
            need, waves, pixels = rv.plan(w, h, 4096, lay.planes, window)
            for name, shape, fs in vc.layouts(window[3], window[2], rgb):
                m = vc.Surface(shape)
                surfaces.append(("%dx%d rgb %d %s %s" % (w, h, rgb, window, name), m))
                for f in fs:
                    views.append(m.view(f, rc.crop(im, window)))
                    regions.append((s,) + tuple(window))
                    rows.append((w, rgb, window[2], window[3], waves, pixels, lay.planes * lay.k, _rows_loaded(lay, need)))
    return regions, views, surfaces, rows


def test_mixed_shapes_in_one_call(api, enc, cases):
    """alias, spikes, chroma and 100x100_rgb, every fixed window of each into every layout, ONE call: the crops of the originals,
    untouched fill, unchanged inputs; the counters are the plan by marking, rows_loaded the directories' n_rows of the needed
    segments"""
    regions, views, surfaces, rows = _targets(cases, rv.fixed_windows)
    assert len(regions) > 100
    p = rv.Inputs([c[4] for c in cases], [c[5] for c in cases], 64)
    s0, other0 = enc.region16_view_stats(), (enc.region16_stats(), enc.index16_view_stats(), enc.region_view_stats())
    code, hdrs, st = rv.device_call(api, enc, True, p, regions, views)
    assert code == rv.OK and (st == rv.OK).all(), st
    assert hdrs == [_hdr(c[3]) for c in cases]
    for what, m in surfaces:
        m.check(what)
    p.check()
    d = rv.delta(enc.region16_view_stats(), s0)
    assert d["regions"] == len(regions) and d["undecoded"] == 0
    assert d["segments_walked"] == sum(r[4] for r in rows)
    assert d["segments_skipped"] == sum(r[6] - r[4] for r in rows)
    assert d["pixels_walked"] == sum(r[5] for r in rows)
    assert d["rows_loaded"] == sum(r[7] for r in rows) > 0
    now = enc.region16_view_stats()
    k = now["table_bytes"] // (131071 * 64)  # the tables of the call: a launch holds that many waves
    assert k >= 1 and now["table_bytes"] % (131071 * 64) == 0
    npass, nlaunch, most = rv.passes_and_launches(rows, 1 << 62, True, k)
    assert (d["passes"], d["launches"], now["plane_bytes"]) == (npass, nlaunch, most)
    assert (enc.region16_stats(), enc.index16_view_stats(), enc.region_view_stats()) == other0
    part = api._CRegion16ViewStats(*[7] * 10)
    assert api.lib().felics_get_region_view_wide_stats(enc._h, C.byref(part), 16) == 0
    assert (part.regions, part.undecoded, part.segments_walked, part.table_bytes) == (now["regions"], now["undecoded"], 7, 7)


def test_full_frame_window_is_the_views_call(api, enc, cases):
    """the full-frame window of every stream: byte for byte what felics_decompress_views_device_indexed16 writes into the same views"""
    import torch

    regions, views, surfaces, _ = _targets(cases, lambda w, h: [(0, 0, w, h)])
    stream_of = [r[0] for r in regions]
    p = rv.Inputs([cases[s][4] for s in stream_of], [cases[s][5] for s in stream_of], 64)  # (the views call: a stream per view)
    code, hdrs, st = rv.device_call(api, enc, True, p, [(i,) + r[1:] for i, r in enumerate(regions)], views)
    assert code == rv.OK and (st == rv.OK).all()
    got = [m.got().copy() for _, m in surfaces]
    for _, m in surfaces:
        m.check()
        m.dev.copy_(torch.from_numpy(m.host.view(np.int16)))
    hd, st = enc.decompress_views_device_indexed16(p.streams_ptr, p.offs, p.lens, p.index_ptr, p.ioffs, p.ilens, views)
    assert (st == rv.OK).all()
    for (what, m), g in zip(surfaces, got):
        assert (m.got() == g).all(), what
    p.check()


def test_passes(api, enc, cases):
    """FELICS_TEST_INDEX16_PASS=3: a launch holds three waves, so the six waves of an RGB window that needs two segments are cut inside
    the region and inside plane 1; FELICS_TEST_INDEX_VIEWS_PASS caps the planes at two windows a pass.  The same samples as uncapped,
    passes and launches as planned."""
    rgb100 = next(i for i, c in enumerate(cases) if c[:3] == (100, 100, 1))
    alias = next(i for i, c in enumerate(cases) if c[:3] == (64, 130, 0))
    wins = [(rgb100, 90, 40, 10, 20), (alias, 5, 60, 10, 8), (rgb100, 10, 10, 20, 10), (rgb100, 0, 83, 40, 5), (rgb100, 80, 90, 20, 10),
            (rgb100, 33, 40, 40, 5)]
    assert rc.needed_by_marking(100, 100, 4096, wins[0][1:]) == [0, 1]
    p = rv.Inputs([c[4] for c in cases], [c[5] for c in cases], 64)
    out = []
    for cap, k in ((None, None), (2 * 12 * 200, 3)):
        views, surfaces, rows = [], [], []
        for r in wins:
            w, h, rgb, im, _, _, lay = cases[r[0]]
            m = vc.Surface((r[4] + 2, r[3] + 3, 4) if rgb else (r[4] + 2, r[3] + 3))
            f = (lambda a, r=r: a[1:1 + r[4], 2:2 + r[3], :3]) if rgb else (lambda a, r=r: a[1:1 + r[4], 2:2 + r[3]])
            views.append(m.view(f, rc.crop(im, r[1:])))
            surfaces.append(m)
            rows.append((w, rgb, r[3], r[4], rv.plan(w, h, 4096, lay.planes, r[1:])[1]))
        assert rows[0][4] == 6
        s0 = enc.region16_view_stats()
        env = {"FELICS_TEST_INDEX_VIEWS_PASS": str(cap), "FELICS_TEST_INDEX16_PASS": str(k)} if cap else {}
        with rv.Env(**env):
            code, hdrs, st = rv.device_call(api, enc, True, p, wins, views)
        assert code == rv.OK and (st == rv.OK).all()
        for m in surfaces:
            m.check()
        d = rv.delta(enc.region16_view_stats(), s0)
        now = enc.region16_view_stats()
        tables = now["table_bytes"] // (131071 * 64)
        assert tables == 3 if cap else tables >= 1
        npass, nlaunch, most = rv.passes_and_launches(rows, cap or 1 << 62, True, tables)
        assert (d["passes"], d["launches"], now["plane_bytes"]) == (npass, nlaunch, most)
        assert npass == (3 if cap else 1) and most == (4800 if cap else 12000)
        out.append([m.got().copy() for m in surfaces])
    assert all((a == b).all() for a, b in zip(*out))
    p.check()


def test_per_region_isolation(api, enc, cases, oracle):
    """one call: a window outside its stream's image, a view of the other depth, a stream with a bad header, a forged bit offset in
    a needed segment and the same forgery where no region needs it, intact regions around them.  Every code is the host model's; a
    region refused before the launch leaves its surface untouched, every intact one holds its crop."""
    _, _, _, cimg, cstream, cidx, _ = next(c for c in cases if c[:3] == (100, 100, 1))
    _, _, _, gimg, gstream, gidx, _ = next(c for c in cases if c[:3] == (64, 130, 0))
    forged = ic.corruptions(cidx)["bit_offset_plus_1"]  # checkpoint (0, 1) moved by a bit: segment (0, 0) no longer ends on it
    nosig = b"FLCX" + cstream[4:]
    streams = [cstream, gstream, nosig, cstream, cstream]
    indexes = [cidx, gidx, cidx, forged, forged]
    # (stream, window, depth of the view, may its samples be written)
    entries = [
        (0, (33, 40, 31, 3), 1, False),
        (0, (90, 90, 20, 20), 1, False),   # outside the image
        (1, (5, 60, 10, 8), 1, False),
        (1, (10, 10, 20, 4), 0, False),    # an 8-bit view of a 16-bit stream
        (2, (10, 10, 5, 5), 1, False),     # the stream with the bad header
        (1, (0, 128, 64, 2), 1, False),
        (3, (90, 40, 10, 2), 1, True),     # needs segment (0, 0) to its end: refused by the walk
        (4, (0, 0, 100, 40), 1, False),    # the same forgery, not needed: served
        (0, (0, 0, 100, 100), 1, False),
    ]
    p = rv.Inputs(streams, indexes, 64)
    regions, views, surfaces, want = [], [], [], []
    for s, window, depth, loose in entries:
        rgb = streams[s] is not gstream
        img = cimg if rgb else gimg
        x, y, w, h = window
        shape = (h + 2, w + 5, 3) if rgb else (h + 2, w + 5)
        m = vc.Surface(shape)
        host = vc.filled(shape)
        f = lambda a, w=w, h=h: a[1:1 + h, 2:2 + w]  # noqa: E731
        view = m.view(f)
        hview = rv.host_view(f(host), True)
        if not depth:  # the same place as a view of depth 8
            view, hview = (t[:4] + (0,) + t[5:] for t in (view, hview))
        code = rv.host_call(api, True, streams[s], indexes[s], window, hview)
        if code == rv.OK:
            assert (f(host) == rc.crop(img, window)).all()
            m.view(f, rc.crop(img, window))
        elif loose:
            m.view(f, loose=True)
        regions.append((s,) + window)
        views.append(view)
        surfaces.append(m)
        want.append(code)
    assert want[1] == rv.E_INVALID_ARGUMENT and want[3] == rv.E_INVALID_DIMENSIONS and want[4] not in (rv.OK, rv.E_INVALID_INDEX)
    assert want[6] == rv.E_INVALID_INDEX and want[7] == rv.OK and [want[i] for i in (0, 2, 5, 8)] == [rv.OK] * 4
    s0 = enc.region16_view_stats()
    code, hdrs, st = rv.device_call(api, enc, True, p, regions, views)
    assert list(st) == want and code == want[1]
    for i, m in enumerate(surfaces):
        m.check("entry %d" % i)
    p.check()
    assert hdrs[2] == (0, 0, 0, 0) and hdrs[0] == hdrs[3] == (1, 1, 100, 100)
    assert rv.delta(enc.region16_view_stats(), s0)["undecoded"] == 3


def test_refusals_before_launch(api, enc, cases, oracle):
    """an index at a multiple of 16 that is no multiple of 64, a stream number too large, a view of another size than its window, an
    aliasing view, a ticket outstanding: the code in every status; a call whose only stream is 8-bit: FELICS_E_UNSUPPORTED in every
    status.  Every surface and the counters stay as they were."""
    import torch

    _, _, _, img, stream, index, _ = next(c for c in cases if c[:3] == (64, 130, 0))
    m = vc.Surface((3, 12, 40))
    regions = [(k % 2, 10 * k, 5, 31, 10) for k in range(3)]
    views = [m.view(lambda a, k=k: a[k, 1:11, 3:34]) for k in range(3)]
    p = rv.Inputs([stream] * 2, [index] * 2, 64)
    s0 = enc.region16_view_stats()

    def refused(code=rv.E_INVALID_ARGUMENT, regions=regions, views=views, inputs=p, **kw):
        rc_, hdrs, st = rv.device_call(api, enc, True, inputs, regions, views, **kw)
        assert rc_ == code and (st == code).all(), (rc_, st)
        m.check()
        assert rv.delta(enc.region16_view_stats(), s0)["segments_walked"] == 0

    odd = p.ioffs.copy()
    odd[1] += 16
    refused(ioffs=odd)
    refused(regions=[regions[0], (2,) + regions[1][1:], regions[2]])
    refused(views=[views[0], views[1][:1] + (30,) + views[1][2:], views[2]])
    refused(views=[views[0], views[1], views[2][:2] + (9,) + views[2][3:]])
    refused(views=[views[0], views[1][:5] + (0, 2, 0), views[2]])  # row_stride = 0 with 10 rows
    assert enc.region16_view_stats() == s0
    s8 = oracle.compress((img >> 8).astype(np.uint8))
    refused(code=rv.E_UNSUPPORTED, inputs=rv.Inputs([s8] * 2, [api.index_build(s8, 4096)] * 2, 64))
    s0 = enc.region16_view_stats()
    frames = torch.zeros((2, 64, 64), dtype=torch.uint8, device="cuda")
    out = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    sub = enc.submit_batch_device(frames.data_ptr(), 2, 64, 64, 0, 0, out.data_ptr(), 1 << 15)
    try:
        refused()
    finally:
        enc.wait_batch(sub)
    # and the same call decodes once nothing stands in the way; the Python method raises with the statuses of a refused one
    for k, r in enumerate(regions):
        m.view(lambda a, k=k: a[k, 1:11, 3:34], rc.crop(img, r[1:]))
    hd, st = enc.decompress_region_views_device_indexed16(p.streams_ptr, p.offs, p.lens, p.index_ptr, p.ioffs, p.ilens, regions, views)
    assert (st == rv.OK).all() and [(h.width, h.height) for h in hd] == [(64, 130)] * 2
    m.check()
    with pytest.raises(api.FelicsError) as ei:
        enc.decompress_region_views_device_indexed16(p.streams_ptr, p.offs, p.lens, p.index_ptr, p.ioffs, p.ilens,
                                                     [regions[0], (0, 60, 0, 31, 10), regions[2]], views)
    assert ei.value.code == rv.E_INVALID_ARGUMENT and list(ei.value.status) == [rv.OK, rv.E_INVALID_ARGUMENT, rv.OK]
    p.check()


def test_empty_regions(api, enc, cases):
    """empty windows, the far corner among them, with zero-sized views: their stream's header and index-header code and no walk;
    n_regions = 0"""
    good = next(c for c in cases if c[:3] == (100, 100, 1))
    bad = ic.corruptions(good[5])["reserved"]
    p = rv.Inputs([good[4], good[4]], [good[5], bad], 64)
    regions = [(0, 0, 0, 0, 0), (0, 100, 100, 0, 0), (0, 0, 0, 100, 0), (0, 50, 50, 0, 1), (1, 100, 100, 0, 0), (1, 0, 0, 0, 7)]
    views = [(0, r[3], r[4], 1, 1, 0, 0, 0) for r in regions]
    s0 = enc.region16_view_stats()
    code, hdrs, st = rv.device_call(api, enc, True, p, regions, views)
    assert list(st) == [rv.OK] * 4 + [rv.E_INVALID_INDEX] * 2 and code == rv.E_INVALID_INDEX
    d = rv.delta(enc.region16_view_stats(), s0)
    assert (d["regions"], d["undecoded"], d["segments_walked"], d["pixels_walked"], d["launches"], d["passes"], d["rows_loaded"]) == \
        (6, 2, 0, 0, 0, 0, 0)
    assert d["segments_skipped"] == 4 * 3 * good[6].k
    for r, v in zip(regions, views):
        assert rv.host_call(api, True, good[4], good[5] if r[0] == 0 else bad, r[1:], v) == (rv.OK if r[0] == 0 else rv.E_INVALID_INDEX)
    code, hdrs, st = rv.device_call(api, enc, True, p, [], [])
    assert code == rv.OK and hdrs == [(0, 0, 0, 0)] * 2
    hd, st = enc.decompress_region_views_device_indexed16(p.streams_ptr, p.offs, p.lens, p.index_ptr, p.ioffs, p.ilens, [], [])
    assert len(st) == 0
    p.check()


def test_ready_event(api, cases):
    """As tests/test_index16_views_gpu.py::test_ready_event: a side stream stalls, then copies streams and indexes to the device and
    writes the fill over the surfaces; the call gets the event recorded behind that work and no host synchronisation.  Had a library
    stream started early it would have read zeros for a stream or an index (a status) or been overwritten by the fill."""
    import torch

    import felics_amd

    e = felics_amd.Encoder(0)
    try:
        wins = [(5, 60, 10, 8), (10, 10, 5, 5), (0, 124, 33, 1), (90, 40, 10, 2)]  # of alias, spikes, chroma, 100x100_rgb
        specs = [lambda a: a[:, :10], lambda a: a[::-1], lambda a: a[..., :3], lambda a: a.transpose(1, 2, 0)]
        shapes = [(8, 23), (5, 5), (1, 33, 4), (3, 2, 10)]
        surfs, views = [], []
        for c, win, f, shape in zip(cases, wins, specs, shapes):
            m = vc.Surface(shape)
            views.append(m.view(f, rc.crop(c[3], win)))
            surfs.append(m)
        p = rv.Inputs([c[4] for c in cases], [c[5] for c in cases], 64)
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
        code, hdrs, st = rv.device_call(api, e, True, p, [(i,) + w for i, w in enumerate(wins)], views, ready_event=ev.cuda_event)
        assert code == rv.OK and (st == rv.OK).all(), "a stream or an index was read before the producer had written it"
        for m in surfs:
            m.check()
        p.check()
        del big
    finally:
        e.close()


def test_torch_targets(api, enc, cases):
    """decompress_region_arrays_device_indexed16: a window of both RGB streams and of a gray one into the slices of int16-typed
    batch tensors (torch's uint16 is younger than some of its builds; the bytes are what is compared)"""
    import torch

    rgbs = [i for i, c in enumerate(cases) if c[2]]
    gray = next(i for i, c in enumerate(cases) if c[:3] == (64, 130, 0))
    p = rv.Inputs([c[4] for c in cases], [c[5] for c in cases], 64)
    batch = np.full((len(rgbs), 3, 20, 30), 0x5A5A, np.uint16)
    tile = np.full((64, 80), 0x5A5A, np.uint16)
    d_batch, d_tile = torch.from_numpy(batch.view(np.int16)).cuda(), torch.from_numpy(tile.view(np.int16)).cuda()

    class U16:
        """a uint16 view of an int16 tensor's slice for view_of_array"""

        def __init__(self, t):
            self.__cuda_array_interface__ = {"shape": tuple(t.shape), "typestr": "<u2", "data": (t.data_ptr(), False), "version": 2,
                                             "strides": tuple(2 * v for v in t.stride())}

    regions = [(s, 2, 9, 30, 20) for s in rgbs] + [(gray, 10, 50, 40, 32)]
    arrays = [U16(d_batch[i].permute(1, 2, 0)) for i in range(len(rgbs))] + [U16(d_tile[16:48, 20:60])]
    torch.cuda.synchronize()
    hd, st = enc.decompress_region_arrays_device_indexed16(p.streams_ptr, p.offs, p.lens, p.index_ptr, p.ioffs, p.ilens, regions, arrays)
    assert (st == rv.OK).all() and len(hd) == len(cases)
    want = np.stack([cases[s][3][9:29, 2:32].transpose(2, 0, 1) for s in rgbs])
    assert (d_batch.cpu().numpy().view(np.uint16) == want).all()
    tile[16:48, 20:60] = cases[gray][3][50:82, 10:50]
    assert (d_tile.cpu().numpy().view(np.uint16) == tile).all()
    p.check()
