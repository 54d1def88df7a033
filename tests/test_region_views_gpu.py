"""Regions into device views, mixed shapes in one call (felics_decompress_region_views_device_indexed), on the GPU.

Streams come from the CPU oracle and indexes from felics_index_build.  Streams and indexes lie between guard bytes in device memory and
are compared unchanged after every call; every target is a surface of 0xA5 compared WHOLE afterwards: the samples must be the window's,
every other byte -- alpha, pitch padding, neighbouring cells, guard bands -- must still hold 0xA5."""
import ctypes as C

import numpy as np
import pytest

from tests import index_common as ic
from tests import index_views_common as vc
from tests import region_common as rc
from tests import region_views_common as rv

pytestmark = pytest.mark.gpu
GRAY = [(100, 100), (8200, 2), (4096, 3), (1, 9000), (4097, 1), (5000, 3), (512, 256), (64, 64)]
RGB = [(100, 100), (64, 64)]
AT_8192 = (512, 256, 0)  # the one stream whose index is cut every 8192 pixels


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
    """[(w, h, rgb, image, oracle stream, segment size, index)] of the mixed call: computed once, read by every test"""
    out = []
    for rgb, shapes in ((0, GRAY), (1, RGB)):
        for w, h in shapes:
            im = ic.images(w, h, rgb, 1)[0]
            stream = oracle.compress(im)
            seg = 8192 if (w, h, rgb) == AT_8192 else 4096
            out.append((w, h, rgb, im, stream, seg, api.index_build(stream, seg)))
    return out


def _hdr(im):
    return (int(im.ndim == 3), 0, im.shape[1], im.shape[0])


def _targets(cases, windows_of):
    """every window windows_of(w, h) of every stream into every layout: (regions, views, surfaces, plan rows)"""
    regions, views, surfaces, rows = [], [], [], []
    for s, (w, h, rgb, im, stream, seg, index) in enumerate(cases):
        for window in windows_of(w, h):
            need, waves, pixels = rv.plan(w, h, seg, 3 if rgb else 1, window)
            for name, shape, fs in vc.layouts(window[3], window[2], rgb):
                m = vc.Surface(shape)
                surfaces.append(("%dx%d rgb %d %s %s" % (w, h, rgb, window, name), m))
                for f in fs:
                    views.append(m.view(f, rc.crop(im, window)))
                    regions.append((s,) + tuple(window))
                    rows.append((w, rgb, window[2], window[3], waves, pixels, (3 if rgb else 1) * ic.Layout(index).k))
    return regions, views, surfaces, rows


def test_mixed_shapes_in_one_call(api, enc, cases):
    """ten streams of nine shapes, every FIXED window of each into every layout, several regions to a stream, ONE call: the crops of
    the originals, untouched fill, unchanged inputs; the counters are the plan by marking"""
    regions, views, surfaces, rows = _targets(cases, lambda w, h: rc.FIXED[(w, h)])
    assert len(regions) > 100 and len({r[0] for r in regions}) == len(cases)
    p = rv.Inputs([c[4] for c in cases], [c[6] for c in cases], 16)
    s0, other0 = enc.region_view_stats(), (enc.region_stats(), enc.index_view_stats())
    code, hdrs, st = rv.device_call(api, enc, False, p, regions, views)
    assert code == rv.OK and (st == rv.OK).all(), st
    assert hdrs == [_hdr(c[3]) for c in cases]
    for what, m in surfaces:
        m.check(what)
    p.check()
    d = rv.delta(enc.region_view_stats(), s0)
    assert d["regions"] == len(regions) and d["undecoded"] == 0
    assert d["segments_walked"] == sum(r[4] for r in rows)
    assert d["segments_skipped"] == sum(r[6] - r[4] for r in rows)
    assert d["pixels_walked"] == sum(r[5] for r in rows)
    npass, nlaunch, most = rv.passes_and_launches(rows, 1 << 62, False)
    assert (d["passes"], d["launches"]) == (npass, nlaunch) == (1, 3)  # (rows of 1 .. 100, of 4096 .. 5000 and of 8200 samples)
    assert enc.region_view_stats()["plane_bytes"] == most
    assert (enc.region_stats(), enc.index_view_stats()) == other0  # (the other region and view counters do not count these calls)
    part = api._CRegionViewStats(*[7] * 8)
    assert api.lib().felics_get_region_view_stats(enc._h, C.byref(part), 16) == 0
    now = enc.region_view_stats()
    assert (part.regions, part.undecoded, part.segments_walked, part.plane_bytes) == (now["regions"], now["undecoded"], 7, 7)


def test_a_plan_with_a_hole(api, enc, cases):
    """(5000, 0, 100, 2) of 8200 x 2 needs segments 1 and 3 and not 2"""
    case = next(c for c in cases if c[:3] == (8200, 2, 0))
    window = (5000, 0, 100, 2)
    assert rc.needed_by_marking(8200, 2, 4096, window) == [1, 3]
    m = vc.Surface((2, 113))
    view = m.view(lambda a: a[:, :100], rc.crop(case[3], window))
    p = rv.Inputs([case[4]], [case[6]], 16)
    s0 = enc.region_view_stats()
    code, hdrs, st = rv.device_call(api, enc, False, p, [(0,) + window], [view])
    assert code == rv.OK and list(st) == [rv.OK]
    m.check()
    d = rv.delta(enc.region_view_stats(), s0)
    assert (d["segments_walked"], d["segments_skipped"]) == (2, 3)
    assert d["pixels_walked"] == 4096 + (8200 + 5100 - 3 * 4096)


def test_full_frame_window_is_the_views_call(api, enc, cases):
    """the full-frame window of every stream: byte for byte what felics_decompress_views_device_indexed writes into the same views"""
    regions, views, surfaces, _ = _targets(cases, lambda w, h: [(0, 0, w, h)])
    stream_of = [r[0] for r in regions]
    p = rv.Inputs([cases[s][4] for s in stream_of], [cases[s][6] for s in stream_of], 16)  # (the views call: a stream per view)
    code, hdrs, st = rv.device_call(api, enc, False, p, [(i,) + r[1:] for i, r in enumerate(regions)], views)
    assert code == rv.OK and (st == rv.OK).all()
    got = [m.dev.cpu().numpy() for _, m in surfaces]
    for _, m in surfaces:
        m.check()
        m.dev.fill_(vc.FILL)
    hd, st = enc.decompress_views_device_indexed(p.streams_ptr, p.offs, p.lens, p.index_ptr, p.ioffs, p.ilens, views)
    assert (st == rv.OK).all()
    for (what, m), g in zip(surfaces, got):
        assert (m.dev.cpu().numpy() == g).all(), what
    p.check()


def test_passes(api, enc, cases):
    """five RGB windows of 200 pixels capped at two a pass, gray windows among them: three passes, the launches of the plan, the
    same samples as uncapped"""
    rgb100 = next(i for i, c in enumerate(cases) if c[:3] == (100, 100, 1))
    wide = next(i for i, c in enumerate(cases) if c[:3] == (8200, 2, 0))
    wins = [(rgb100, 10, 10, 20, 10), (wide, 5000, 0, 100, 2), (rgb100, 90, 40, 10, 20), (rgb100, 0, 0, 20, 10), (rgb100, 80, 90, 20, 10),
            (wide, 4100, 1, 50, 1), (rgb100, 33, 40, 40, 5)]
    p = rv.Inputs([c[4] for c in cases], [c[6] for c in cases], 16)
    out = []
    for cap in (None, 2 * 6 * 200):
        views, surfaces, rows = [], [], []
        for r in wins:
            w, h, rgb, im, _, seg, _ = cases[r[0]]
            m = vc.Surface((r[4] + 2, r[3] + 3, 4) if rgb else (r[4] + 2, r[3] + 3))
            f = (lambda a, r=r: a[1:1 + r[4], 2:2 + r[3], :3]) if rgb else (lambda a, r=r: a[1:1 + r[4], 2:2 + r[3]])
            views.append(m.view(f, rc.crop(im, r[1:])))
            surfaces.append(m)
            rows.append((w, rgb, r[3], r[4], rv.plan(w, h, seg, 3 if rgb else 1, r[1:])[1]))
        s0 = enc.region_view_stats()
        with rv.Env(**({"FELICS_TEST_INDEX_VIEWS_PASS": str(cap)} if cap else {})):
            code, hdrs, st = rv.device_call(api, enc, False, p, wins, views)
        assert code == rv.OK and (st == rv.OK).all()
        for m in surfaces:
            m.check()
        d = rv.delta(enc.region_view_stats(), s0)
        npass, nlaunch, most = rv.passes_and_launches(rows, cap or 1 << 62, False)
        assert (d["passes"], d["launches"], enc.region_view_stats()["plane_bytes"]) == (npass, nlaunch, most)
        assert npass == (3 if cap else 1) and most == (2400 if cap else 6000)
        out.append([m.dev.cpu().numpy() for m in surfaces])
    assert all((a == b).all() for a, b in zip(*out))
    p.check()


def test_per_region_isolation(api, enc, cases, oracle):
    """one call: a window outside its stream's image, a view of the other depth, a stream with a bad header, a forged bit offset in
    a needed segment and the same forgery where no region needs it, intact regions around them.  Every code is the host model's; a
    region refused before the launch leaves its surface untouched, every intact one holds its crop."""
    _, _, _, cimg, cstream, _, cidx = next(c for c in cases if c[:3] == (100, 100, 1))
    _, _, _, gimg, gstream, _, gidx = next(c for c in cases if c[:3] == (100, 100, 0))
    forged = ic.corruptions(cidx)["offset_plus_1"]  # checkpoint (0, 1) moved by a bit: segment (0, 0) no longer ends on it
    nosig = b"FLCX" + cstream[4:]
    streams = [cstream, gstream, nosig, cstream, cstream]
    indexes = [cidx, gidx, cidx, forged, forged]
    to_seg0_end, in_seg0 = (90, 40, 10, 2), (0, 0, 100, 40)
    # (stream, window, the view's size, depth of the view, may its samples be written)
    entries = [
        (0, (33, 40, 31, 3), None, 0, False),
        (0, (90, 90, 20, 20), None, 0, False),   # outside the image
        (1, (33, 40, 31, 3), None, 0, False),
        (1, (10, 10, 20, 4), None, 1, False),    # a 16-bit view of an 8-bit stream
        (2, (10, 10, 5, 5), None, 0, False),     # the stream with the bad header
        (1, (90, 40, 10, 2), None, 0, False),
        (3, to_seg0_end, None, 0, True),         # needs segment (0, 0) to its end: refused by the walk
        (4, in_seg0, None, 0, False),            # the same forgery, not needed: served
        (0, (0, 0, 100, 100), None, 0, False),
    ]
    p = rv.Inputs(streams, indexes, 16)
    regions, views, surfaces, want = [], [], [], []
    for s, window, _, depth, loose in entries:
        rgb = streams[s] is not gstream
        img = cimg if rgb else gimg
        x, y, w, h = window
        shape = (h + 2, 2 * w + 6, 3) if rgb else (h + 2, 2 * w + 6)
        m = vc.Surface(shape)
        host = np.full(shape, vc.FILL, np.uint8)
        f = lambda a, w=w, h=h: a[1:1 + h, 2:2 + w]  # noqa: E731
        view = m.view(f)
        hview = rv.host_view(f(host), False)
        if depth:  # the same place as a view of depth 16 (even address and strides)
            view, hview = ((t[0] + t[0] % 2,) + t[1:4] + (1, t[5] + t[5] % 2, 2, 0) for t in (view, hview))
        code = rv.host_call(api, False, streams[s], indexes[s], window, hview)
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
    s0 = enc.region_view_stats()
    code, hdrs, st = rv.device_call(api, enc, False, p, regions, views)
    assert list(st) == want and code == want[1]
    for i, m in enumerate(surfaces):
        m.check("entry %d" % i)
    p.check()
    assert hdrs[2] == (0, 0, 0, 0) and hdrs[0] == hdrs[3] == (1, 0, 100, 100)
    assert rv.delta(enc.region_view_stats(), s0)["undecoded"] == 3


def test_refusals_before_launch(api, enc, cases, oracle):
    """a misaligned index, a stream number too large, a view of another size than its window, an aliasing view, a ticket
    outstanding: the code in every status; a call whose only stream is 16-bit: FELICS_E_UNSUPPORTED in every status.  Every surface
    and the counters stay as they were."""
    import torch

    _, _, _, img, stream, _, index = next(c for c in cases if c[:3] == (100, 100, 0))
    m = vc.Surface((3, 12, 40))
    regions = [(k % 2, 10 * k, 5, 31, 10) for k in range(3)]
    views = [m.view(lambda a, k=k: a[k, 1:11, 3:34]) for k in range(3)]
    p = rv.Inputs([stream] * 2, [index] * 2, 16)
    s0 = enc.region_view_stats()

    def refused(code=rv.E_INVALID_ARGUMENT, regions=regions, views=views, inputs=p, **kw):
        rc_, hdrs, st = rv.device_call(api, enc, False, inputs, regions, views, **kw)
        assert rc_ == code and (st == code).all(), (rc_, st)
        m.check()
        assert rv.delta(enc.region_view_stats(), s0)["segments_walked"] == 0

    odd = p.ioffs.copy()
    odd[1] += 8
    refused(ioffs=odd)
    refused(regions=[regions[0], (2,) + regions[1][1:], regions[2]])
    refused(views=[views[0], views[1][:1] + (30,) + views[1][2:], views[2]])
    refused(views=[views[0], views[1], views[2][:2] + (9,) + views[2][3:]])
    refused(views=[views[0], views[1][:5] + (0, 1, 0), views[2]])  # row_stride = 0 with 10 rows
    assert enc.region_view_stats() == s0
    s16 = oracle.compress(np.arange(100 * 100, dtype=np.uint16).reshape(100, 100))
    refused(code=rv.E_UNSUPPORTED, inputs=rv.Inputs([s16] * 2, [index] * 2, 16))
    s0 = enc.region_view_stats()
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
    hd, st = enc.decompress_region_views_device_indexed(p.streams_ptr, p.offs, p.lens, p.index_ptr, p.ioffs, p.ilens, regions, views)
    assert (st == rv.OK).all() and [(h.width, h.height) for h in hd] == [(100, 100)] * 2
    m.check()
    with pytest.raises(api.FelicsError) as ei:
        enc.decompress_region_views_device_indexed(p.streams_ptr, p.offs, p.lens, p.index_ptr, p.ioffs, p.ilens,
                                                   [regions[0], (0, 95, 0, 31, 10), regions[2]], views)
    assert ei.value.code == rv.E_INVALID_ARGUMENT and list(ei.value.status) == [rv.OK, rv.E_INVALID_ARGUMENT, rv.OK]
    p.check()


def test_empty_regions(api, enc, cases):
    """empty windows, the far corner among them, with zero-sized views: their stream's header and index-header code and no walk;
    n_regions = 0"""
    good = next(c for c in cases if c[:3] == (100, 100, 1))
    bad = ic.corruptions(good[6])["version"]
    p = rv.Inputs([good[4], good[4]], [good[6], bad], 16)
    regions = [(0, 0, 0, 0, 0), (0, 100, 100, 0, 0), (0, 0, 0, 100, 0), (0, 50, 50, 0, 1), (1, 100, 100, 0, 0), (1, 0, 0, 0, 7)]
    views = [(0, r[3], r[4], 1, 0, 0, 0, 0) for r in regions]
    s0 = enc.region_view_stats()
    code, hdrs, st = rv.device_call(api, enc, False, p, regions, views)
    assert list(st) == [rv.OK] * 4 + [rv.E_INVALID_INDEX] * 2 and code == rv.E_INVALID_INDEX
    d = rv.delta(enc.region_view_stats(), s0)
    k = ic.Layout(good[6]).k
    assert (d["regions"], d["undecoded"], d["segments_walked"], d["pixels_walked"], d["launches"], d["passes"]) == (6, 2, 0, 0, 0, 0)
    assert d["segments_skipped"] == 4 * 3 * k
    for r, v in zip(regions, views):
        assert rv.host_call(api, False, good[4], good[6] if r[0] == 0 else bad, r[1:], v) == (rv.OK if r[0] == 0 else rv.E_INVALID_INDEX)
    code, hdrs, st = rv.device_call(api, enc, False, p, [], [])
    assert code == rv.OK and hdrs == [(0, 0, 0, 0)] * 2
    hd, st = enc.decompress_region_views_device_indexed(p.streams_ptr, p.offs, p.lens, p.index_ptr, p.ioffs, p.ilens, [], [])
    assert len(st) == 0
    p.check()


def test_ready_event(api, cases):
    """As tests/test_index_views_gpu.py::test_ready_event: a side stream stalls, then copies streams and indexes to the device and
    writes the fill over the surfaces; the call gets the event recorded behind that work and no host synchronisation.  Had a library
    stream started early it would have read zeros for a stream or an index (a status) or been overwritten by the fill."""
    import torch

    import felics_amd

    e = felics_amd.Encoder(0)
    try:
        pick = [(100, 100, 0), (64, 64, 1), (512, 256, 0), (100, 100, 1)]
        sel = [next(c for c in cases if c[:3] == k) for k in pick]
        wins = [(33, 40, 31, 3), (10, 10, 5, 5), (100, 100, 200, 50), (90, 40, 10, 2)]
        specs = [lambda a: a[:, :31], lambda a: a[..., :3], lambda a: a[::-1], lambda a: a.transpose(1, 2, 0)]
        shapes = [(3, 44), (5, 5, 4), (50, 200), (3, 2, 10)]
        surfs, views = [], []
        for c, win, f, shape in zip(sel, wins, specs, shapes):
            m = vc.Surface(shape)
            views.append(m.view(f, rc.crop(c[3], win)))
            surfs.append(m)
        p = rv.Inputs([c[4] for c in sel], [c[6] for c in sel], 16)
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
        code, hdrs, st = rv.device_call(api, e, False, p, [(i,) + w for i, w in enumerate(wins)], views, ready_event=ev.cuda_event)
        assert code == rv.OK and (st == rv.OK).all(), "a stream or an index was read before the producer had written it"
        for m in surfs:
            m.check()
        p.check()
        del big
    finally:
        e.close()


def test_torch_targets(api, enc, cases):
    """decompress_region_arrays_device_indexed: a window of every RGB stream and of a gray one into the slices of batch tensors"""
    import torch

    rgbs = [i for i, c in enumerate(cases) if c[2]]
    gray = next(i for i, c in enumerate(cases) if c[:3] == (512, 256, 0))
    p = rv.Inputs([c[4] for c in cases], [c[6] for c in cases], 16)
    batch = torch.full((len(rgbs), 3, 20, 30), 0x5A, dtype=torch.uint8, device="cuda")
    tile = torch.full((64, 80), 0x5A, dtype=torch.uint8, device="cuda")
    regions = [(s, 7, 9, 30, 20) for s in rgbs] + [(gray, 100, 100, 40, 32)]
    arrays = [batch[i].permute(1, 2, 0) for i in range(len(rgbs))] + [tile[16:48, 20:60]]
    torch.cuda.synchronize()
    hd, st = enc.decompress_region_arrays_device_indexed(p.streams_ptr, p.offs, p.lens, p.index_ptr, p.ioffs, p.ilens, regions, arrays)
    assert (st == rv.OK).all() and len(hd) == len(cases)
    want = np.stack([cases[s][3][9:29, 7:37].transpose(2, 0, 1) for s in rgbs])
    assert torch.equal(batch, torch.from_numpy(want).cuda())
    wt = np.full((64, 80), 0x5A, np.uint8)
    wt[16:48, 20:60] = cases[gray][3][100:132, 100:140]
    assert torch.equal(tile, torch.from_numpy(wt).cuda())
    p.check()
