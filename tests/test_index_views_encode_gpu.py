"""Indexed encode of views and mixed shapes (felics_compress_views_device_indexed), on the GPU.

The reference for a stream is the CPU oracle's of the dense copy of the view, the reference for an index felics_index_build of that
stream.  Streams and indexes are written between guard bytes of 0x5A, the indexes 16 bytes apart from each other, and both buffers
are read back WHOLE after every call: what is not a stream's slot or an index must still hold 0x5A."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import index_common as ic

pytestmark = pytest.mark.gpu
GUARD = 256
E_BUFFER_TOO_SMALL, E_UNSUPPORTED, E_INVALID_ARGUMENT = -8, -10, -11


@pytest.fixture(scope="module")
def api():
    from felics_amd import api as a

    return a


@pytest.fixture(scope="module")
def enc():
    """a default context (no test variable set)"""
    import felics_amd

    e = felics_amd.Encoder(0)
    yield e
    e.close()


class Surface:
    """A host array and its copy in device memory; view(v) turns a numpy view of the host array into the library's view tuple."""

    def __init__(self, host, upload=True):
        import torch

        self.host = np.ascontiguousarray(host)
        self.dev = torch.from_numpy(self.host if upload else np.zeros_like(self.host)).cuda()
        torch.cuda.synchronize()
        self.base = self.host.__array_interface__["data"][0]

    def view(self, v):
        from felics_amd import api

        h, w = v.shape[:2]
        color, depth = int(v.ndim == 3), int(v.dtype == np.uint16)
        if h * w == 0:
            return (0, w, h, color, depth, 0, 0, 0)
        off = v.__array_interface__["data"][0] - self.base
        t = (self.dev.data_ptr() + off, w, h, color, depth, v.strides[0], v.strides[1], v.strides[2] if v.ndim == 3 else 0)
        lo, hi = api.view_extent(t)
        assert off + lo >= 0 and off + hi <= self.host.nbytes, (lo, hi, off)  # the caller's bounds check
        return t


def _dense(img):
    s = Surface(img)
    return (s, s.host)


class Result:
    pass


def _run(e, api, pairs, segs, cap=None, producer=None):
    """One call on pairs = [(surface, numpy view), ...] with segs[i] pixels per segment (0: no index).  Indexes where index_plan puts
    them plus 16 bytes of gap in front of each; guards and gaps checked.  producer: started once the buffers stand, returns the
    ready event (and what must stay alive); the host does not wait for it.  Returns the streams and indexes as bytes and the device
    buffers as they lie."""
    import torch

    views = [s.view(v) for s, v in pairs]
    dense = [np.ascontiguousarray(v) for _, v in pairs]
    n = len(views)
    planned, ilens, _ = api.index_plan(views, segs)
    ioffs = planned + np.uint64(16) * (np.arange(n, dtype=np.uint64) + np.uint64(1))
    icap = int((ioffs + ilens).max()) if n else 0
    if cap is None:
        cap = sum(d.size * d.itemsize * 5 // 4 + 96 for d in dense) + 4096
    r = Result()
    r.d_out = torch.full((GUARD + cap + GUARD,), 0x5A, dtype=torch.uint8, device="cuda")
    r.d_idx = torch.full((GUARD + max(icap, 16) + GUARD,), 0x5A, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ready_event, keep = producer() if producer else (None, None)
    r.offs, r.lens, r.ioffs, r.ilens = e.compress_views_device_indexed(views, segs, r.d_out.data_ptr() + GUARD, cap, r.d_idx.data_ptr() + GUARD, icap,
                                                                     idx_offsets=ioffs, ready_event=ready_event)
    assert (r.ilens == ilens).all() and (r.ioffs == ioffs).all()
    del keep
    out, idx = r.d_out.cpu().numpy(), r.d_idx.cpu().numpy()
    assert (out[:GUARD] == 0x5A).all() and (out[GUARD + cap:] == 0x5A).all(), "guard bytes around d_out"
    untouched = np.ones(len(idx), bool)
    for o, ln in zip(ioffs, ilens):
        untouched[GUARD + int(o):GUARD + int(o) + int(ln)] = False
    assert (idx[untouched] == 0x5A).all(), "guard bytes around d_index and the gaps between the indexes"
    assert all(int(o) % 16 == 0 for o in r.offs)
    r.streams = [out[GUARD + int(o):GUARD + int(o) + int(ln)].tobytes() for o, ln in zip(r.offs, r.lens)]
    r.indexes = [idx[GUARD + int(o):GUARD + int(o) + int(ln)].tobytes() for o, ln in zip(ioffs, ilens)]
    r.views, r.dense, r.segs, r.cap, r.icap = views, dense, list(segs), cap, icap
    return r


def _check(r, oracle, api, what=""):
    """streams against the oracle's of the dense copies, indexes against felics_index_build of those; returns the reference indexes"""
    refs = []
    for i, (img, seg) in enumerate(zip(r.dense, r.segs)):
        want = oracle.compress(img)
        assert r.streams[i] == want, "%s view %d %s: stream differs at %s" % (what, i, img.shape, ic.first_difference(r.streams[i], want))
        ref = api.index_build(want, seg) if seg else b""
        d = ic.first_difference(r.indexes[i], ref)
        assert d is None, "%s view %d %s segment %d: index differs at %d of %d / %d: %s" % (
            what, i, img.shape, seg, d, len(r.indexes[i]), len(ref), ic.where_in_index(ref, d) if d < len(ref) else "length")
        refs.append(ref)
    return refs


def _delta(after, before):
    return {k: after[k] - before[k] for k in after}


def _buckets(shapes):
    """sub-batches the 1.25 rule gives images of one colour: sorted by tiles T, a bucket holds T_min .. ceil(1.25 T_min)"""
    tiles = sorted((w * h + 4095) // 4096 for w, h in shapes if w * h)
    count = 0
    while tiles:
        lim = (5 * tiles[0] + 3) // 4
        tiles = [t for t in tiles if t > lim]
        count += 1
    return count


def test_every_small_shape_in_one_call(enc, api, oracle):
    """All of index_common.SHAPES, the empty ones included, gray and RGB, as dense views in ONE call, the segment alternating."""
    keys = [(w, h, rgb) for w, h in ic.SHAPES for rgb in (0, 1)]
    pairs = [_dense(ic.images(w, h, rgb, 1)[0]) for w, h, rgb in keys]
    segs = [ic.SEGMENTS[i % 2] for i in range(len(keys))]
    before, sub = enc.index_emit_stats(), enc.stats()["submissions"]
    r = _run(enc, api, pairs, segs)
    refs = _check(r, oracle, api, "small shapes")
    d = _delta(enc.index_emit_stats(), before)
    asked = sum(1 for w, h, _ in keys if w * h)
    assert d == {"indexes": asked, "in_mixed": asked, "redone": 0,
                 "checkpoints": sum(ic.Layout(x).planes * ic.Layout(x).k for x in refs)}, d
    assert all(len(x) == 64 for x, (w, h, _) in zip(r.indexes, keys) if w * h == 0)
    assert enc.stats()["submissions"] - sub <= 2 * _buckets(ic.SHAPES) < len(keys) // 2
    # the struct: a short out_size leaves the rest of the caller's struct alone
    st = api._CIndexEmitStats(7, 7, 7, 7)
    assert api.lib().felics_get_index_emit_stats(enc._h, C.byref(st), 16) == 0
    assert st.indexes >= asked and (st.in_mixed, st.redone) == (7, 7)


@pytest.fixture(scope="module")
def every_class(enc, api):
    """One call with a view of every class (the result, shared by the two tests below)."""
    rng = np.random.default_rng(71)
    from felics_amd import synth

    s128 = Surface(synth.gray8(128, 110, 1, "S1"))
    s64 = Surface(rng.integers(0, 256, (125, 64), np.uint8))
    s4224 = Surface(synth.gray8(4224, 3, 2, "S2"))
    rgba = Surface(np.concatenate([synth.rgb8(130, 70, 3), rng.integers(0, 256, (70, 130, 1), np.uint8)], axis=2))
    chw = Surface(np.ascontiguousarray(synth.rgb8(130, 70, 4).transpose(2, 0, 1)))
    wide = Surface(synth.gray8(250, 90, 5, "S1"))
    g16 = Surface(synth.gray16(80, 60, 6))
    pairs = [
        (s128, s128.host[3:103, 5:105]),        # 100 x 100 at (5, 3), pitch 128: segments start mid-row, the window crosses rows
        (s64, s64.host[2:122, 9:46]),           # 37 x 120, pitch 64: W < 64 and no multiple of 16
        (s4224, s4224.host[:, 100:4196]),       # 4096 x 3, pitch 4224: x0 = 0 on every boundary, the whole 2 W
        (rgba, rgba.host[..., :3]),             # RGBA read as RGB
        (rgba, rgba.host[..., 2::-1]),          # the same frame BGR
        (chw, chw.host.transpose(1, 2, 0)),     # planar C x H x W
        (wide, wide.host[:, ::2]),              # pixel_stride = 2: gathered
        (wide, wide.host[::-1, 20:150]),        # a negative row stride: gathered
        (g16, g16.host[5:50, 8:70]),            # 16-bit: its stream, no index
        (s64, s64.host[10:40, 3:33]),           # a small gray8 view without an index
    ]
    segs = [4096, 4096, 4096, 4096, 4096, 4096, 4096, 4096, 0, 0]
    before = enc.view_stats()
    r = _run(enc, api, pairs, segs)
    r.view_classes = _delta(enc.view_stats(), before)
    return r


def test_views_of_every_class(every_class, api, oracle):
    r = every_class
    _check(r, oracle, api, "classes")
    assert [int(v) for v in r.ilens[-2:]] == [0, 0] and all(int(v) > 64 for v in r.ilens[:-2])
    assert (r.view_classes["in_place"], r.view_classes["gathered"], r.view_classes["dense"]) == (7, 3, 0), r.view_classes
    assert [ic.Layout(x).k for x in r.indexes[:8]] == [3, 2, 3, 3, 3, 3, 3, 3]


def test_round_trip_on_the_device(every_class, enc):
    """The streams and indexes of the 8-bit indexed views, as they lie in device memory, decoded into fresh surfaces of other layouts."""
    import torch

    r = every_class
    keep = [i for i, s in enumerate(r.segs) if s]
    targets, views = [], []
    for i in keep:
        img = r.dense[i]
        h, w = img.shape[:2]
        if img.ndim == 2:  # a window of a pitched surface
            t = torch.full((h + 2, w + 13), 0xA5, dtype=torch.uint8, device="cuda")
            views.append((t.data_ptr() + (w + 13) + 5, w, h, 0, 0, w + 13, 1, 0))
            targets.append((t, lambda a, h=h, w=w: a[1:1 + h, 5:5 + w]))
        else:  # planar C x H x W
            t = torch.full((3, h, w), 0xA5, dtype=torch.uint8, device="cuda")
            views.append((t.data_ptr(), w, h, 1, 0, w, 1, h * w))
            targets.append((t, lambda a: a.transpose(1, 2, 0)))
    torch.cuda.synchronize()
    _, status = enc.decompress_views_device_indexed(r.d_out.data_ptr() + GUARD, r.offs[keep], r.lens[keep], r.d_idx.data_ptr() + GUARD,
                                                    r.ioffs[keep], r.ilens[keep], views)
    assert (status == 0).all(), status
    for i, (t, pick) in zip(keep, targets):
        assert (pick(t.cpu().numpy()) == r.dense[i]).all(), i


@pytest.mark.parametrize("rgb", (0, 1))
def test_large_k_and_padding_tiles(enc, api, oracle, rgb):
    """4096 x 132 (132 tiles) and 1000 x 541 (133 tiles, through a pitch-1024 surface) share a bucket: K = 132 and 133 at one tile
    per segment -- three chunks of intervals in the states kernel, a padding tile behind the shorter plane -- then 9 tiles per
    segment.  Banded content: contexts that stay silent over many checkpoints."""
    (w0, h0, _, plans0), (w1, h1, _, plans1) = ic.LARGE[0], ic.LARGE[1]
    assert (w0, h0, plans0[0]) == (4096, 132, (0, 1, 130, 131)) and (w1, h1, plans1[0]) == (1000, 541, (0, 65, 131))
    a = Surface(ic.banded(w0, h0, rgb, plans0[0]))
    wide = np.zeros((h1, 1024, 3) if rgb else (h1, 1024), np.uint8)
    wide[:, 12:12 + w1] = ic.banded(w1, h1, rgb, plans1[0])
    b = Surface(wide)
    pairs = [(a, a.host), (b, b.host[:, 12:12 + w1])]
    for seg_tiles in (1, 9):
        sub = enc.stats()["submissions"]
        r = _run(enc, api, pairs, [seg_tiles * ic.GRANULE] * 2)
        assert enc.stats()["submissions"] - sub == 1  # one bucket
        _check(r, oracle, api, "large, %d tiles per segment" % seg_tiles)
        if seg_tiles == 1:
            assert [ic.Layout(x).k for x in r.indexes] == [132, 133]
            for index, (w, h, plan) in zip(r.indexes, ((w0, h0, plans0[0]), (w1, h1, plans1[0]))):
                rows = ic.state_rows(index)
                for what, least in ic.measures(w, h, 1, plan):
                    assert ic.measure(rows, what) >= least, (w, h, what, ic.measure(rows, what))


REMEDIES = {"FELICS_TEST_LOOKBACK_FAIL": "lookback_fallbacks", "FELICS_TEST_SCATTER_ORDER": "scatter_fallbacks", "FELICS_TEST_TILE_CAP": "tile_overflows",
            "FELICS_TWO_PASS": "two_pass", "exact": None}


@pytest.mark.parametrize("variant", list(REMEDIES))
def test_remedies(api, oracle, variant):
    """Each remedy of a sub-batch, and exact placement (a d_out of exactly the rounded sizes: a first run for the sizes, a second
    that places the streams), on a fresh context with FELICS_POISON on: streams and indexes exact, the counters moved, and the
    same call once more on the context."""
    import felics_amd
    from felics_amd import synth

    env = {variant: "1"} if variant.startswith("FELICS_") else {}
    grays = [_dense(synth.gray8(300 + 17 * i, 200 + 11 * i, i, "S1")) for i in range(6)]
    rgbs = [_dense(synth.rgb8(120 + 9 * i, 90 + 5 * i, i)) for i in range(4)]
    big = Surface(synth.gray8(640, 400, 9, "S1"))
    pairs = grays + rgbs + [(big, big.host[7:300, 11:411]), (big, big.host[50:390, 100:620])]
    segs = [ic.SEGMENTS[i % 2] for i in range(len(pairs))]
    cap = sum((len(oracle.compress(np.ascontiguousarray(v))) + 15) // 16 * 16 for _, v in pairs) if variant == "exact" else None
    os.environ.update(env)
    os.environ["FELICS_POISON"] = "1"
    try:
        e = felics_amd.Encoder(0)
        try:
            _check(_run(e, api, pairs, segs, cap=cap), oracle, api, variant)
            st, ies = e.stats(), e.index_emit_stats()
            if REMEDIES[variant]:
                assert st[REMEDIES[variant]] >= 1, st
                assert ies["redone"] >= 1, ies
            else:  # no remedy: the run that placed the streams wrote every index, in the mixed kernels
                assert (ies["indexes"], ies["in_mixed"], ies["redone"]) == (len(pairs), len(pairs), 0), ies
            _check(_run(e, api, pairs, segs, cap=cap), oracle, api, variant + " again")
        finally:
            e.close()
    finally:
        for k in list(env) + ["FELICS_POISON"]:
            del os.environ[k]


def _slow_producer(stream, finals, surfaces):
    """On `stream`: tens of milliseconds of element-wise passes over a large tensor, then the copies that write the frames."""
    import torch

    with torch.cuda.stream(stream):
        big = torch.zeros(1 << 26, dtype=torch.float32, device="cuda")
        for _ in range(600):
            big.add_(1.0)
        for f, s in zip(finals, surfaces):
            s.copy_(f, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(stream)
    return ev, big


def test_ready_event(api, oracle):
    """The surfaces hold zeros; a producer on a side stream takes tens of milliseconds and writes the frames last; the call gets the
    event recorded behind it and no host synchronisation.  Streams and indexes must be those of the final frames.  (A race test in
    the one direction that cannot fail falsely; run once.)"""
    import torch

    import felics_amd
    from felics_amd import synth

    e = felics_amd.Encoder(0)
    try:
        final = [synth.gray8(1024, 600, 1, "S1"), np.concatenate([synth.rgb8(640, 360, 2), np.zeros((360, 640, 1), np.uint8)], axis=2),
                 synth.gray8(333, 222, 4, "S2")]
        surfs = [Surface(f, upload=False) for f in final]
        finals_dev = [torch.from_numpy(f).cuda() for f in final]
        pick = [(0, lambda a: a[3:590, 5:1000]), (1, lambda a: a[..., :3]), (0, lambda a: a[::-1, ::2]), (2, lambda a: a),
                (1, lambda a: a[5:300, 7:600, 2::-1])]
        pairs = [(surfs[k], f(surfs[k].host)) for k, f in pick]
        side = torch.cuda.Stream()

        def producer():
            ev, keep = _slow_producer(side, finals_dev, [s.dev for s in surfs])
            return ev.cuda_event, (ev, keep)

        # (the surfaces' host arrays hold the final frames, their device copies zeros until the producer has run)
        _check(_run(e, api, pairs, [16384] * len(pairs), producer=producer), oracle, api, "behind the producer's event")
    finally:
        e.close()


def test_refusals(enc, api):
    """Every refusal comes before anything is launched: d_index still holds 0x5A afterwards."""
    import torch

    frames = torch.zeros((2, 64, 65), dtype=torch.uint8, device="cuda")
    frames16 = torch.zeros((64, 65), dtype=torch.int16, device="cuda")
    out = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    views = [(frames[i].data_ptr(), 65, 64, 0, 0, 65, 1, 0) for i in range(2)]
    wide = (frames16.data_ptr(), 65, 64, 0, 1, 130, 2, 0)
    isize = ic.index_size(65, 64, 0, 4096)
    d_idx = torch.full((2 * isize + 64,), 0x5A, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    u64 = C.POINTER(C.c_uint64)

    def call(vs=views, segs=(4096, 4096), ioffs=(0, isize), icap=2 * isize, at=0, null=()):
        n = len(vs)
        cv = (api._CView * n)(*[api._cview(v) for v in vs])
        sg = (C.c_uint32 * n)(*segs)
        io = (C.c_uint64 * n)(*ioffs)
        offs, lens = (C.c_uint64 * n)(), (C.c_uint64 * n)()
        args = dict(views=cv, segs=sg, ioffs=io, offs=offs, lens=lens)
        for k in null:
            args[k] = None
        return api.lib().felics_compress_views_device_indexed(enc._h, n, args["views"], args["segs"], None, out.data_ptr(), out.numel(),
                                                              d_idx.data_ptr() + at, icap, args["ioffs"], args["offs"], args["lens"])

    for k in ("views", "segs", "ioffs", "offs", "lens"):
        assert call(null=(k,)) == E_INVALID_ARGUMENT, k
    assert call(ioffs=(0, isize + 8)) == E_INVALID_ARGUMENT      # an unaligned index offset
    assert call(at=8) == E_INVALID_ARGUMENT                      # ... an unaligned d_index
    assert call(ioffs=(0, isize - 16)) == E_INVALID_ARGUMENT     # overlapping indexes
    assert call(ioffs=(isize, 16)) == E_INVALID_ARGUMENT         # ... in either order
    assert call(icap=2 * isize - 1) == E_BUFFER_TOO_SMALL        # d_index_cap one byte short
    assert call(vs=[views[0], wide]) == E_UNSUPPORTED            # a 16-bit view with a segment
    assert call(segs=(4096, 6000)) == E_INVALID_ARGUMENT         # a bad segment
    sub = enc.submit_batch_device(frames.data_ptr(), 2, 65, 64, 0, 0, out.data_ptr(), out.numel())
    try:
        assert call() == E_INVALID_ARGUMENT                      # an outstanding ticket
    finally:
        enc.wait_batch(sub)
    assert (d_idx.cpu().numpy() == 0x5A).all()
    assert call() == 0
    assert call(vs=[views[0], wide], segs=(4096, 0)) == 0        # the 16-bit view takes part without an index
    host = d_idx.cpu().numpy()
    assert (host[2 * isize:] == 0x5A).all() and bytes(host[:4]) == b"FLCX"
