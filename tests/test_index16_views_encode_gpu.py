"""felics_compress_views_device_indexed16 on the GPU: the version-2 restart index written while encoding views and mixed shapes.

Every comparison is byte for byte: the streams against felics_compress_views_device's of the same views, every index against
api.index16_build of its stream.  The index buffer lies inside a pattern-filled allocation with guard bytes behind d_index_cap; the
library places the indexes, so the test checks that their ranges tile [0, idx_total) -- multiples of 64, no gap, no overlap -- and
that the pattern survives behind idx_total."""
import ctypes as C
import os

import numpy as np
import pytest

from tests import index16_common as ic
from tests import index16_encode_cases as ec
from tests import index16_views_encode_cases as vc
from tests.index16_views_encode_cases import Surface, dense

pytestmark = pytest.mark.gpu

PATTERN = 0x5A
GUARD = 4096
E_BUFFER_TOO_SMALL, E_UNSUPPORTED, E_INVALID_ARGUMENT = -8, -10, -11


@pytest.fixture(scope="module")
def api():
    from felics_amd import api as a

    return a


@pytest.fixture(scope="module")
def enc():
    import felics_amd

    e = felics_amd.Encoder(0)
    yield e
    e.close()


def _error(e):
    from felics_amd import api

    return api.lib().felics_last_error(e._h).decode()


def _cap_of(pairs):
    return sum(v.size * v.itemsize * 5 // 4 + 96 for _, v in pairs) + 4096


class Reference:
    """the views of a case, the streams felics_compress_views_device makes of them and the indexes index16_build makes of those: computed
    once per case, read by every call on it"""

    def __init__(self, e, api, pairs, segs):
        import torch

        self.pairs, self.segs = pairs, list(segs)
        self.views = [s.view(v) for s, v in pairs]
        cap = _cap_of(pairs) + sum(v.size * v.itemsize * 16 for _, v in pairs)  # (room for streams that outgrow their slots)
        d_out = torch.zeros(cap, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        offs, lens = e.compress_views_device(self.views, d_out.data_ptr(), cap)
        host = d_out.cpu().numpy()
        self.streams = [host[int(o):int(o + n)].tobytes() for o, n in zip(offs, lens)]
        self.indexes = [api.index16_build(s, seg) if seg else b"" for s, seg in zip(self.streams, self.segs)]
        self.need = sum(len(x) for x in self.indexes)


class Result:
    pass


def _call(e, ref, idx_cap, cap=None, expect=0, producer=None):
    """one raw call on the reference's views into an index buffer of idx_cap bytes inside a pattern-filled allocation with GUARD bytes
    behind it.  Checks the return code, and that nothing behind idx_cap changed.  producer: started once the buffers stand, returns
    the ready event (and what must stay alive); the host does not wait for it."""
    import torch

    r = Result()
    r.cap = cap = cap or _cap_of(ref.pairs)
    r.d_out = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    r.d_idx = torch.full((idx_cap + GUARD,), PATTERN, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert r.d_idx.data_ptr() % 64 == 0
    ready_event, keep = producer() if producer else (None, None)
    rc, r.offs, r.lens, r.ioffs, r.ilens, r.total = e.compress_views_device_indexed16_raw(ref.views, ref.segs, r.d_out.data_ptr(), cap, r.d_idx.data_ptr(),
                                                                                         idx_cap, ready_event)
    assert rc == expect, (rc, _error(e))
    del keep
    host = r.d_out.cpu().numpy()
    r.hidx = r.d_idx.cpu().numpy()
    assert (r.hidx[idx_cap:] == PATTERN).all(), "bytes behind d_index_cap"
    r.streams = [host[int(o):int(o + n)].tobytes() for o, n in zip(r.offs, r.lens)]
    return r


def _placement(r, ref):
    """idx_lens and idx_total are the reference's; the offsets are multiples of 64 and the ranges tile [0, idx_total) without gaps; a
    view without an index has offset and length 0.  Returns the views with an index in the order they were placed."""
    assert [int(n) for n in r.ilens] == [len(x) for x in ref.indexes] and r.total == ref.need
    placed = sorted((i for i, x in enumerate(ref.indexes) if x), key=lambda i: int(r.ioffs[i]))
    at = 0
    for i in placed:
        assert int(r.ioffs[i]) == at and at % 64 == 0, (i, int(r.ioffs[i]), at)
        at += len(ref.indexes[i])
    assert at == r.total
    assert all(int(r.ioffs[i]) == 0 for i, x in enumerate(ref.indexes) if not x)
    return placed


def _check(e, ref, slack=192, **kw):
    """a call with room for every index: streams, placement, every index, the pattern behind idx_total"""
    r = _call(e, ref, ref.need + slack, **kw)
    assert r.streams == ref.streams
    for i in _placement(r, ref):
        o, x = int(r.ioffs[i]), ref.indexes[i]
        assert r.hidx[o:o + len(x)].tobytes() == x, "view %d %s segment %d" % (i, ref.pairs[i][1].shape, ref.segs[i])
    assert (r.hidx[r.total:] == PATTERN).all(), "bytes behind idx_total"
    return r


def _delta(after, before):
    return {k: after[k] - before[k] for k in after}


def _mixed(rgb):
    frames, segs = vc.mixed_rgb() if rgb else vc.mixed_gray()
    return [dense(f) for f in frames], segs


@pytest.fixture(scope="module")
def mixed_refs(enc, api):
    return {rgb: Reference(enc, api, *_mixed(rgb)) for rgb in (0, 1)}


def test_mixed_gray(enc, mixed_refs):
    """the four gray shapes of one bucket three times over, segments cycling through 4096, 8192, 12 288 and 0, the views not in bucket
    order: one sub-batch, written by the table-driven kernels"""
    before = enc.index16_view_emit_stats()
    _check(enc, mixed_refs[0])
    d = _delta(enc.index16_view_emit_stats(), before)
    assert enc.index16_view_emit_stats()["shapes_max"] >= 3
    assert (d["views"], d["indexes"], d["sub_batches"], d["redone"]) == (12, 9, 1, 0), d


def test_mixed_rgb(enc, mixed_refs):
    before = enc.index16_view_emit_stats()
    _check(enc, mixed_refs[1])
    d = _delta(enc.index16_view_emit_stats(), before)
    assert enc.index16_view_emit_stats()["shapes_max"] >= 3
    assert (d["views"], d["indexes"], d["sub_batches"], d["redone"]) == (9, 7, 1, 0), d


def test_same_shape_group(enc, api):
    """frames of ONE shape that ask for different segments (and one for none): the bucket takes the uniform encode path, the same
    table-driven writer serves it with rows that all name one shape"""
    frames = [ic.noise(64, 130, 0, bits, 400 + bits) for bits in (12, 10, 8, 6)] + [ic.ramp(64, 130, 0)]
    ref = Reference(enc, api, [dense(f) for f in frames], [4096, 8192, 0, 4096, 12288])
    before = enc.index16_view_emit_stats()
    _check(enc, ref)
    d = _delta(enc.index16_view_emit_stats(), before)
    assert (d["indexes"], d["sub_batches"], d["redone"]) == (4, 1, 0) and enc.index16_view_emit_stats()["shapes_max"] == 1, d


def test_everything_in_one_call(enc, api):
    """every frame of the two case modules (the empty ones included), the mixed gray and RGB shapes, the second bucket, two frames of a
    shape that is alone in its bucket asking for two different segments, a gray8 and an RGB8 view with segment 0, a zero-sized gray16
    view with a segment, a 16-bit view with segment 0 between two that want one"""
    from felics_amd import synth

    frames, segs = [], []
    for k, (img, _) in enumerate({**ic.cases(), **ec.cases()}.values()):
        frames.append(img)
        segs.append((4096, 8192)[k % 2])
    for more in (vc.mixed_gray(), vc.mixed_rgb(), vc.second_bucket()):
        frames += more[0]
        segs += more[1]
    frames += [ic.noise(16128, 2, 0, 9, 90), synth.gray8(100, 90, 1, "S1"), synth.rgb8(60, 50, 2), np.zeros((0, 7), np.uint16)]
    segs += [8192, 0, 0, 4096]  # (16128 x 2 is in ic.cases() with 4096 or 8192: the other segment here)
    frames += [ic.noise(64, 130, 0, 10, 91), ic.noise(64, 130, 0, 10, 92), ic.noise(64, 130, 0, 10, 93)]
    segs += [4096, 0, 8192]
    assert segs[list(ic.cases()).index("16128x2")] == 4096
    ref = Reference(enc, api, [dense(f) for f in frames], segs)
    asked_empty = [i for i, f in enumerate(frames) if f.size == 0 and segs[i]]
    assert len(asked_empty) == 3 and all(len(ref.indexes[i]) == 64 for i in asked_empty)
    before = enc.index16_view_emit_stats()
    _check(enc, ref)
    d = _delta(enc.index16_view_emit_stats(), before)
    assert d["views"] == len(frames) and d["indexes"] == sum(1 for s in segs if s) - len(asked_empty) and d["redone"] == 0, d
    assert d["index_bytes"] == ref.need and d["sub_batches"] >= 4, d


def test_layouts(enc, api):
    """a pitched gray16 crop, every other column, bottom-up, RGBA read as RGB, BGR (channel_stride = -2), planar C x H x W: the indexes
    are those of the dense copies' streams"""
    rng = np.random.default_rng(7)
    big = Surface(ic.noise(200, 140, 0, 11, 71))
    rgba = Surface(np.concatenate([ic.noise(48, 100, 1, 10, 72), rng.integers(0, 65536, (100, 48, 1), np.uint16)], axis=2))
    chw = Surface(np.ascontiguousarray(ic.noise(40, 150, 1, 10, 73).transpose(2, 0, 1)))
    pairs = [
        (big, big.host[3:133, 5:69]),         # 64 x 130 at (5, 3), pitch 200
        (big, big.host[:, ::2]),              # pixel_stride = 4
        (big, big.host[::-1, 20:84]),         # a negative row stride
        (rgba, rgba.host[..., :3]),           # RGBA read as RGB
        (rgba, rgba.host[..., 2::-1]),        # the same frame BGR
        (chw, chw.host.transpose(1, 2, 0)),   # planar
    ]
    assert pairs[4][1].strides[2] == -2
    ref = Reference(enc, api, pairs, [4096, 8192, 4096, 4096, 8192, 4096])
    for (_, v), s in zip(pairs, ref.streams):  # (the reference's streams are those of the dense copies)
        assert s == Reference(enc, api, [dense(np.ascontiguousarray(v))], [0]).streams[0]
    _check(enc, ref)


def test_short_index_buffer(enc, mixed_refs):
    """d_index_cap short by 64 bytes, by the last-placed index and 64, and by everything: -8, complete streams, the right totals, every
    index that fits right, nothing of the others begun and nothing behind the cap; a second call with idx_total succeeds"""
    ref = mixed_refs[0]
    full = _check(enc, ref, slack=0)
    last = max((i for i, x in enumerate(ref.indexes) if x), key=lambda i: int(full.ioffs[i]))
    for short in (64, len(ref.indexes[last]) + 64, ref.need):
        cap = ref.need - short
        r = _call(enc, ref, cap, expect=E_BUFFER_TOO_SMALL)
        assert r.streams == ref.streams
        untouched = np.ones(cap, bool)
        for i in _placement(r, ref):
            o, x = int(r.ioffs[i]), ref.indexes[i]
            if o + len(x) <= cap:
                assert r.hidx[o:o + len(x)].tobytes() == x, i
                untouched[o:o + len(x)] = False
        assert (r.hidx[:cap][untouched] == PATTERN).all(), "an index that does not fit is not begun"
    _check(enc, ref, slack=0)


def _spiky(w, h, spikes, seed):
    """samples 0 / 1 above a flat lower half that holds, for each of `spikes` contexts d = 2, 3, ...: an event of operand 0 in context d
    (left neighbour d, the one above 0, the sample d + 1), whose Rice parameter so settles at 0, and two rows on a full-scale spike in
    the same context -- a unary run of about 65 000 bits, 8 KB, each.  Six of them: a stream of 50 KB for a frame of 16 to 24 KB."""
    f = ic.chosen(w, h, (0, 1), seed)
    f[h // 2:] = 0
    for i in range(spikes):
        d, y = 2 + i, h // 2 + 2 + 4 * i
        f[y, 5], f[y, 6] = d, d + 1
        f[y + 2, 5], f[y + 2, 6] = d, 65535
    return f


def test_slot_overflow_and_exact_run(api):
    """A stream that outgrows its slot inside the mixed bucket, one inside a same-shape group, and a d_out_cap that cannot hold the
    slots: streams and indexes as ever.

    The slots of this call are felics_compress_views_device's -- the frame's size and a quarter, whatever d_out_cap is -- and a
    full-range noise frame compresses to 1.07 of its size, so it cannot outgrow one (measured with the oracle: 17 729 bytes for the
    16 640 of a 64 x 130 frame, slot 20 864).  The noise frame stays in the bucket; the overflow felics_stats.slot_overflows counts
    comes from a frame of full-scale spikes beside it, whose stream is many times its frame.  A d_out_cap a little under the sum of
    the slots takes the sizes-only run and the exact second run, and no remedy."""
    import felics_amd

    rng = np.random.default_rng(5)
    frames, segs = vc.mixed_gray()
    frames = frames[:6] + [rng.integers(0, 65536, size=(130, 64), dtype=np.uint16), _spiky(96, 128, 6, 3)]
    segs = segs[:6] + [4096, 8192]
    group = [ic.noise(64, 130, 0, 10, 31), _spiky(64, 130, 6, 4), ic.noise(64, 130, 0, 8, 32)]
    with felics_amd.Encoder(0) as e:
        ref = Reference(e, api, [dense(f) for f in frames], segs)
        assert len(ref.streams[7]) > frames[7].nbytes * 5 // 4 + 64 > 0 and len(ref.streams[6]) < frames[6].nbytes * 5 // 4
        before, st = e.stats()["slot_overflows"], e.index16_view_emit_stats()
        _check(e, ref, cap=_cap_of(ref.pairs) + 2 * len(ref.streams[7]))
        d = _delta(e.index16_view_emit_stats(), st)
        assert e.stats()["slot_overflows"] >= before + 1 and d["redone"] >= 1, (e.stats(), d)
        # the same inside a group of one shape, with two segments
        gref = Reference(e, api, [dense(f) for f in group], [4096, 8192, 4096])
        before, st = e.stats()["slot_overflows"], e.index16_view_emit_stats()
        _check(e, gref, cap=_cap_of(gref.pairs) + 2 * len(gref.streams[1]))
        d = _delta(e.index16_view_emit_stats(), st)
        assert e.stats()["slot_overflows"] >= before + 1 and d["redone"] >= 1, (e.stats(), d)
        # a buffer that cannot hold the slots: a little under their sum, and exactly the rounded sizes
        quiet = Reference(e, api, [dense(f) for f in frames[:7]], segs[:7])
        slots = sum((f.nbytes + f.nbytes // 4 + 64 + 15) // 16 * 16 for f in frames[:7])
        for cap in (slots - 16, sum((len(s) + 15) // 16 * 16 for s in quiet.streams)):
            before, st = e.stats()["slot_overflows"], e.index16_view_emit_stats()
            _check(e, quiet, cap=cap)
            d = _delta(e.index16_view_emit_stats(), st)
            assert e.stats()["slot_overflows"] == before and (d["indexes"], d["redone"]) == (6, 0), d


@pytest.mark.parametrize("env", ({"FELICS_WIDE_LANE": "0"}, {"FELICS_WIDE_LANE": "1"}, {"FELICS_WIDE_LANE": "7"}, {"FELICS_POISON": "1"},
                                 {"FELICS_TEST_INDEX16_EMIT_CPS": "5"}), ids=lambda e: "-".join("%s=%s" % kv for kv in e.items()))
def test_forced_variants(api, env):
    """the mixed cases whichever chain kernel gave the events their k, on a poisoned workspace, and with sub-batches of five checkpoints
    at most: the cut of the gray bucket shows in sub_batches"""
    import felics_amd

    os.environ.update(env)
    try:
        with felics_amd.Encoder(0) as e:
            for rgb in (0, 1):
                pairs, segs = _mixed(rgb)
                ref = Reference(e, api, pairs, segs)
                before = e.index16_view_emit_stats()
                _check(e, ref)
                d = _delta(e.index16_view_emit_stats(), before)
                want = 1
                if "FELICS_TEST_INDEX16_EMIT_CPS" in env:
                    cut = vc.sub_batches([vc.shape_of(v) for _, v in pairs], segs, 3 if rgb else 1, 5)
                    want = sum(1 for c in cut if any(segs[i] for i in c))
                    assert want > 2
                assert d["sub_batches"] == want and d["redone"] == 0, (d, want)
    finally:
        for k in env:
            del os.environ[k]


def test_ready_event(api, mixed_refs):
    """the surfaces hold zeros; a side stream works for a while and then copies the frames in, an event recorded behind it; the call
    gets the event and no host synchronisation.  The result equals the synchronised call's."""
    import torch

    import felics_amd

    ref = mixed_refs[0]
    with felics_amd.Encoder(0) as e:
        surfs = [Surface(s.host, upload=False) for s, _ in ref.pairs]
        late = Reference.__new__(Reference)
        late.pairs, late.segs = [(s, s.host) for s in surfs], ref.segs
        late.views = [s.view(s.host) for s in surfs]
        late.streams, late.indexes, late.need = ref.streams, ref.indexes, ref.need
        finals = [s.dev for s, _ in ref.pairs]
        side = torch.cuda.Stream()

        def producer():
            with torch.cuda.stream(side):
                busy = torch.zeros(1 << 24, dtype=torch.float32, device="cuda")
                for _ in range(200):
                    busy.add_(1.0)
                for f, s in zip(finals, surfs):
                    s.dev.copy_(f, non_blocking=True)
                ev = torch.cuda.Event()
                ev.record(side)
            return ev.cuda_event, (ev, busy)

        _check(e, late, producer=producer)


def test_round_trip_on_the_device(enc, mixed_refs):
    """Encoder.compress_views_device_indexed16 (the two-call pattern inside); its buffers and arrays go straight into
    decompress_views_device_indexed16, into fresh pitched surfaces: every status 0, the samples equal the input"""
    import torch

    for rgb in (0, 1):
        ref = mixed_refs[rgb]
        keep = [i for i, s in enumerate(ref.segs) if s]
        res = enc.compress_views_device_indexed16(ref.views, ref.segs)
        assert all(int(o) % 64 == 0 for o in res.idx_offsets)
        targets, views = [], []
        for i in keep:
            img = ref.pairs[i][1]
            h, w = img.shape[:2]
            c = 3 if rgb else 1
            pitch = (w + 13) * c
            t = torch.full((h + 2, pitch * 2), 0xA5, dtype=torch.uint8, device="cuda")
            views.append((t.data_ptr() + pitch * 2 + 5 * c * 2, w, h, rgb, 1, pitch * 2, c * 2, 2 if rgb else 0))
            targets.append(t)
        torch.cuda.synchronize()
        _, status = enc.decompress_views_device_indexed16(res.streams.data_ptr(), res.offsets[keep], res.lens[keep], res.index.data_ptr(),
                                                          res.idx_offsets[keep], res.idx_lens[keep], views)
        assert (status == 0).all(), status
        for i, t in zip(keep, targets):
            img = ref.pairs[i][1]
            h, w = img.shape[:2]
            got = t.cpu().numpy().view(np.uint16).reshape(h + 2, -1)[1:1 + h]
            got = got[:, 5 * 3:(5 + w) * 3].reshape(h, w, 3) if rgb else got[:, 5:5 + w]
            assert (got == img).all(), i


def test_refusals(enc, api, mixed_refs):
    """every refusal comes before anything is launched: stats()["submissions"] does not move"""
    import torch

    frames = torch.zeros((2, 130, 64), dtype=torch.int16, device="cuda")
    frames8 = torch.zeros((130, 64), dtype=torch.uint8, device="cuda")
    out = torch.zeros(1 << 17, dtype=torch.uint8, device="cuda")
    d_idx = torch.full((1 << 17,), PATTERN, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    views = [(frames[i].data_ptr(), 64, 130, 0, 1, 128, 2, 0) for i in range(2)]
    narrow = (frames8.data_ptr(), 64, 130, 0, 0, 64, 1, 0)
    u64 = C.POINTER(C.c_uint64)

    def call(vs=views, segs=(4096, 8192), at=0, null=(), index=True):
        n = len(vs)
        cv = (api._CView * n)(*[api._cview(v) for v in vs])
        args = dict(views=cv, segs=(C.c_uint32 * n)(*segs), offs=(C.c_uint64 * n)(), lens=(C.c_uint64 * n)(), ioffs=(C.c_uint64 * n)(),
                    ilens=(C.c_uint64 * n)())
        for k in null:
            args[k] = None
        total = C.c_uint64(7)
        return api.lib().felics_compress_views_device_indexed_wide(enc._h, n, args["views"], args["segs"], None, out.data_ptr(), out.numel(),
                                                                   d_idx.data_ptr() + at if index else None, d_idx.numel() - 64, args["offs"],
                                                                   args["lens"], args["ioffs"], args["ilens"], C.byref(total))

    before = enc.stats()["submissions"]
    assert call(vs=[views[0], narrow]) == E_UNSUPPORTED           # an 8-bit view with a segment
    assert call(null=("segs",)) == E_INVALID_ARGUMENT             # no segment array at all
    for seg in (4095, 4097, 2048):
        assert call(segs=(4096, seg)) == E_INVALID_ARGUMENT, seg
    assert call(at=16) == E_INVALID_ARGUMENT                      # d_index + 16
    assert call(index=False) == E_INVALID_ARGUMENT                # a NULL d_index with an index asked for
    for k in ("views", "offs", "lens", "ioffs", "ilens"):
        assert call(null=(k,)) == E_INVALID_ARGUMENT, k
    ticket = enc.submit_batch_device(frames.data_ptr(), 2, 64, 130, 0, 1, out.data_ptr(), out.numel())
    try:
        assert call() == E_INVALID_ARGUMENT                       # an outstanding ticket
    finally:
        enc.wait_batch(ticket)
    assert enc.stats()["submissions"] == before + 1               # the ticket: no refusal launched anything
    assert (d_idx.cpu().numpy() == PATTERN).all()
    assert call() == 0
    assert call(vs=[views[0], narrow], segs=(4096, 0)) == 0       # the 8-bit view takes part without an index
    assert call(segs=(0, 0), index=False) == 0                    # no index asked for: d_index may be NULL


def test_emit_stats(enc, api, mixed_refs):
    """views, indexes, rows (the sum of the directories' n_rows), bytes and sub-batches of one known call; a shorter out_size writes no
    more than that"""
    ref = mixed_refs[1]
    before = enc.index16_view_emit_stats()
    _check(enc, ref)
    d = _delta(enc.index16_view_emit_stats(), before)
    rows = sum(sum(ic.Layout16(x).n_rows()) for x in ref.indexes if x)
    assert rows > 0
    assert (d["views"], d["indexes"], d["rows_written"], d["index_bytes"], d["sub_batches"], d["redone"]) == (9, 7, rows, ref.need, 1, 0), d
    st = api._CIndex16ViewEmitStats(*([7] * 7))
    assert api.lib().felics_get_index_view_wide_emit_stats(enc._h, C.byref(st), 16) == 0
    assert st.views >= 9 and st.indexes >= 7 and (st.rows_written, st.index_bytes, st.sub_batches, st.shapes_max, st.redone) == (7,) * 5
