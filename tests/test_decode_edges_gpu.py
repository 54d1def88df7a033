"""The GPU decoders on the corpus of decode_cases.py -- the frames test_decode_cases_cpu.py proves to reach the edges the bit readers,
the code readers and the estimator tables branch on -- in every form: the same-shape call at all four addresses (mod 4) of the
committed placement, the mixed call, views (pitched gray, RGBA), the indexed calls at both segment sizes and all four addresses,
two calls in a row on one context, and corrupt variants between intact streams.  Streams come from the oracle; decoded pixels are
compared with the source frames; every output buffer lies between guard bytes that must stay untouched; Encoder.decode_stats()
says which form the streams took.  Every comparison is exact."""
import contextlib
import os

import numpy as np
import pytest

from tests import decode_cases as dc
from tests import index16_common as ic16

pytestmark = pytest.mark.gpu

GUARD = 256
FILL = 0xA5
FORMS = ("wave", "lane")
SWITCHES = {"wave": {"FELICS_TEST_DECODE_LANES": "0", "FELICS_TEST_DECODE16_LANES": "0"},
            "lane": {"FELICS_TEST_DECODE_LANES": "1", "FELICS_TEST_DECODE16_LANES": "1"}}
STAT_FORMS = ("wave8", "lanes8", "wave16", "lanes16", "host", "undecoded")
SEGMENTS = (4096, 12288)  # the smallest segment the index format takes, and a larger one


@pytest.fixture(scope="module")
def enc():
    import felics_amd

    e = felics_amd.Encoder(0)
    yield e
    e.close()


@contextlib.contextmanager
def _env(**kv):
    """environment variables for the calls inside (the library reads them per call)"""
    old = {k: os.environ.get(k) for k in kv}
    os.environ.update(kv)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


_streams = {}


def _stream(oracle, f):
    """the oracle's stream of a corpus frame: computed once, shared and left unchanged"""
    if f.key not in _streams:
        _streams[f.key] = oracle.compress(f.img)
    return _streams[f.key]


def _device(data):
    import torch

    return torch.from_numpy(np.frombuffer(data, dtype=np.uint8).copy()).cuda()


def _form_of(f, form, whole_waves=False, count=0):
    """the decode_stats field a stream of frame f is counted in under the forced form"""
    d = str(dc.depth_of(f.kind))
    if not f.on_gpu:
        return "host"
    return ("lanes" if form == "lane" and f.lanes and (not whole_waves or count >= 64) else "wave") + d


def _moved(enc, before):
    after = enc.decode_stats()
    return {k: after[k] - before[k] for k in STAT_FORMS + ("streams",)}


def _counts(forms):
    out = dict.fromkeys(STAT_FORMS, 0)
    for k in forms:
        out[k] += 1
    out["streams"] = len(forms)
    return out


def _up16(n):
    return (n + 15) // 16 * 16


def _full_waves(frames, form):
    """`frames`, and for the 16-bit lane form of the mixed and views calls -- which takes whole waves of 64 streams of one shape --
    every group the form takes made up to a multiple of 64 with its own frames again.  -> (items, forms per item)"""
    items = list(frames)
    if form == "lane":
        for g in dc.groups(frames):
            if g[0].lanes and dc.depth_of(g[0].kind) == 16:
                items += [g[i % len(g)] for i in range((-len(g)) % 64)]
    size = {}
    for f in items:
        size[(f.kind, f.shape)] = size.get((f.kind, f.shape), 0) + 1
    return items, [_form_of(f, form, dc.depth_of(f.kind) == 16, size[(f.kind, f.shape)]) for f in items]


# ------------------------------------------------------------------------------------------------------------------------
# the same-shape call
# ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("kind", dc.KINDS)
def test_same_shape_calls_at_every_address(enc, oracle, kind, form):
    """felics_decompress_batch_device per shape of the kind, the streams at the addresses of each of the four rotations: k_decode8 /
    k_decode16 (wave) or the lane kernels (lane; rows below eight samples keep the wave form)."""
    import torch

    frames = dc.of_kind(kind)
    streams = [_stream(oracle, f) for f in frames]
    index = {f.key: i for i, f in enumerate(frames)}
    grps = dc.groups(frames)
    start, at = [], GUARD
    for g in grps:
        start.append(at)
        at += _up16(g[0].img.nbytes * len(g)) + GUARD
    want = np.full(at, FILL, np.uint8)
    for g, s in zip(grps, start):
        want[s:s + g[0].img.nbytes * len(g)] = np.stack([f.img for f in g]).reshape(-1).view(np.uint8)
    for rot in dc.ROTATIONS:
        blob, offs, lens = dc.place(frames, streams, rot)
        assert [o & 3 for o in offs] == [dc.placement(f.case, f.index, rot) for f in frames]
        d_in = _device(blob)
        d_px = torch.full((at,), FILL, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        with _env(**SWITCHES[form]):
            for g, s in zip(grps, start):
                ids = [index[f.key] for f in g]
                before = enc.decode_stats()
                hdr, status = enc.decompress_batch_device(d_in.data_ptr(), [offs[i] for i in ids], [lens[i] for i in ids],
                                                          d_px.data_ptr() + s, g[0].img.nbytes * len(g))
                assert (status == 0).all() and (hdr.width, hdr.height) == (g[0].w, g[0].h), (g[0].key, rot, status)
                assert _moved(enc, before) == _counts([_form_of(f, form) for f in g]), (g[0].key, rot)
        host = d_px.cpu().numpy()
        if not (host == want).all():
            for g, s in zip(grps, start):
                for j, f in enumerate(g):
                    a, b = s + j * f.img.nbytes, s + (j + 1) * f.img.nbytes
                    assert (host[a:b] == want[a:b]).all(), ("pixels", f.key, rot, dc.placement(f.case, f.index, rot))
            raise AssertionError("bytes outside the frames written, rotation %d: first at %d" % (rot, int(np.argmax(host != want))))


# ------------------------------------------------------------------------------------------------------------------------
# the mixed call
# ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("depth", (8, 16))
def test_mixed_call(enc, oracle, depth, form):
    """felics_decompress_images_device on all frames of a depth, gray and RGB, in one call: DecMixed (wave), LaneMixed (lane)."""
    import torch

    frames = [f for f in dc.corpus() if dc.depth_of(f.kind) == depth]
    rot = 1 if form == "wave" else 3
    blob, offs, lens = dc.place(frames, [_stream(oracle, f) for f in frames], rot)
    index = {f.key: i for i, f in enumerate(frames)}
    items, forms = _full_waves(frames, form)
    cap = sum(_up16(f.img.nbytes) for f in items)
    d_in = _device(blob)
    d_px = torch.full((GUARD + cap + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    before = enc.decode_stats()
    with _env(**SWITCHES[form]):
        po, hdrs, status = enc.decompress_images_device(d_in.data_ptr(), [offs[index[f.key]] for f in items], [lens[index[f.key]] for f in items],
                                                        d_px.data_ptr() + GUARD, cap)
    assert _moved(enc, before) == _counts(forms)
    if form == "lane":
        assert sum(k.startswith("lanes") for k in forms) >= 64
    assert (status == 0).all(), [items[i].key for i in np.flatnonzero(status)]
    host = d_px.cpu().numpy()
    assert (host[:GUARD] == FILL).all() and (host[GUARD + cap:] == FILL).all()
    at = 0
    for f, o in zip(items, po):
        assert int(o) == at
        got = host[GUARD + at:GUARD + at + f.img.nbytes].view(f.img.dtype).reshape(f.shape)
        assert (got == f.img).all(), (f.key, dc.placement(f.case, f.index, rot))
        at += _up16(f.img.nbytes)


# ------------------------------------------------------------------------------------------------------------------------
# views
# ------------------------------------------------------------------------------------------------------------------------

class _Surface:
    """what decompress_arrays_device takes: an object with __cuda_array_interface__"""

    def __init__(self, ptr, shape, typestr, strides):
        self.__cuda_array_interface__ = {"shape": shape, "typestr": typestr, "data": (ptr, False), "strides": strides, "version": 3}


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("kind", dc.KINDS)
def test_views(enc, oracle, kind, form):
    """felics_decompress_views_device: gray frames into surfaces with a pitch of W + 1 samples (DecPitched, LanePitched), colour
    frames into RGBA (ConvStrided).  The whole surface is compared, the pattern bytes between the samples included."""
    import torch

    frames = dc.of_kind(kind)
    rot = 2 if form == "wave" else 0
    blob, offs, lens = dc.place(frames, [_stream(oracle, f) for f in frames], rot)
    index = {f.key: i for i, f in enumerate(frames)}
    items, forms = _full_waves(frames, form)
    size = 2 if kind.endswith("16") else 1
    dt = np.dtype("<u2") if size == 2 else np.dtype("u1")
    rgb = kind.startswith("rgb")
    where, at = [], GUARD
    for f in items:
        where.append(at)
        at += _up16(f.h * f.w * 4 * size if rgb else f.h * (f.w + 1) * size) + 16
    at += GUARD
    pattern = ((np.arange(at, dtype=np.uint64) * 37 + 11) & 0xFF).astype(np.uint8)
    want = pattern.copy()
    d_px = torch.from_numpy(pattern).cuda()
    arrays = []
    for f, o in zip(items, where):
        shape = (f.h, f.w, 3) if rgb else (f.h, f.w)
        strides = (f.w * 4 * size, 4 * size, size) if rgb else ((f.w + 1) * size, size)
        np.ndarray(shape, dt, want, o, strides)[...] = f.img
        arrays.append(_Surface(d_px.data_ptr() + o, shape, "<u2" if size == 2 else "|u1", strides))
    d_in = _device(blob)
    torch.cuda.synchronize()
    before = enc.decode_stats()
    with _env(**SWITCHES[form]):
        hdrs, status = enc.decompress_arrays_device(d_in.data_ptr(), [offs[index[f.key]] for f in items], [lens[index[f.key]] for f in items], arrays)
    assert _moved(enc, before) == _counts(forms)
    assert (status == 0).all(), [items[i].key for i in np.flatnonzero(status)]
    host = d_px.cpu().numpy()
    if not (host == want).all():
        bad = int(np.argmax(host != want))
        j = int(np.searchsorted(where, bad, side="right")) - 1
        raise AssertionError("surface byte %d differs: frame %s, byte %d of its surface" % (bad, items[max(j, 0)].key, bad - where[max(j, 0)]))


# ------------------------------------------------------------------------------------------------------------------------
# the indexed calls
# ------------------------------------------------------------------------------------------------------------------------

def _indexed_groups(kind):
    """the shapes of the kind the indexed walks take (a GPU form's rows)"""
    return dc.groups([f for f in dc.of_kind(kind) if f.on_gpu])


@pytest.mark.parametrize("lanes", (0, 1))
@pytest.mark.parametrize("kind", dc.KINDS[:2])
def test_indexed_calls_8(enc, oracle, kind, lanes):
    """felics_decompress_batch_device_indexed per shape, indexes built on the host at both segment sizes, the streams at the addresses
    of all four rotations: the checkpoint walk reads the stream through init_at (grid s).  lanes = 1: groups with rows of eight
    samples and more are made up to 64 streams with their own frames again and take the lane form."""
    import torch

    from felics_amd import api

    frames = dc.of_kind(kind)
    streams = [_stream(oracle, f) for f in frames]
    index = {f.key: i for i, f in enumerate(frames)}
    placed = [dc.place(frames, streams, rot) for rot in dc.ROTATIONS]
    d_ins = [_device(p[0]) for p in placed]
    planes = 3 if kind.startswith("rgb") else 1
    with _env(FELICS_TEST_INDEX_LANES=str(lanes)):
        for g in _indexed_groups(kind):
            by_lane = bool(lanes) and g[0].lanes
            items = g + ([g[i % len(g)] for i in range((-len(g)) % 64)] if by_lane else [])
            ids = [index[f.key] for f in items]
            per, n = g[0].img.nbytes, len(items)
            want = np.full(GUARD + per * n + GUARD, FILL, np.uint8)
            want[GUARD:GUARD + per * n] = np.stack([f.img for f in items]).reshape(-1)
            for seg in SEGMENTS:
                built = {f.key: api.index_build(_stream(oracle, f), seg) for f in g}
                stride = max(_up16(len(built[g[0].key])), 64)
                iblob = b"".join(built[f.key] + bytes(stride - len(built[f.key])) for f in items)
                d_idx = _device(iblob)
                k = (g[0].w * g[0].h + seg - 1) // seg
                for rot, (_, offs, lens) in zip(dc.ROTATIONS, placed):
                    d_px = torch.full((len(want),), FILL, dtype=torch.uint8, device="cuda")
                    torch.cuda.synchronize()
                    before = enc.decode_stats()
                    _, status = enc.decompress_batch_device_indexed(d_ins[rot].data_ptr(), [offs[i] for i in ids], [lens[i] for i in ids],
                                                                    d_idx.data_ptr(), stride, d_px.data_ptr() + GUARD, per * n)
                    after = enc.decode_stats()
                    assert (status == 0).all(), (g[0].key, seg, rot, status)
                    in_lanes = n // 64 * 64 * planes * k if by_lane else 0
                    assert after["lane_segments8"] - before["lane_segments8"] == in_lanes, (g[0].key, seg, rot)
                    assert after["segments8"] - before["segments8"] == n * planes * k - in_lanes, (g[0].key, seg, rot)
                    host = d_px.cpu().numpy()
                    assert (host == want).all(), (g[0].key, seg, rot, int(np.argmax(host != want)) - GUARD)


@pytest.mark.parametrize("kind", dc.KINDS[2:])
def test_indexed_calls_16(enc, oracle, kind):
    """felics_decompress_batch_device_indexed_wide per shape, version-2 indexes built on the host at both segment sizes, the streams at
    the addresses of all four rotations."""
    import torch

    from felics_amd import api

    frames = dc.of_kind(kind)
    streams = [_stream(oracle, f) for f in frames]
    index = {f.key: i for i, f in enumerate(frames)}
    placed = [dc.place(frames, streams, rot) for rot in dc.ROTATIONS]
    d_ins = [_device(p[0]) for p in placed]
    planes = 3 if kind.startswith("rgb") else 1
    for g in _indexed_groups(kind):
        ids = [index[f.key] for f in g]
        per, n = g[0].img.nbytes, len(g)
        want = np.full(GUARD + per * n + GUARD, FILL, np.uint8)
        want[GUARD:GUARD + per * n] = np.stack([f.img for f in g]).reshape(-1).view(np.uint8)
        for seg in SEGMENTS:
            iblob, ioffs, ilens = ic16.pack([api.index16_build(_stream(oracle, f), seg) for f in g], 64)
            d_idx = _device(iblob)
            k = (g[0].w * g[0].h + seg - 1) // seg
            for rot, (_, offs, lens) in zip(dc.ROTATIONS, placed):
                d_px = torch.full((len(want),), FILL, dtype=torch.uint8, device="cuda")
                torch.cuda.synchronize()
                before = enc.index16_stats()
                _, status = enc.decompress_batch_device_indexed16(d_ins[rot].data_ptr(), [offs[i] for i in ids], [lens[i] for i in ids],
                                                                  d_idx.data_ptr(), ioffs, ilens, d_px.data_ptr() + GUARD, per * n)
                after = enc.index16_stats()
                assert (status == 0).all(), (g[0].key, seg, rot, status)
                assert after["segments16"] - before["segments16"] == n * planes * k, (g[0].key, seg, rot)
                host = d_px.cpu().numpy()
                assert (host == want).all(), (g[0].key, seg, rot, int(np.argmax(host != want)) - GUARD)


# ------------------------------------------------------------------------------------------------------------------------
# consecutive calls
# ------------------------------------------------------------------------------------------------------------------------

def _pair(kind):
    """two frames of one shape, the first leaving contexts trained that the second uses (from the model)"""
    for g in dc.groups([f for f in dc.of_kind(kind) if f.lanes]):
        for a in g:
            for b in g:
                if a is not b and not (a.img == b.img).all() and dc.shared_trained_contexts(a, b):
                    return a, b
    raise AssertionError("no pair of " + kind)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("kind", dc.KINDS[2:])
def test_two_calls_in_a_row(enc, oracle, kind, form):
    """Two 16-bit calls in a row on one context, one stream each: the second call's stream gets the table the first one's had, with
    contexts in it that the first frame trained to a k other than 14 and the second frame uses.  A row of the earlier call taken for
    this call's would give those events another k."""
    import torch

    a, b = _pair(kind)
    shared = dc.shared_trained_contexts(a, b)
    assert shared and all(a.model()[0]["final"][c] != 14 for c in shared)
    first_k = {int(c): int(k) for c, k in zip(b.events(0)[1][::-1], b.events(0)[3][::-1])}  # the k of each context's first event
    assert all(first_k[c] == 14 for c in shared)
    with _env(**SWITCHES[form]):
        for n, f in enumerate((a, b, a)):
            blob, offs, lens = dc.place([f], [_stream(oracle, f)], n)
            d_in = _device(blob)
            d_px = torch.full((GUARD + f.img.nbytes + GUARD,), FILL, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            before = enc.decode_stats()
            _, status = enc.decompress_batch_device(d_in.data_ptr(), offs, lens, d_px.data_ptr() + GUARD, f.img.nbytes)
            assert (status == 0).all() and _moved(enc, before) == _counts([_form_of(f, form)])
            host = d_px.cpu().numpy()
            assert (host[:GUARD] == FILL).all() and (host[GUARD + f.img.nbytes:] == FILL).all()
            assert (host[GUARD:GUARD + f.img.nbytes].view(np.uint16).reshape(f.shape) == f.img).all(), (f.key, n)


# ------------------------------------------------------------------------------------------------------------------------
# corrupt variants
# ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("kind", dc.KINDS)
def test_corrupt_variants_between_intact_streams(enc, oracle, kind, form):
    """The variants of decode_cases.variants() -- cut by a byte, cut in the longest run, cut on a chunk boundary of each grid, the
    hand-assembled tails -- each with the intact stream in front of it and behind it, in one same-shape call: a status other than 0
    exactly where the oracle rejects, the oracle's pixels where both accept, the host decoder's code (-2 or -3) for the tails, the
    intact streams decoded exactly, the guard bytes untouched."""
    import felics_amd
    import torch
    from felics_amd import api

    (f,) = dc.variant_frames(kind)
    assert f.lanes
    good = _stream(oracle, f)
    rot = dc.KINDS.index(kind)
    vs = dc.variants(f, good, dc.placement(f.case, f.index, rot))
    names = [None] + [x for name, _ in vs for x in (name, None)]
    streams = [good] + [x for _, v in vs for x in (v, good)]
    blob, offs, lens = dc.place([f] * len(streams), streams, rot)
    per = f.img.nbytes
    d_in = _device(blob)
    d_px = torch.full((GUARD + per * len(streams) + GUARD,), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    before = enc.decode_stats()
    with _env(**SWITCHES[form]), pytest.raises(felics_amd.DecompressionError) as ei:
        enc.decompress_batch_device(d_in.data_ptr(), offs, lens, d_px.data_ptr() + GUARD, per * len(streams))
    status = ei.value.status
    assert _moved(enc, before) == _counts([_form_of(f, form)] * len(streams))
    host = d_px.cpu().numpy()
    assert (host[:GUARD] == FILL).all() and (host[GUARD + per * len(streams):] == FILL).all()
    for i, (name, s) in enumerate(zip(names, streams)):
        got = host[GUARD + i * per:GUARD + (i + 1) * per].view(f.img.dtype).reshape(f.shape)
        if name is None:
            assert status[i] == 0 and (got == f.img).all(), (i, names[i - 1] if i else None)
            continue
        try:
            want = oracle.decompress(s)
        except Exception:
            want = None
        assert (status[i] != 0) == (want is None), (name, status[i])
        if want is not None:
            assert (got == want).all(), name
        if name.startswith("tail"):
            with pytest.raises(felics_amd.DecompressionError) as host_error:
                api.decompress_bytes(s)
            assert host_error.value.code in (-2, -3) and status[i] == host_error.value.code, (name, status[i], host_error.value.code)
