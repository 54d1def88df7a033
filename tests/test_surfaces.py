"""Surfaces on the GPU (felics_submit_surfaces_device / felics_compress_surfaces_device / felics_wait_batch): n frames of one shape a
fixed stride apart, queued behind a ready event and read where they lie -- gray8 and gray16 with a row pitch, RGB8 and RGB16 of any
strides.  Every frame is a strided numpy view of a host buffer, the library gets the same strides over a device copy of that buffer,
and every stream is compared with the CPU oracle's of the dense copy (never this library's) and decoded back.  Fresh contexts with
FELICS_POISON=1."""
import io
import math
import os

import numpy as np
import pytest
from numpy.lib.stride_tricks import as_strided

pytestmark = pytest.mark.gpu

E_BUFFER_TOO_SMALL = -8
E_INVALID_ARGUMENT = -11
GRAY, RGB, D8, D16 = 0, 1, 0, 1
TYPES = {"gray8": (np.uint8, GRAY), "rgb8": (np.uint8, RGB), "gray16": (np.uint16, GRAY), "rgb16": (np.uint16, RGB)}


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


def _slot(frame_bytes):
    """felics_compress_images_device's slot: the frame and a quarter, 16-byte aligned."""
    return (frame_bytes + frame_bytes // 4 + 64 + 15) & ~15


def _frames(host, base, shape, strides):
    """A strided view of a flat host array: strides in SAMPLES from sample `base`.  (as_strided does not check bounds: Buffer.desc
    does, through the library's own extent.)"""
    size = host.itemsize
    return as_strided(host[base:], shape=shape, strides=tuple(s * size for s in strides), writeable=False)


class Buffer:
    """A flat host array of samples and its copy in device memory.  frames(...) is a strided numpy view of the host side (N x H x W or
    N x H x W x 3, strides in SAMPLES from sample `base`); desc(view) is the library's descriptor of the same bytes on the device
    side, bounds-checked with felics_surfaces_extent as a caller would."""

    def __init__(self, host):
        import torch

        self.host = np.ascontiguousarray(host).reshape(-1)
        self.dev = torch.from_numpy(self.host).cuda()
        torch.cuda.synchronize()
        self.addr = self.host.__array_interface__["data"][0]

    def frames(self, base, shape, strides):
        return _frames(self.host, base, shape, strides)

    def desc(self, v):
        from felics_amd import api

        n, h, w = v.shape[:3]
        color = RGB if v.ndim == 4 else GRAY
        depth = D16 if v.dtype == np.uint16 else D8
        off = v.__array_interface__["data"][0] - self.addr
        view = (self.dev.data_ptr() + off if h * w else 0, w, h, color, depth, v.strides[1], v.strides[2], v.strides[3] if v.ndim == 4 else 0)
        d = (view, v.strides[0], n)
        lo, hi = api.surfaces_extent(d)
        assert off + lo >= 0 and off + hi <= self.host.nbytes, (off, lo, hi, self.host.nbytes)  # the caller's bounds check
        return d


def _streams(out, offs, lens):
    host = out.cpu().numpy()
    return [host[int(o):int(o) + int(n)].tobytes() for o, n in zip(offs, lens)]


def _want(oracle, v):
    return [oracle.compress(np.ascontiguousarray(f)) for f in v]


def _decode_back(got, v):
    import felics_amd

    for g, f in zip(got, v):
        back = felics_amd.decompress_image(io.BytesIO(g))
        assert back.shape == f.shape and (back == f).all(), f.shape


def _run(e, buf, v, oracle, what, cap=None, queued=True, decode=True):
    """One blocking surfaces call on the frames v of buf: streams against the oracle, the stats that must move and those that must not."""
    import torch

    n = v.shape[0]
    slot = _slot(v[0].size * v.itemsize)
    cap = n * slot if cap is None else cap
    out = torch.zeros(cap + 16, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    s0, v0, o0 = e.surface_stats(), e.view_stats(), e.stats()["slot_overflows"]
    offs, lens = e.compress_surfaces_device(buf.desc(v), out.data_ptr(), cap)
    got = _streams(out, offs, lens)
    want = _want(oracle, v)
    for i, (g, w_) in enumerate(zip(got, want)):
        assert g == w_, "%s frame %d shape %s strides %s: %d vs %d bytes" % (what, i, v.shape, v.strides, len(g), len(w_))
    if decode:
        _decode_back(got, v)
    s1 = e.surface_stats()
    assert s1["submissions"] == s0["submissions"] + 1, (what, s0, s1)
    assert e.view_stats() == v0, (what, "felics_view_stats moved")
    if queued:
        assert s1["queued"] == s0["queued"] + 1 and s1["immediate"] == s0["immediate"], (what, s0, s1)
        assert s1["frames_in_place"] == s0["frames_in_place"] + n and s1["frames_gathered"] == s0["frames_gathered"], (what, s0, s1)
        if all(len(w_) <= slot for w_ in want):
            assert s1["bytes_staged"] == s0["bytes_staged"], (what, s0, s1)
            assert [int(o) for o in offs] == [i * slot for i in range(n)], (what, offs)
            assert e.stats()["slot_overflows"] == o0, (what, e.stats())
        else:  # (16-bit noise can outgrow the slot: the slot-overflow remedy, which gathers, is then the documented outcome)
            assert e.stats()["slot_overflows"] > o0 and s1["bytes_staged"] > s0["bytes_staged"], (what, s0, s1)
    return offs, lens, got


def _pitches(w, pixel_bytes):
    """Row padding: none, 1 and 5 pixels, and up to a multiple of 256 bytes (pitches in pixels of `pixel_bytes` bytes)."""
    per = 256 // math.gcd(256, pixel_bytes)
    return [w, w + 1, w + 5, (w + per) // per * per]


SHAPES = [(1, 1), (2, 1), (1, 5), (7, 3), (15, 9), (16, 16), (17, 33), (64, 64), (100, 50), (129, 65)]


@pytest.mark.parametrize("kind", list(TYPES))
def test_parity_sweep(oracle, kind):
    """Windows of one buffer of random samples, y0, x0 > 0, rows `pitch` apart (a window at pitch = w wraps over the row ends: no
    padding at all), 1 and 3 frames, plus a window that ends on the buffer's last sample; RGB also as RGBA, BGR and planar.  All of
    them queued and read in place: nothing staged, felics_view_stats untouched."""
    dtype, color = TYPES[kind]
    rng = np.random.default_rng(101 + len(kind))
    e = _encoder()
    try:
        px = 3 if color == RGB else 1
        size = np.dtype(dtype).itemsize
        total = 1 << 19
        hi = 256 if dtype == np.uint8 else 65536
        buf = Buffer(rng.integers(0, hi, size=total, dtype=dtype))
        for w, h in SHAPES:
            for pitch in _pitches(w, size * px):
                for n in (1, 3):
                    fs = (h + 2) * pitch * px + 7 * px  # frames an odd number of pixels apart: every alignment
                    base = (2 * pitch + 3) * px      # y0 = 2, x0 = 3
                    if color == GRAY:
                        v = buf.frames(base, (n, h, w), (fs, pitch, 1))
                    else:
                        v = buf.frames(base, (n, h, w, 3), (fs, pitch * 3, 3, 1))
                    _run(e, buf, v, oracle, "%s %dx%d pitch %d n %d" % (kind, w, h, pitch, n))
            # the window that ends on the buffer's last sample
            pitch, n = w + 5, 3
            fs = (h + 1) * pitch * px
            last = (n - 1) * fs + (h - 1) * pitch * px + (w - 1) * px + px - 1
            if color == GRAY:
                v = buf.frames(total - 1 - last, (n, h, w), (fs, pitch, 1))
            else:
                v = buf.frames(total - 1 - last, (n, h, w, 3), (fs, pitch * 3, 3, 1))
            assert v[-1].reshape(-1)[-1] == buf.host[-1]
            _run(e, buf, v, oracle, "%s %dx%d last" % (kind, w, h))
            if color == RGB:
                for pitch in (w, w + 5):
                    n = 3
                    rgba = buf.frames(8, (n, h, w, 3), ((h + 1) * pitch * 4 + 4, pitch * 4, 4, 1))  # rgba[..., :3]
                    _run(e, buf, rgba, oracle, "%s %dx%d rgba pitch %d" % (kind, w, h, pitch))
                    bgr = buf.frames(2 + 9, (n, h, w, 3), ((h + 1) * pitch * 3, pitch * 3, 3, -1))  # rgb[..., ::-1]
                    _run(e, buf, bgr, oracle, "%s %dx%d bgr pitch %d" % (kind, w, h, pitch))
                    plane = (h + 1) * pitch
                    planar = buf.frames(5, (n, h, w, 3), (3 * plane + 1, pitch, 1, plane))  # nchw.permute(0, 2, 3, 1)
                    _run(e, buf, planar, oracle, "%s %dx%d planar pitch %d" % (kind, w, h, pitch))
        st = e.stats()
        assert st["failed"] == 0 and st["two_pass"] == 0, st
    finally:
        e.close()


@pytest.mark.parametrize("kind", ["gray8", "gray16"])
def test_frame_strides(oracle, kind):
    """Overlapping windows two rows apart, frame_stride 0 (n identical streams) and a negative frame stride (the frames in reverse)."""
    dtype, _ = TYPES[kind]
    rng = np.random.default_rng(7)
    e = _encoder()
    try:
        pitch, w, h = 150, 129, 65
        buf = Buffer(rng.integers(0, 256 if dtype == np.uint8 else 65536, size=pitch * 120, dtype=dtype))
        over = buf.frames(pitch + 3, (4, h, w), (2 * pitch, pitch, 1))
        _run(e, buf, over, oracle, kind + " overlapping")
        same = buf.frames(pitch + 3, (3, h, w), (0, pitch, 1))
        _, _, got = _run(e, buf, same, oracle, kind + " stride 0")
        assert got[0] == got[1] == got[2]
        fwd = buf.frames(pitch + 3, (3, 17, w), (20 * pitch, pitch, 1))
        rev = buf.frames(pitch + 3 + 40 * pitch, (3, 17, w), (-20 * pitch, pitch, 1))
        _, _, a = _run(e, buf, fwd, oracle, kind + " forward")
        _, _, b = _run(e, buf, rev, oracle, kind + " reversed")
        assert a == b[::-1]
    finally:
        e.close()


@pytest.mark.parametrize("kind", ["gray8", "gray16"])
def test_queue(oracle, kind):
    """Every lane holds a ticket, surfaces and dense batches alternating: one more submission is refused, so is a blocking call; the
    tickets come back in order.  Four rounds with changing content, a 300 x 170 window at pitch 512."""
    import torch

    from felics_amd import api

    dtype, _ = TYPES[kind]
    depth = D16 if dtype == np.uint16 else D8
    rng = np.random.default_rng(11)
    e = _encoder()
    try:
        lanes = e.lane_count()
        assert lanes >= 2
        w, h, pitch, n = 300, 170, 512, 3
        slot = _slot(w * h * np.dtype(dtype).itemsize)
        for round_ in range(4):
            hi = (256 if dtype == np.uint8 else 65536) >> round_
            bufs = [Buffer(rng.integers(0, hi, size=pitch * (n * (h + 3) + 8), dtype=dtype)) for _ in range(lanes)]
            wins = [b.frames(2 * pitch + 5 + k, (n, h, w), ((h + 3) * pitch, pitch, 1)) for k, b in enumerate(bufs)]
            dense = [torch.from_numpy(np.ascontiguousarray(v)).cuda() for v in wins]
            outs = [torch.zeros(n * slot, dtype=torch.uint8, device="cuda") for _ in range(lanes + 1)]
            torch.cuda.synchronize()
            subs = []
            for k in range(lanes):
                if k % 2 == 0:
                    subs.append(e.submit_surfaces_device(bufs[k].desc(wins[k]), outs[k].data_ptr(), n * slot))
                else:
                    subs.append(e.submit_batch_device(dense[k].data_ptr(), n, w, h, GRAY, depth, outs[k].data_ptr(), n * slot))
            try:
                with pytest.raises(api.FelicsError) as ei:
                    e.submit_surfaces_device(bufs[0].desc(wins[0]), outs[lanes].data_ptr(), n * slot)
                assert ei.value.code == E_INVALID_ARGUMENT
                with pytest.raises(api.FelicsError) as ei:
                    e.submit_batch_device(dense[0].data_ptr(), n, w, h, GRAY, depth, outs[lanes].data_ptr(), n * slot)
                assert ei.value.code == E_INVALID_ARGUMENT
                with pytest.raises(api.FelicsError) as ei:
                    e.compress_surfaces_device(bufs[0].desc(wins[0]), outs[lanes].data_ptr(), n * slot)
                assert ei.value.code == E_INVALID_ARGUMENT
                with pytest.raises(api.FelicsError) as ei:
                    e.compress_batch_device(dense[0].data_ptr(), n, w, h, GRAY, depth, outs[lanes].data_ptr(), n * slot)
                assert ei.value.code == E_INVALID_ARGUMENT
            finally:
                res = [e.wait_batch(s) for s in subs]
            for k in range(lanes):
                offs, lens = res[k]
                assert [int(o) for o in offs] == [i * slot for i in range(n)]
                got = _streams(outs[k], offs, lens)
                assert got == _want(oracle, wins[k]), (round_, k)
                if round_ == 0:
                    _decode_back(got, wins[k])
        st = e.surface_stats()
        assert st["queued"] == st["submissions"] == 4 * ((lanes + 1) // 2) and st["bytes_staged"] == 0, st
    finally:
        e.close()


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


def test_ready_event(oracle):
    """The surfaces hold zeros; a producer on a side stream takes tens of milliseconds and writes them last; two submissions (gray8
    pitched, gray16 pitched) are queued behind the event recorded behind it, with no host synchronisation.  The streams must be those
    of the final frames.  (A race test in the one direction that cannot fail falsely; run once.)"""
    import torch

    e = _encoder()
    try:
        rng = np.random.default_rng(59)
        pitch, w, h, n = 640, 600, 300, 2
        finals = [rng.integers(0, 200, size=pitch * (n * h + 4), dtype=np.uint8), rng.integers(0, 4000, size=pitch * (n * h + 4), dtype=np.uint16)]
        surfs = [Buffer(np.zeros_like(f)) for f in finals]
        finals_dev = [torch.from_numpy(f).cuda() for f in finals]
        slots = [_slot(w * h * f.itemsize) for f in finals]
        outs = [torch.zeros(n * s, dtype=torch.uint8, device="cuda") for s in slots]
        descs = [s.desc(s.frames(pitch + 7, (n, h, w), (h * pitch, pitch, 1))) for s in surfs]
        want = [_want(oracle, _frames(f, pitch + 7, (n, h, w), (h * pitch, pitch, 1))) for f in finals]
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        ev, keep = _slow_producer(side, finals_dev, [s.dev for s in surfs])
        subs = [e.submit_surfaces_device(d, o.data_ptr(), n * s, ready_event=ev.cuda_event) for d, o, s in zip(descs, outs, slots)]
        res = [e.wait_batch(s) for s in subs]
        for k in range(2):
            got = _streams(outs[k], *res[k])
            assert got == want[k], "submission %d was encoded from a surface the producer had not finished" % k
        del keep
        st = e.surface_stats()
        assert st["queued"] == 2 and st["bytes_staged"] == 0, st
    finally:
        e.close()


@pytest.mark.parametrize("env", ["FELICS_TEST_TILE_CAP", "FELICS_TEST_LOOKBACK_FAIL", "FELICS_TEST_SCATTER_ORDER", "FELICS_TWO_PASS"])
def test_remedies_with_two_submissions_in_flight(oracle, env):
    """Each remedy of felics_stats forced on a fresh context with two surface submissions in flight (pitched gray8, RGBA read as
    RGB): the counter moves, every stream is right, and a second pair on the context passes as well."""
    import torch

    from felics_amd import synth

    e = _encoder(**{env: "1"})
    try:
        rng = np.random.default_rng(47)
        g8 = Buffer(synth.gray8(900, 500, 1, "S1"))
        c8 = Buffer(np.concatenate([synth.rgb8(300, 220, 2), rng.integers(0, 256, size=(220, 300, 1), dtype=np.uint8)], axis=2))
        wins = [g8.frames(3 * 900 + 5, (3, 140, 700), (150 * 900, 900, 1)), c8.frames(1200 + 8, (2, 100, 250, 3), (105 * 1200, 1200, 4, 1))]
        bufs = [g8, c8]
        want = [_want(oracle, v) for v in wins]
        for again in range(2):
            slots = [_slot(v[0].size) for v in wins]
            outs = [torch.zeros(v.shape[0] * s, dtype=torch.uint8, device="cuda") for v, s in zip(wins, slots)]
            torch.cuda.synchronize()
            subs = [e.submit_surfaces_device(b.desc(v), o.data_ptr(), o.numel()) for b, v, o in zip(bufs, wins, outs)]
            res = [e.wait_batch(s) for s in subs]
            for k in range(2):
                got = _streams(outs[k], *res[k])
                assert got == want[k], (env, again, k)
                if not again:
                    _decode_back(got, wins[k])
        st, ss = e.stats(), e.surface_stats()
        if env == "FELICS_TEST_TILE_CAP":
            assert st["tile_overflows"] >= 1, st
        elif env == "FELICS_TEST_LOOKBACK_FAIL":
            assert st["lookback_fallbacks"] >= 1, st
        elif env == "FELICS_TEST_SCATTER_ORDER":
            assert st["scatter_fallbacks"] >= 1, st
        else:
            assert st["two_pass"] == 1 and ss["immediate"] == 4 and ss["queued"] == 0, (st, ss)
        if env != "FELICS_TWO_PASS":
            assert ss["queued"] >= 2 and ss["bytes_staged"] > 0, ss  # (the redone sub-batches wanted dense frames)
        assert e.view_stats()["bytes_staged"] == 0
    finally:
        e.close()


def _overflow_case(kind):
    """(frames, the stream size the issue's oracle run found, the slot) -- a frame whose stream outgrows its slot between two
    ordinary frames of the same shape (noise: their streams nearly fill their slots, so the three do not fit the slots' room)."""
    from tests.test_mixed_batch16 import _spiky

    if kind == "gray8":
        yy, xx = np.mgrid[0:48, 0:64]
        bad = (((yy + xx) & 1) * 255).astype(np.uint8)
        rng = np.random.default_rng(3)
        calm = [rng.integers(0, 256, size=(48, 64), dtype=np.uint8) for _ in range(2)]
        return [calm[0], bad, calm[1]], 5697, 3904
    bad = _spiky(np.random.default_rng(5), 42, 40, spikes=1)
    rng = np.random.default_rng(4)
    calm = [rng.integers(0, 65536, size=(42, 40), dtype=np.uint16) for _ in range(2)]
    return [calm[0], bad, calm[1]], 8637, 4272


@pytest.mark.parametrize("kind", ["gray8", "gray16"])
def test_slot_overflow_with_two_submissions_in_flight(oracle, kind):
    """A stream that outgrows its slot, in both of two submissions in flight: slot_overflows grows, the streams are placed exactly
    (16-byte aligned, ascending, non-overlapping) and are right; with a d_out that cannot hold them the wait reports the need."""
    import torch

    from felics_amd import api

    frames, size, slot = _overflow_case(kind)
    assert len(oracle.compress(frames[1])) == size and _slot(frames[1].nbytes) == slot
    h, w = frames[0].shape
    pitch = w + 24
    host = np.zeros((3, h + 2, pitch), frames[0].dtype)
    for i, f in enumerate(frames):
        host[i, 1:h + 1, 5:5 + w] = f
    e = _encoder()
    try:
        buf = Buffer(host)
        v = buf.frames(pitch + 5, (3, h, w), ((h + 2) * pitch, pitch, 1))
        want = _want(oracle, v)
        need = sum((len(x) + 15) // 16 * 16 for x in want)
        assert need > 3 * slot
        cap = need
        before = e.stats()["slot_overflows"]
        outs = [torch.zeros(cap, dtype=torch.uint8, device="cuda") for _ in range(2)]
        torch.cuda.synchronize()
        subs = [e.submit_surfaces_device(buf.desc(v), o.data_ptr(), cap) for o in outs]
        res = [e.wait_batch(s) for s in subs]
        for k in range(2):
            offs, lens = res[k]
            assert [int(x) for x in lens] == [len(x) for x in want]
            assert all(int(o) % 16 == 0 for o in offs)
            for i in range(1, 3):
                assert offs[i] >= offs[i - 1] + lens[i - 1]
            got = _streams(outs[k], offs, lens)
            assert got == want, (kind, k)
            _decode_back(got, v)
        assert e.stats()["slot_overflows"] >= before + 2, e.stats()
        assert e.surface_stats()["queued"] == 2
        # d_out holds the slots and not the streams: the wait says what they need
        sub = e.submit_surfaces_device(buf.desc(v), outs[0].data_ptr(), 3 * slot)
        with pytest.raises(api.FelicsError) as ei:
            e.wait_batch(sub)
        assert ei.value.code == E_BUFFER_TOO_SMALL and ("need %d bytes" % need) in str(ei.value)
        assert e.surface_stats()["queued"] == 3
    finally:
        e.close()


def test_long_codes(oracle):
    """A 210 x 200 gray16 window at a pitch of 256 samples with a code of about 2^16 bits: several pack windows."""
    from tests.test_mixed_batch16 import _spiky

    img = _spiky(np.random.default_rng(9), 200, 210, spikes=1)
    host = np.zeros((2, 204, 256), np.uint16)
    host[0, 2:202, 9:219] = img
    host[1, 2:202, 9:219] = img[::-1].copy()
    e = _encoder()
    try:
        buf = Buffer(host)
        v = buf.frames(2 * 256 + 9, (2, 200, 210), (204 * 256, 256, 1))
        _run(e, buf, v, oracle, "long codes")
        assert len(oracle.compress(img)) > (1 << 16) // 8
    finally:
        e.close()


def test_immediate_case(oracle):
    """What cannot be read in place or queued is done at once through the views call's path and handed over at the wait: gray8 with
    pixel_stride 2, bottom-up gray16, width 0, and a d_out too small for the slots (exact placement) or for the streams (the need in
    lens[0], the second attempt succeeds).  Counted in `immediate` and `frames_gathered`, never in felics_view_stats."""
    import torch

    from felics_amd import api

    rng = np.random.default_rng(13)
    e = _encoder()
    try:
        b8 = Buffer(rng.integers(0, 256, size=100 * 80 * 4, dtype=np.uint8))
        b16 = Buffer(rng.integers(0, 65536, size=100 * 80 * 4, dtype=np.uint16))
        s0 = e.surface_stats()
        every_other = b8.frames(7, (3, 33, 17), (80 * 100, 100, 2))
        _run(e, b8, every_other, oracle, "pixel_stride 2", queued=False)
        s1 = e.surface_stats()
        assert s1["immediate"] == s0["immediate"] + 1 and s1["frames_gathered"] == s0["frames_gathered"] + 3, (s0, s1)
        assert s1["bytes_staged"] == s0["bytes_staged"] + 3 * 33 * 17 and s1["queued"] == s0["queued"], (s0, s1)
        bottom_up = b16.frames(40 * 100 + 3, (2, 33, 17), (45 * 100, -100, 1))
        _run(e, b16, bottom_up, oracle, "bottom-up gray16", queued=False)
        s2 = e.surface_stats()
        assert s2["immediate"] == s1["immediate"] + 1 and s2["frames_gathered"] == s1["frames_gathered"] + 2, (s1, s2)
        # width 0: two header-only streams
        out = torch.zeros(256, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        sub = e.submit_surfaces_device(((0, 0, 9, GRAY, D8, 0, 1, 0), 0, 2), out.data_ptr(), 256)
        offs, lens = e.wait_batch(sub)
        got = _streams(out, offs, lens)
        assert got == [oracle.compress(np.zeros((9, 0), np.uint8))] * 2
        s3 = e.surface_stats()
        assert s3["immediate"] == s2["immediate"] + 1 and s3["frames_gathered"] == s2["frames_gathered"], (s2, s3)
        # a pitched window whose d_out cannot hold the slots: immediate, exact placement; 16 bytes less: the need, then success
        win = b8.frames(205, (3, 50, 90), (60 * 100, 100, 1))
        want = _want(oracle, win)
        exact = sum((len(x) + 15) // 16 * 16 for x in want)
        assert exact < 3 * _slot(50 * 90)
        out = torch.zeros(exact, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        sub = e.submit_surfaces_device(b8.desc(win), out.data_ptr(), exact - 16)
        with pytest.raises(api.FelicsError) as ei:
            e.wait_batch(sub)
        assert ei.value.code == E_BUFFER_TOO_SMALL and ("need %d bytes" % exact) in str(ei.value)
        sub = e.submit_surfaces_device(b8.desc(win), out.data_ptr(), exact)
        offs, lens = e.wait_batch(sub)
        assert _streams(out, offs, lens) == want
        s4 = e.surface_stats()
        assert s4["immediate"] == s3["immediate"] + 2 and s4["queued"] == s0["queued"], (s3, s4)
        assert s4["frames_gathered"] == s3["frames_gathered"] and s4["frames_in_place"] == s3["frames_in_place"] + 6, (s3, s4)
        assert e.view_stats() == {"views": 0, "dense": 0, "in_place": 0, "gathered": 0, "bytes_staged": 0}
        # count == 0: nothing to queue (refused), nothing to do (OK)
        with pytest.raises(api.FelicsError) as ei:
            e.submit_surfaces_device(((b8.dev.data_ptr(), 4, 4, GRAY, D8, 4, 1, 0), 16, 0), out.data_ptr(), exact)
        assert ei.value.code == E_INVALID_ARGUMENT
        offs, lens = e.compress_surfaces_device(((b8.dev.data_ptr(), 4, 4, GRAY, D8, 4, 1, 0), 16, 0), out.data_ptr(), exact)
        assert len(offs) == 0 and e.surface_stats() == s4
    finally:
        e.close()


@pytest.mark.parametrize("kind", list(TYPES))
def test_dense_descriptor(oracle, kind):
    """Three dense 300 x 170 frames back to back: the surfaces call takes felics_submit_batch_device's path and gives the streams
    (and the placement) of compress_batch_device; torch tensors go in through surfaces_of_array."""
    import torch

    from felics_amd import synth

    dtype, color = TYPES[kind]
    depth = D16 if dtype == np.uint16 else D8
    make = {"gray8": lambda s: synth.gray8(300, 170, s, "S1"), "rgb8": lambda s: synth.rgb8(300, 170, s),
            "gray16": lambda s: synth.gray16(300, 170, s), "rgb16": lambda s: np.stack([synth.gray16(300, 170, s + c) for c in range(3)], axis=-1)}[kind]
    host = np.ascontiguousarray(np.stack([make(s) for s in range(3)]))
    e = _encoder()
    try:
        frames = torch.from_numpy(host).cuda()
        cap = 3 * _slot(host[0].nbytes)
        out_a = torch.zeros(cap, dtype=torch.uint8, device="cuda")
        out_b = torch.zeros(cap, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        offs_a, lens_a = e.compress_batch_device(frames.data_ptr(), 3, 300, 170, color, depth, out_a.data_ptr(), cap)
        view = (frames.data_ptr(), 300, 170, color, depth) + ((host.strides[1], host.strides[2], host.strides[3]) if color == RGB else (host.strides[1], host.strides[2], 0))
        s0 = e.surface_stats()
        offs_b, lens_b = e.compress_surfaces_device((view, host.strides[0], 3), out_b.data_ptr(), cap)
        assert list(offs_a) == list(offs_b) and list(lens_a) == list(lens_b)
        got = _streams(out_b, offs_b, lens_b)
        assert got == _streams(out_a, offs_a, lens_a)
        assert got == [oracle.compress(f) for f in host]
        s1 = e.surface_stats()
        assert s1["queued"] == s0["queued"] + 1 and s1["frames_in_place"] == s0["frames_in_place"] + 3 and s1["bytes_staged"] == 0, (s0, s1)
        if dtype == np.uint8:  # a torch tensor's slice goes in as it is (surfaces_of_array)
            win = frames[:, 3:160, 5:290] if color == GRAY else frames[:, 3:160, 5:290, :]
            out_c = torch.zeros(cap, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            offs, lens = e.compress_surfaces_device(win, out_c.data_ptr(), cap)
            assert _streams(out_c, offs, lens) == [oracle.compress(np.ascontiguousarray(f[3:160, 5:290])) for f in host]
    finally:
        e.close()
