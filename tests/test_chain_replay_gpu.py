"""The 8-bit chain stage (felics_chain.hip: k_enum, k_spine3, k_assign3) at the edges chain_cases.py builds frames for.  Every stream
is byte-compared with the CPU oracle; what each case reaches, and that a subtly different replay would change its streams, is
proved on the CPU in test_chain_cases_cpu.py.

A case is ONE sub-batch (felics_compress_batch_device and felics_submit_batch_device on frames in device memory), so that its planes
lie in the order the case gives them.  One Encoder per environment for the cases whose tiles fit the default slots, with
FELICS_POISON=1, and a fresh one for each case whose tile outgrows them (a context that has met an overflow sizes its tiles for the
worst case from then on, so only a fresh one shows the next: gray8 at 6160 slots and Co at 8208 each in its own).  After every
case the context's counters must say what the trace model predicts: one tile overflow exactly there, no other remedy anywhere."""
import contextlib
import os

import numpy as np
import pytest

from tests import chain_cases as cc

pytestmark = pytest.mark.gpu

GRAY, RGB, D8 = 0, 1, 0


@contextlib.contextmanager
def encoder(**env):
    """A context created under `env` and FELICS_POISON=1 (the workspace is overwritten with 0xA5 before every sub-batch); the
    environment is as it was before the context is used."""
    import felics_amd

    env = dict(env, FELICS_POISON="1")
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        e = felics_amd.Encoder(0)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v
    try:
        yield e
    finally:
        e.close()


def each_case(names=cc.NAMES, **env):
    """(context, case) of every named case: one context created under `env` for the cases whose tiles fit, then a fresh one for each
    case whose tile overflows."""
    with encoder(**env) as e:
        for n in names:
            if n not in cc.OVERFLOWING:
                yield e, cc.case(n)
    for n in names:
        if n in cc.OVERFLOWING:
            with encoder(**env) as e:
                yield e, cc.case(n)


_WANT = {}  # the oracle's streams of a case: computed once


def _want(oracle, c):
    if c.name not in _WANT:
        _WANT[c.name] = [oracle.compress(f) for f in c.frames]
    return _WANT[c.name]


def _where(c, frame, byte):
    """The pixel whose code holds byte `byte` of the frame's stream, from the oracle's code lengths (the planes' bits follow the 14
    header bytes back to back), and the event it is."""
    bit = 8 * (byte - 14)
    per = 3 if c.rgb else 1
    for p in range(per):
        ev = c.trace()[frame * per + p]
        ends = np.cumsum(ev["nbits"])
        if bit < ends[-1]:
            pixel = int(np.searchsorted(ends, bit, side="right"))
            at = int(np.searchsorted(ev["pix"], pixel))  # the first event at or behind the pixel
            if at == len(ev["pix"]):
                return "plane %d, pixel %d (tile %d), behind the plane's last event" % (p, pixel, pixel // cc.TILE)
            ctx = int(ev["ctx"][at])
            in_chain = int((ev["ctx"][:at] == ctx).sum())
            return "plane %d, pixel %d (tile %d); event %d of the plane at pixel %d: context %d, event %d of its chain (record %d of its run)" % (
                p, pixel, pixel // cc.TILE, at, int(ev["pix"][at]), ctx, in_chain,
                int(((ev["ctx"][:at] == ctx) & (ev["pix"][:at] // cc.TILE == ev["pix"][at] // cc.TILE)).sum()) // cc.REC)
        bit -= int(ends[-1])
    return "behind the last plane"


def _compare(c, got, want, what):
    assert len(got) == len(want), (c.name, what)
    for i, (g, w_) in enumerate(zip(got, want)):
        if g != w_:
            n = min(len(g), len(w_))
            diff = next((j for j in range(n) if g[j] != w_[j]), n)
            raise AssertionError("%s, %s, frame %d: differs from the oracle at byte %d (sizes %d vs %d): %s"
                                 % (c.name, what, i, diff, len(g), len(w_), _where(c, i, diff) if diff >= 14 else "the header"))


def _streams(out, offs, lens):
    host = out.cpu().numpy()
    return [host[int(o):int(o) + int(n)].tobytes() for o, n in zip(offs, lens)]


class Batch:
    """A case's frames in device memory and an output buffer whose slots hold every stream (no slot overflow) and are large enough for
    the fixed-slot path (a quarter of a frame at least)."""

    def __init__(self, oracle, c):
        import torch

        self.c, self.want = c, _want(oracle, c)
        self.n, (self.h, self.w) = len(c.frames), c.frames[0].shape[:2]
        self.dev = torch.from_numpy(np.ascontiguousarray(np.stack(c.frames))).cuda()
        self.slot = (max(max(len(s) for s in self.want) + 64, c.frames[0].nbytes // 2) + 15) & ~15
        self.outs = [torch.zeros(self.n * self.slot, dtype=torch.uint8, device="cuda") for _ in range(2)]
        torch.cuda.synchronize()

    def args(self, i=0):
        return (self.dev.data_ptr(), self.n, self.w, self.h, RGB if self.c.rgb else GRAY, D8, self.outs[i].data_ptr(), self.n * self.slot)


def _check_stats(e, c, what):
    """tile_overflows: exactly one in the fresh context of a case whose tile outgrows the default slots, none in the others; nothing else"""
    st = e.stats()
    assert c.overflows == (c.name in cc.OVERFLOWING)
    assert st["tile_overflows"] == (1 if c.overflows else 0), (c.name, what, st)
    assert st["scatter_fallbacks"] == st["lookback_fallbacks"] == st["slot_overflows"] == st["ticket_retries"] == 0 and not st["failed"], (c.name, what, st)


@pytest.mark.parametrize("ns", cc.SLICE_COUNTS)
def test_blocking_call_with_the_cases_slice_counts(oracle, ns):
    """felics_compress_batch_device under FELICS_SLICES = ns, every case that names ns."""
    names = [n for n in cc.NAMES if ns in cc.case(n).slices]
    assert names
    for e, c in each_case(names, FELICS_SLICES=str(ns)):
        b = Batch(oracle, c)
        before = e.stats()["submissions"]
        offs, lens = e.compress_batch_device(*b.args())
        assert e.stats()["submissions"] == before + (2 if c.overflows else 1), (c.name, ns, e.stats())  # one sub-batch, and once more behind an overflow
        _compare(c, _streams(b.outs[0], offs, lens), b.want, "%d slices" % ns)
        _check_stats(e, c, "%d slices" % ns)


@pytest.mark.parametrize("ns", [1, 2, 5])
def test_queued_submissions(oracle, ns):
    """felics_submit_batch_device under FELICS_SLICES_QUEUED = ns: two submissions of every case in flight (one where the case's tile
    overflows: each of two would count its own)."""
    for e, c in each_case(FELICS_SLICES_QUEUED=str(ns)):
        b = Batch(oracle, c)
        tickets = [e.submit_batch_device(*b.args(i)) for i in range(1 if c.overflows else 2)]
        for i, t in enumerate(tickets):
            offs, lens = e.wait_batch(t)
            _compare(c, _streams(b.outs[i], offs, lens), b.want, "queued, %d slices, submission %d" % (ns, i))
        _check_stats(e, c, "queued, %d slices" % ns)


def test_two_pass_pack(oracle):
    """FELICS_TWO_PASS=1: the other consumer of the records' k, k_k_to_pixels_tl, over all cases."""
    for e, c in each_case(FELICS_TWO_PASS="1"):
        b = Batch(oracle, c)
        offs, lens = e.compress_batch_device(*b.args())
        _compare(c, _streams(b.outs[0], offs, lens), b.want, "two-pass")
        _check_stats(e, c, "two-pass")
        assert e.stats()["two_pass"] == 1


def _partner(c, rng):
    """An image of more tiles than the case's frames, within the same bucket of a mixed call (ceil(1.25 T) tiles): noise, two rows."""
    tiles = (5 * c.tiles() + 3) // 4
    assert tiles > c.tiles()
    shape = (2, tiles * cc.TILE // 2) + ((3,) if c.rgb else ())
    return rng.integers(0, 256, size=shape, dtype=np.uint8)


def test_mixed_shapes_with_a_larger_partner(oracle):
    """felics_compress_images_device: every case beside one image of more tiles, one mixed sub-batch -- the case's planes then end
    with empty tiles under the mixed geometry table."""
    import torch

    rng = np.random.default_rng(97)
    for e, c in each_case():
        imgs = c.frames + [_partner(c, rng)]
        want = _want(oracle, c) + [oracle.compress(imgs[-1])]
        dev = [torch.from_numpy(im).cuda() for im in imgs]
        descs = [(t.data_ptr(), im.shape[1], im.shape[0], RGB if c.rgb else GRAY, D8) for im, t in zip(imgs, dev)]
        cap = sum(im.nbytes * 2 + 4096 for im in imgs)
        out = torch.zeros(cap, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        before = e.stats()["submissions"]
        offs, lens = e.compress_images_device(descs, out.data_ptr(), cap)
        if c.overflows:  # (behind the mixed sub-batch that overflowed: the sub-batches of the remedy)
            assert e.stats()["submissions"] >= before + 2, (c.name, e.stats())
        else:
            assert e.stats()["submissions"] == before + 1, (c.name, e.stats())  # one bucket, one sub-batch
        got = _streams(out, offs, lens)
        assert got[-1] == want[-1], (c.name, "the partner")
        _compare(c, got[:-1], want[:-1], "mixed shapes")
        _check_stats(e, c, "mixed shapes")


def test_views_as_crops_of_a_pitched_surface(oracle):
    """felics_compress_views_device: every case's frames as crops of one pitched surface (rows 37 pixels longer than the frames, the
    crops from pixel 5 of theirs)."""
    import torch

    for e, c in each_case():
        n, (h, w) = len(c.frames), c.frames[0].shape[:2]
        px = 3 if c.rgb else 1
        surface = np.full((n * h + 1, (w + 37) * px), 0x5A, np.uint8)
        for i, f in enumerate(c.frames):
            surface[i * h:(i + 1) * h, 5 * px:(5 + w) * px] = f.reshape(h, w * px)
        dev = torch.from_numpy(surface).cuda()
        pitch = surface.shape[1]
        views = [(dev.data_ptr() + i * h * pitch + 5 * px, w, h, RGB if c.rgb else GRAY, D8, pitch, px, 1 if c.rgb else 0) for i in range(n)]
        cap = sum(f.nbytes * 2 + 4096 for f in c.frames)
        out = torch.zeros(cap, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        offs, lens = e.compress_views_device(views, out.data_ptr(), cap)
        _compare(c, _streams(out, offs, lens), _want(oracle, c), "views")
        _check_stats(e, c, "views")


def test_enum_chunk(oracle):
    """The 16.8 MPix frame whose 4100 tiles are one slice (FELICS_SLICES=1), encoded once: k_enum's second chunk of 4096 tiles."""
    c = cc.case("enum_chunk")
    b = Batch(oracle, c)
    with encoder(FELICS_SLICES="1") as e:
        offs, lens = e.compress_batch_device(*b.args())
        assert e.stats()["submissions"] == 1, e.stats()
        _compare(c, _streams(b.outs[0], offs, lens), b.want, "one slice")
        _check_stats(e, c, "one slice")
