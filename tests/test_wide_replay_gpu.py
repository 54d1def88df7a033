"""The 16-bit front end (felics_wide.hip) at the edges wide_cases.py builds frames for: the event sort, the chain heads and both
replays of the estimator with the hand-over between them.  Every stream is byte-compared with the CPU oracle; what each case
reaches, and that a subtly different replay would change its streams, is proved on the CPU in test_wide_cases_cpu.py.

A case is ONE sub-batch, so that its planes lie in the record buffer in the case's order: felics_compress_batch_device on frames
in device memory (the host call cuts a batch into eight chunks, which would give a frame of these small batches a sub-batch to
itself); `submissions` shows that it was one.  The encoder runs with FELICS_POISON=1, and FELICS_WIDE_LANE (read per sub-batch)
forces the limit: 0, the wave-wide kernel alone; the limits the case is aimed at; and one no chain reaches."""
import contextlib
import os

import numpy as np
import pytest

from tests import wide_cases as wc

pytestmark = pytest.mark.gpu

GRAY, RGB, D16 = 0, 1, 1


@pytest.fixture(scope="module")
def enc():
    import felics_amd

    os.environ["FELICS_POISON"] = "1"  # the workspace is overwritten with 0xA5 before every sub-batch
    e = felics_amd.Encoder(0)
    del os.environ["FELICS_POISON"]
    yield e
    e.close()


@contextlib.contextmanager
def forced_limit(limit):
    old = os.environ.get("FELICS_WIDE_LANE")
    os.environ["FELICS_WIDE_LANE"] = str(limit)
    try:
        yield
    finally:
        if old is None:
            del os.environ["FELICS_WIDE_LANE"]
        else:
            os.environ["FELICS_WIDE_LANE"] = old


_WANT = {}  # the oracle's streams of a case: computed once


def _want(oracle, c):
    if c.name not in _WANT:
        _WANT[c.name] = [oracle.compress(f) for f in c.frames]
    return _WANT[c.name]


def _compare(got, want, what):
    assert len(got) == len(want), what
    for i, (g, w_) in enumerate(zip(got, want)):
        if g != w_:
            n = min(len(g), len(w_))
            diff = next((j for j in range(n) if g[j] != w_[j]), n)
            raise AssertionError("%s frame %d: differs from the oracle at byte %d (sizes %d vs %d)" % (what, i, diff, len(g), len(w_)))


def _streams(out, offs, lens):
    host = out.cpu().numpy()
    return [host[int(o):int(o) + int(n)].tobytes() for o, n in zip(offs, lens)]


def _limits(c):
    return (0,) + tuple(sorted(set(c.limits))) + (wc.NEVER,)


@pytest.mark.parametrize("name", wc.NAMES)
def test_case_under_every_limit(enc, oracle, name):
    import torch

    c = wc.case(name)
    want = _want(oracle, c)
    n, (h, w) = len(c.frames), c.frames[0].shape[:2]
    dev = torch.from_numpy(np.ascontiguousarray(np.stack(c.frames))).cuda()
    slot = (max(len(s) for s in want) + 64 + 15) & ~15  # room for every stream: no slot overflow, no second run
    out = torch.zeros(n * slot, dtype=torch.uint8, device="cuda")
    for limit in _limits(c):
        out.zero_()
        torch.cuda.synchronize()
        before = enc.stats()
        with forced_limit(limit):
            offs, lens = enc.compress_batch_device(dev.data_ptr(), n, w, h, RGB if c.frames[0].ndim == 3 else GRAY, D16, out.data_ptr(), n * slot)
        after = enc.stats()
        assert after["submissions"] == before["submissions"] + 1 and after["slot_overflows"] == before["slot_overflows"], (name, limit, before, after)
        _compare(_streams(out, offs, lens), want, "%s, limit %d," % (name, limit))


def _padded_lengths_frame():
    """The `lengths` frame padded to three tiles, beside frames of two."""
    f = wc.case("lengths").frames[0]
    wide = np.empty((2, 4500), np.uint16)
    wide[:, :f.shape[1]] = f
    wide[:, f.shape[1]:] = f[1, -1]  # (equal to both neighbours: no events)
    wide[0, f.shape[1]:] = f[1, -1]
    return wide


def test_mixed_shapes_in_one_sub_batch(oracle):
    """felics_compress_images_device: the dense, single-chain and tile-count frames (two tiles a plane: planes without events, of one
    chain, of 15 000) and a frame of three tiles in ONE mixed sub-batch -- the kernels' per-plane geometry, padded tiles."""
    import torch

    import felics_amd

    imgs = wc.case("dense").frames + wc.case("single").frames + wc.case("tiles").frames + [_padded_lengths_frame()]
    tiles = [-(-im.size // 4096) for im in imgs]
    assert min(tiles) == 2 and max(tiles) == 3 and len({im.shape for im in imgs}) == 4  # one bucket: T_min .. ceil(1.25 T_min)
    ev = wc.events(imgs[-1].astype(np.int32), 4500, 2)
    assert set(wc.CHAIN_LENGTHS) <= set(wc.chains_of(ev)[2].tolist())  # (the padding added no event to a chain)
    want = [oracle.compress(im) for im in imgs]
    dev = [torch.from_numpy(im).cuda() for im in imgs]
    descs = [(t.data_ptr(), im.shape[1], im.shape[0], GRAY, D16) for im, t in zip(imgs, dev)]
    cap = sum((im.nbytes + im.nbytes // 4 + 64 + 15) // 16 * 16 for im in imgs)
    out = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    hand = wc.case("dense").limits[0]
    os.environ["FELICS_POISON"] = "1"
    e = felics_amd.Encoder(0)
    del os.environ["FELICS_POISON"]
    try:
        for limit in (0, 1, hand, wc.NEVER):
            out.zero_()
            torch.cuda.synchronize()
            before = e.stats()["submissions"]
            with forced_limit(limit):
                offs, lens = e.compress_images_device(descs, out.data_ptr(), cap)
            assert e.stats()["submissions"] == before + 1, (limit, e.stats())
            _compare(_streams(out, offs, lens), want, "mixed shapes, limit %d," % limit)
    finally:
        e.close()


@pytest.mark.parametrize("name", ["dense", "tiles"])
def test_pitched_surface_read_in_place(oracle, name):
    """felics_submit_surfaces_device on a gray16 surface with padded rows: the count and emit kernels read the frames where they lie
    (frames_in_place rises by the number of frames), everything behind them is the same sub-batch as the dense call's."""
    import torch

    import felics_amd

    c = wc.case(name)
    want = _want(oracle, c)
    n, (h, w) = len(c.frames), c.frames[0].shape
    pitch, lead = w + 5, 3
    host = np.full(lead + n * h * pitch, 0x1234, np.uint16)
    for i, f in enumerate(c.frames):
        host[lead + i * h * pitch:lead + (i + 1) * h * pitch].reshape(h, pitch)[:, :w] = f
    dev = torch.from_numpy(host).cuda()
    slot = (2 * w * h + 2 * w * h // 4 + 64 + 15) & ~15
    assert max(len(s) for s in want) <= slot  # (no slot overflow: its remedy would gather the frames)
    out = torch.zeros(n * slot, dtype=torch.uint8, device="cuda")
    surfaces = ((dev.data_ptr() + 2 * lead, w, h, GRAY, D16, 2 * pitch, 2, 0), 2 * h * pitch, n)
    os.environ["FELICS_POISON"] = "1"
    e = felics_amd.Encoder(0)
    del os.environ["FELICS_POISON"]
    try:
        for limit in _limits(c):
            out.zero_()
            torch.cuda.synchronize()
            s0 = e.surface_stats()
            with forced_limit(limit):
                offs, lens = e.wait_batch(e.submit_surfaces_device(surfaces, out.data_ptr(), n * slot))
            s1 = e.surface_stats()
            assert s1["frames_in_place"] == s0["frames_in_place"] + n and s1["frames_gathered"] == s0["frames_gathered"], (limit, s0, s1)
            _compare(_streams(out, offs, lens), want, "%s on a pitched surface, limit %d," % (name, limit))
    finally:
        e.close()
