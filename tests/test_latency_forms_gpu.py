"""k_front (8-bit samples) has every interior trip of a wave's quarter in flight before it classifies the first
(profiles/latency_forms.txt), at the edges that code branches on.  A trip is 256 consecutive pixels; it is interior -- its nine loads are
issued ahead -- if it lies in one image row below the first and inside the wave's quarter (1024 pixels, four trips); any other trip
issues no load ahead and takes the general neighbour rule.  Every stream is byte-compared with the CPU oracle; there is no tolerance
anywhere.  The contexts are created under FELICS_POISON=1: the workspace is overwritten with garbage before every submission."""
import os

import numpy as np
import pytest

gpu = pytest.mark.gpu  # (the check of the shapes' geometry needs no GPU and runs with the CPU suite)

TILE, TRIP = 4096, 256


def _encoder(**env):
    """A fresh context; FELICS_POISON and `env` are read when it is created."""
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


@pytest.fixture(scope="module")
def enc():
    e = _encoder()
    yield e
    e.close()


@pytest.fixture(scope="module")
def enc_ballot():
    e = _encoder(FELICS_SCATTER="ballot")
    yield e
    e.close()


def _ramp_noise(rng, w, h, a):
    """A smooth ramp plus uniform noise in [-a, a], modulo 256."""
    ramp = np.add.outer(np.arange(h), np.arange(w)) // 2
    return ((ramp + rng.integers(-a, a + 1, size=(h, w))) % 256).astype(np.uint8)


def _compare(got, want, what):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        if g != w:
            n = min(len(g), len(w))
            diff = next((j for j in range(n) if g[j] != w[j]), n)
            raise AssertionError("%s, frame %d: differs from the oracle at byte %d (sizes %d vs %d)" % (what, i, diff, len(g), len(w)))


# Widths 255 and 257 give no interior trip (every trip crosses a row end), 256 and 512 give interior trips from row 1 on
# (one and two a row); height 1 is the first row alone (the general rule), 2 leaves one interior row, 17 fills a tile and starts a
# ragged one.  31 x 7 and 300 x 3: a plane smaller than a quarter, three waves of the workgroup with nothing.  600 x 4: the last
# quarter holds 352 pixels -- an interior trip and one that crosses a row end and ends the plane inside itself.  512 x 5: the third
# quarter is two interior trips and the fourth is empty (fewer than four trips issued ahead).
FRONT_SHAPES = [(w, h) for w in (255, 256, 257, 512) for h in (1, 2, 17)] + [(31, 7), (300, 3), (600, 4), (512, 5)]


def _interior_trips(w, h):
    n = 0
    for tile in range(0, w * h, TILE):
        for quarter in range(tile, min(tile + TILE, w * h), TILE // 4):
            end = min(quarter + TILE // 4, w * h)
            for r in range(quarter, end, TRIP):
                n += r // w > 0 and r % w + TRIP <= w and r + TRIP <= end
    return n


def test_front_shapes_reach_what_they_are_for():
    assert [_interior_trips(255, h) for h in (1, 2, 17)] == [0, 0, 0] and [_interior_trips(257, h) for h in (1, 2, 17)] == [0, 0, 0]
    assert [_interior_trips(256, h) for h in (1, 2, 17)] == [0, 1, 16] and [_interior_trips(512, h) for h in (1, 2, 17)] == [0, 2, 32]
    assert _interior_trips(31, 7) == 0 and 31 * 7 < TILE // 4 and 300 * 3 < TILE // 4
    assert (600 * 4) % TRIP != 0 and _interior_trips(600, 4) == 4   # rows 1 .. 3: the trip at x = 0 of each, and pixel 2048 = (248, 3)
    assert _interior_trips(512, 5) == 8


@gpu
@pytest.mark.parametrize("w,h", FRONT_SHAPES)
def test_front_trips_both_rank_forms(enc, enc_ballot, oracle, w, h):
    """A quiet and a loud frame of the shape, with ranks from returning adds and -- a context created under FELICS_SCATTER=ballot --
    from ballots: both equal the oracle, neither needed a redo."""
    rng = np.random.default_rng(w * 1000 + h)
    frames = [_ramp_noise(rng, w, h, 1), _ramp_noise(rng, w, h, 40)]
    want = [oracle.compress(f) for f in frames]
    for e, what in ((enc, "adds"), (enc_ballot, "ballots")):
        before = e.stats()["scatter_fallbacks"]
        _compare(e.compress_batch(frames), want, "%s %d x %d" % (what, w, h))
        assert e.stats()["scatter_fallbacks"] == before, what


@gpu
def test_pitched_views_both_rank_forms(enc, enc_ballot, oracle):
    """Crops of wider surfaces, read where they lie (k_front on PitchedGeom: a trip's row and the row above it are a pitch apart)."""
    import torch

    rng = np.random.default_rng(5)
    frames = [_ramp_noise(rng, w, h, 1 + 39 * (i & 1)) for i, (w, h) in enumerate([(256, 17), (512, 5), (600, 4), (257, 17), (300, 3)])]
    want = [oracle.compress(f) for f in frames]
    views = []
    for i, f in enumerate(frames):
        h, w = f.shape
        surface = torch.from_numpy(rng.integers(0, 256, size=(h + 3, w + 7 + i)).astype(np.uint8)).cuda()
        surface[2:2 + h, 3 + i:3 + i + w] = torch.from_numpy(f).cuda()
        views.append(surface[2:2 + h, 3 + i:3 + i + w])
    cap = sum(2 * v.numel() + 4096 for v in views)
    for e, what in ((enc, "adds"), (enc_ballot, "ballots")):
        d_out = torch.empty(cap, dtype=torch.uint8, device="cuda")
        offs, lens = e.compress_arrays_device(views, d_out.data_ptr(), cap)
        torch.cuda.synchronize()
        host = d_out.cpu().numpy()
        _compare([host[int(o):int(o) + int(l)].tobytes() for o, l in zip(offs, lens)], want, "pitched views, " + what)


@gpu
def test_mixed_shapes_in_one_call(enc, oracle):
    """Frames of different shapes in one submission (k_front on PlaneGeom): the grid is the largest plane's, so the smaller planes'
    workgroups past their last tile have no trip at all."""
    import torch

    rng = np.random.default_rng(6)
    frames = [_ramp_noise(rng, w, h, 1 + 39 * (i & 1)) for i, (w, h) in enumerate([(512, 17), (256, 2), (31, 7), (600, 4), (256, 17), (255, 17)])]
    tensors = [torch.from_numpy(f).cuda() for f in frames]
    cap = sum(2 * t.numel() + 4096 for t in tensors)
    d_out = torch.empty(cap, dtype=torch.uint8, device="cuda")
    offs, lens = enc.compress_images_device([(t.data_ptr(), t.shape[1], t.shape[0], 0, 0) for t in tensors], d_out.data_ptr(), cap)
    host = d_out.cpu().numpy()
    _compare([host[int(o):int(o) + int(l)].tobytes() for o, l in zip(offs, lens)], [oracle.compress(f) for f in frames], "mixed shapes")


@gpu
def test_rgb8_keeps_two_trips_in_flight(enc, oracle):
    """One RGB8 image: the Y / Co / Cg kernels (int16 samples), which keep the order they had."""
    rng = np.random.default_rng(11)
    f = np.stack([_ramp_noise(rng, 512, 17, 1), _ramp_noise(rng, 512, 17, 40), rng.integers(0, 256, size=(17, 512)).astype(np.uint8)], axis=-1).copy()
    _compare(enc.compress_batch([f]), [oracle.compress(f)], "rgb8 512 x 17")
