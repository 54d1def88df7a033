"""k_pack_t's 8-bit instantiations build the codes of two pixels per instruction (felics_amd/csrc/felics_pairs.h) on both of their
branch-free paths: the k path (a tile with more than WORD_PATH_MAX_SLOTS slots in use: both codes of every pixel) and the word path
(the in-range code alone).  Every stream is byte-compared with the CPU oracle; there is no tolerance anywhere.

A thread takes sixteen consecutive pixels, four dwords of two pairs.  The widths put the first-column pixel of a group (j0, coded a
second time on the scalar functions) into the even and the odd half of a pair and into the first and the last pair of a dword, and
make the 16-byte loads unaligned; the contents reach n = 1 (a constant plane), ctx = 255, n = 256 and Rice codes past 32 bits, so
that groups on the general path lie beside fast ones.  Which path a frame is meant to take is asserted from the oracle's own
per-pixel trace, never from the library under test."""
import os

import numpy as np
import pytest

gpu = pytest.mark.gpu  # (the check of the contents against the oracle's trace needs no GPU and runs with the CPU suite)

TILE = 4096                  # pixels of a pack tile
REC = 16                     # slots of a record: a context's run of a tile is rounded up to whole records
WORD_PATH_MAX_SLOTS = 2048   # felics_kernels.hip: a tile with more slots in use takes the k path
CLS_IN, CLS_RAW = 0, 3       # oracle/felics_oracle.c: a pixel in range; the first two samples (stored as they are)

WIDTHS = [16, 17, 18, 19, 31, 33]
ROWS = 48                    # a few rows: enough that a frame of noise 16 pixels wide has more than 2048 slots in use
# (the estimator starts at k = 5, where the longest Rice code of an 8-bit sample has 15 bits: the two 0 / 255 patterns reach ctx = 255 and
# n = 256 but no long code, so `spikes` is there for the codes past 32 bits -- a flat plane whose flicker brings k down to 0, then 255)
CONTENTS = ["noise", "ramp", "constant", "columns", "checkerboard", "spikes"]
TILE_SHAPES = [(64, 64), (241, 17)]  # (W, H): one whole tile; a tile plus one pixel
TILE_CONTENTS = ["noise", "ramp", "noise over spikes"]  # (the last: long codes in a tile on the k path)


def _content(kind, rng, w, h):
    y, x = np.mgrid[0:h, 0:w]
    if kind == "noise":
        return rng.integers(0, 256, size=(h, w)).astype(np.uint8)
    if kind == "ramp":  # a ramp plus one bit of noise: few events, most pixels in range
        return (((x + y) // 2 + rng.integers(0, 2, size=(h, w))) % 256).astype(np.uint8)
    if kind == "constant":
        return np.full((h, w), 77, dtype=np.uint8)
    if kind == "columns":
        return ((x & 1) * 255).astype(np.uint8)
    if kind == "checkerboard":
        return (((x + y) & 1) * 255).astype(np.uint8)
    if kind == "spikes":  # isolated pixels one above a flat plane, every few of them at full scale
        lone = (x + 3 * y) % 5 == 0
        return np.where(lone, np.where((7 * x + y) % 11 == 0, 255, 101), 100).astype(np.uint8)
    if kind == "noise over spikes":
        return np.where(y < h // 2, _content("noise", rng, w, h), _content("spikes", rng, w, h)).astype(np.uint8)
    raise ValueError(kind)


def _tile_slots(tr, npix):
    """Slots in use of every tile: per context, its events rounded up to whole records."""
    event = (tr["cls"] != CLS_IN) & (tr["cls"] != CLS_RAW)
    out = []
    for a in range(0, npix, TILE):
        counts = np.bincount(tr["ctx"][a:a + TILE][event[a:a + TILE]].astype(np.int64))
        out.append(int(((counts + REC - 1) // REC * REC).sum()))
    return out


@pytest.fixture(scope="module")
def enc():
    import felics_amd

    old = os.environ.get("FELICS_POISON")
    os.environ["FELICS_POISON"] = "1"  # (the workspace is overwritten with garbage before every submission; read at creation)
    try:
        e = felics_amd.Encoder(0)
    finally:
        if old is None:
            del os.environ["FELICS_POISON"]
        else:
            os.environ["FELICS_POISON"] = old
    yield e
    e.close()


@pytest.fixture(scope="module")
def cases(oracle):
    """{(kind, w, h): (frame, the oracle's stream, slots in use per tile)}, computed once for the whole file."""
    out = {}
    shapes = [(kind, w, ROWS) for w in WIDTHS for kind in CONTENTS] + [(kind, w, h) for w, h in TILE_SHAPES for kind in TILE_CONTENTS]
    for kind, w, h in shapes:
        f = _content(kind, np.random.default_rng(w * 100 + h), w, h)
        tr = oracle.trace_channel(f.astype(np.int32), w, h, 0)
        out[(kind, w, h)] = (f, oracle.compress(f), _tile_slots(tr, w * h), tr)
    return out


def test_the_contents_reach_what_they_are_for(cases):
    for (kind, w, h), (f, _, slots, tr) in cases.items():
        event = (tr["cls"] != CLS_IN) & (tr["cls"] != CLS_RAW)
        length = 3 + (tr["val"][event].astype(np.int64) >> tr["k"][event]) + tr["k"][event]
        if kind in ("spikes", "noise over spikes"):  # Rice codes of more than 32 bits beside short ones
            assert length.max() > 32 and length.min() <= 8, (kind, w, h, int(length.max()))
        if kind in ("noise", "noise over spikes"):  # the k path, in every tile that holds whole groups below the first row
            assert all(s > WORD_PATH_MAX_SLOTS for s in slots[: max(1, (w * h) // TILE)]), (w, h, slots)
        elif kind == "ramp":  # the word path, with events and pixels in range side by side
            assert 0 < max(slots) <= WORD_PATH_MAX_SLOTS and event.sum() > 16, (w, h, slots)
        elif kind == "constant":  # n = 1: no event at all
            assert max(slots) == 0 and not event.any()
        elif kind == "columns":  # every pixel between its neighbours 0 and 255: ctx = 255, n = 256
            assert tr["ctx"].max() == 255 and (tr["cls"][tr["ctx"] == 255] == CLS_IN).all()
        elif kind == "checkerboard":  # every pixel 255 away from both its neighbours: an event of value 254 in context 0
            assert event.sum() > w * (h - 1) - h and tr["val"][event].max() == 254


def _encode_uniform(enc, frames):
    import torch

    n, (h, w) = len(frames), frames[0].shape
    d_in = torch.from_numpy(np.stack(frames)).cuda()
    cap = n * (2 * w * h + 4096)
    d_out = torch.empty(cap, dtype=torch.uint8, device="cuda")
    offs, lens = enc.compress_batch_device(d_in.data_ptr(), n, w, h, 0, 0, d_out.data_ptr(), cap)
    host = d_out.cpu().numpy()
    return [host[int(o):int(o) + int(l)].tobytes() for o, l in zip(offs, lens)]


def _compare(got, want, what):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        if g != w:
            n = min(len(g), len(w))
            diff = next((j for j in range(n) if g[j] != w[j]), n)
            raise AssertionError("%s, frame %d: differs from the oracle at byte %d (sizes %d vs %d)" % (what, i, diff, len(g), len(w)))


@gpu
@pytest.mark.parametrize("w", WIDTHS)
def test_contents_at_width(enc, cases, w):
    """The contents at one width in one uniform batch (k_pack_t<u8, PlaneOut>)."""
    chosen = [cases[(kind, w, ROWS)] for kind in CONTENTS]
    _compare(_encode_uniform(enc, [c[0] for c in chosen]), [c[1] for c in chosen], "width %d (%s)" % (w, ", ".join(CONTENTS)))
    st = enc.stats()
    assert st["scatter_fallbacks"] == 0 and st["lookback_fallbacks"] == 0 and st["tile_overflows"] == 0, st


@gpu
@pytest.mark.parametrize("w,h", TILE_SHAPES)
def test_whole_tiles(enc, cases, w, h):
    chosen = [cases[(kind, w, h)] for kind in TILE_CONTENTS]
    _compare(_encode_uniform(enc, [c[0] for c in chosen]), [c[1] for c in chosen], "%d x %d (%s)" % (w, h, ", ".join(TILE_CONTENTS)))


@gpu
def test_mixed_shapes_in_one_call(enc, cases):
    """Frames of different shapes in one submission (k_pack_t<u8, MixedOut>): every content, odd and even widths, a whole tile."""
    import torch

    keys = [("noise", 17, ROWS), ("ramp", 18, ROWS), ("checkerboard", 19, ROWS), ("noise", 64, 64), ("constant", 31, ROWS), ("columns", 33, ROWS),
            ("ramp", 241, 17), ("noise", 16, ROWS), ("spikes", 17, ROWS), ("noise over spikes", 64, 64)]
    tensors = [torch.from_numpy(cases[k][0]).cuda() for k in keys]
    cap = sum(2 * t.numel() + 4096 for t in tensors)
    d_out = torch.empty(cap, dtype=torch.uint8, device="cuda")
    offs, lens = enc.compress_images_device([(t.data_ptr(), t.shape[1], t.shape[0], 0, 0) for t in tensors], d_out.data_ptr(), cap)
    host = d_out.cpu().numpy()
    _compare([host[int(o):int(o) + int(l)].tobytes() for o, l in zip(offs, lens)], [cases[k][1] for k in keys], "mixed shapes")


@gpu
def test_pitched_views(enc, cases):
    """Crops of wider surfaces, read where they lie (k_pack_t<u8, PitchedOut>): a group that straddles a row end is put together
    from two loads, its first-column pixel in every position the widths give."""
    import torch

    keys = [("noise", 17, ROWS), ("ramp", 19, ROWS), ("noise", 33, ROWS), ("checkerboard", 18, ROWS), ("ramp", 64, 64), ("noise", 241, 17), ("spikes", 31, ROWS),
            ("noise over spikes", 64, 64)]
    rng = np.random.default_rng(5)
    views = []
    for i, k in enumerate(keys):
        f = cases[k][0]
        h, w = f.shape
        surface = torch.from_numpy(rng.integers(0, 256, size=(h + 3, w + 7 + i)).astype(np.uint8)).cuda()
        surface[2:2 + h, 3 + i:3 + i + w] = torch.from_numpy(f).cuda()
        views.append(surface[2:2 + h, 3 + i:3 + i + w])
    cap = sum(2 * v.numel() + 4096 for v in views)
    d_out = torch.empty(cap, dtype=torch.uint8, device="cuda")
    offs, lens = enc.compress_arrays_device(views, d_out.data_ptr(), cap)
    torch.cuda.synchronize()
    host = d_out.cpu().numpy()
    _compare([host[int(o):int(o) + int(l)].tobytes() for o, l in zip(offs, lens)], [cases[k][1] for k in keys], "pitched views")
