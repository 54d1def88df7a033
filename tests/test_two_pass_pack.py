"""The two-pass pack (k_lengths, k_bitscan_slice, k_finish_sizes, k_zero_edges or k_place_streams + k_zero_streams, k_pack, their
_mixed and _pitched forms; LaneBits and put_pixel) at its word, window, slot and plane edges.

Every stream is byte-compared with the CPU oracle.  The frames are the cases of tests/pack_layout.py: what each of them reaches -- a
window boundary between two codes, inside a short code, inside a run, between two threads' groups; a run that begins in a window's
last word, ends in a window's first, covers a window; a tile inside a word it shares with both neighbours; every position of a tile's
or a plane's first bit; the word a slot is cut at -- is worked out from the oracle's per-pixel code lengths alone and asserted here
through that helper and, case by case, in tests/test_pack_layout_cpu.py.  Shapes are one to three tiles of 4096 pixels.

All 16-bit streams take this path: same shape (the host and the device entry point; fixed slots, exact placement, the slot cut and
its redo), mixed shapes (felics_compress_images*), gray16 surfaces read at their pitch (felics_compress_surfaces_device) and gray16
views (felics_compress_views_device, which gathers them into a mixed sub-batch).  8-bit streams take it on the remedy path: a
context created with FELICS_TWO_PASS=1.  Contexts run with FELICS_POISON=1: the workspace is garbage before every submission.

Not tested: k_bitscan_slice scans the low and high 16 bits of the tile totals apart, which matters only when 64 consecutive tiles
sum to 2^32 bits or more; no content sustains 2^26 bits a tile, because the estimator raises k after the first long code of a
context.  Planes of more than 1024 tiles (the scan's second trip) are test_gpu_parity.test_sixteen_bit_4k's."""
import os

import numpy as np
import pytest

from tests import pack_layout as pl

pytestmark = pytest.mark.gpu

GRAY, RGB, D8, D16 = 0, 1, 0, 1
GUARD, PATTERN = 4096, 0xC3  # bytes behind the capacity passed to a device call, and what they are filled with


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


@pytest.fixture(scope="module")
def enc():
    e = _encoder()
    yield e
    e.close()


@pytest.fixture(scope="module")
def enc8():
    """The 8-bit remedy path: lengths, bit scan and pack kernels behind the chain stage, as after two look-back failures."""
    e = _encoder(FELICS_TWO_PASS="1")
    yield e
    assert e.stats()["two_pass"] == 1
    e.close()


_WANT = {}  # the oracle's stream of a frame, computed once


def _want(oracle, f):
    key = (f.shape, f.dtype.str, f.tobytes())
    if key not in _WANT:
        _WANT[key] = oracle.compress(f)
    return _WANT[key]


def _compare(what, got, frames, oracle):
    assert len(got) == len(frames), what
    for i, (g, f) in enumerate(zip(got, frames)):
        want = _want(oracle, f)
        if g != want:
            n = min(len(g), len(want))
            diff = next((j for j in range(n) if g[j] != want[j]), n)
            raise AssertionError("%s frame %d of shape %s %s: differs from the oracle at byte %d (sizes %d vs %d)" % (what, i, f.shape, f.dtype, diff, len(g), len(want)))


def _reach(name):
    """The case, with its reach asserted from the oracle (cached: the layouts are worked out once a session)."""
    c = pl.case(name)
    if not getattr(c, "_reach_ok", False):
        got = c.reached()
        assert got == c.edges, (name, sorted(c.edges ^ got))
        c._reach_ok = True
    return c


def _round16(n):
    return (int(n) + 15) // 16 * 16


def _guarded(cap):
    import torch

    out = torch.full((cap + GUARD,), PATTERN, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    return out


def _check_guard(what, host, cap):
    touched = np.flatnonzero(host[cap:] != PATTERN)
    assert len(touched) == 0, "%s: byte %d behind the capacity of %d was written (%d bytes in all)" % (what, int(touched[0]), cap, len(touched))


def _back_to_back(what, offs, lens):
    offs, lens = [int(o) for o in offs], [int(n) for n in lens]
    assert offs[0] == 0 and all(o % 16 == 0 for o in offs), (what, offs)
    assert all(offs[i] == offs[i - 1] + _round16(lens[i - 1]) for i in range(1, len(offs))), (what, offs, lens)


def _device(e, oracle, what, frames, cap=None, slot=0):
    """felics_compress_batch_device on same-shaped frames into a buffer full of a pattern, with guard bytes behind `cap` (default:
    exactly what the streams need placed back to back, which the fixed slots do not fit in: exact placement).  slot: the streams
    are expected at multiples of it, not back to back.  Returns (offsets, lens)."""
    import torch

    want = [_want(oracle, f) for f in frames]
    need = sum(_round16(len(x)) for x in want)
    cap = need if cap is None else cap
    h, w = frames[0].shape[:2]
    d_in = torch.from_numpy(np.stack(frames).view(np.uint8)).cuda()
    out = _guarded(cap)
    offs, lens = e.compress_batch_device(d_in.data_ptr(), len(frames), w, h, RGB if frames[0].ndim == 3 else GRAY,
                                         D16 if frames[0].dtype == np.uint16 else D8, out.data_ptr(), cap)
    host = out.cpu().numpy()
    _check_guard(what, host, cap)
    if slot:
        assert [int(o) for o in offs] == [i * slot for i in range(len(frames))], (what, offs)
    else:
        _back_to_back(what, offs, lens)
        assert int(offs[-1]) + _round16(lens[-1]) == need <= cap, (what, offs, lens, cap)
    _compare(what, [host[int(o):int(o) + int(n)].tobytes() for o, n in zip(offs, lens)], frames, oracle)
    return offs, lens


def _exact(e, oracle, what, batch):
    """The batch and a flat frame behind it through exact placement.  With the flat frame the streams differ in size, so a capacity
    of exactly their rounded sizes either gives slots of less than a quarter frame (exact placement at once) or slots the larger
    streams outgrow (cut, then exact placement): no fixed slots fit."""
    f = batch[0]
    frames = list(batch) + [pl.flat(f.shape[1], f.shape[0], f.dtype.type, f.ndim == 3)]
    sizes = [len(_want(oracle, x)) for x in frames]
    slot = pl.device_slot(sum(_round16(s) for s in sizes), len(frames), f.nbytes)
    assert slot == 0 or max(sizes) > slot, (what, slot, sizes)
    _device(e, oracle, what, frames)


def _slots(e, oracle, what, batch):
    """The frames of the batch that fit the slot of a frame and a quarter through the device entry point with room for exactly those
    slots: k_zero_edges and k_pack into a buffer that holds a pattern, not zeros."""
    slot = pl.default_slot(batch[0].nbytes)
    frames = [f for f in batch if len(_want(oracle, f)) <= slot]
    if frames:
        assert pl.device_slot(slot * len(frames), len(frames), batch[0].nbytes) == slot
        _device(e, oracle, what, frames, slot * len(frames), slot)


# ------------------------------------------------------------------------------------------------------------------------
# 16-bit, one shape a call
# ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", pl.NAMES16)
def test_fixed_slots16(enc, oracle, name):
    """Every case through the host entry point: fixed slots of a frame and a quarter (k_zero_edges, k_pack with the slot's limit), in
    chunks of several frames, so that planes of images behind the first are placed.  The frames with two long codes outgrow that
    slot: cut, and redone with exact placement.  Then the frames that fit through the device entry point, into fixed slots of a
    buffer that is not zero."""
    c = _reach(name)
    for batch in c.batches():
        _compare(name, enc.compress_batch(batch), batch, oracle)
        _slots(enc, oracle, name + " slots", batch)


@pytest.mark.parametrize("name", pl.NAMES16)
def test_exact_placement16(enc, oracle, name):
    """Every case through the device entry point with the capacity the streams need and no more: k_place_streams, k_zero_streams and
    k_pack without a limit.  Offsets are 16-byte aligned and back to back; nothing behind the capacity is written."""
    c = _reach(name)
    for batch in c.batches():
        _exact(enc, oracle, name + " exact", batch)


@pytest.mark.parametrize("name,frames,cap,reach", pl.cut_cases(), ids=[c[0] for c in pl.cut_cases()])
def test_slot_cut16(enc, oracle, name, frames, cap, reach):
    """The batch's last stream outgrows its fixed slot, whose end is the end of the capacity: the first pack is cut inside a long run,
    or in the middle of window 0 or window 1 of a two-window tile, and must not write behind the cut -- the redo repacks every
    stream, so a word too many shows only in the guard bytes.  slot_overflows moves and every stream is the oracle's."""
    n = len(frames)
    slot = pl.device_slot(cap, n, frames[0].nbytes)
    assert slot * n == cap and len(_want(oracle, frames[-1])) > slot
    assert pl.cut_reach(pl.layout(oracle, frames[-1]), slot) == reach
    before = enc.stats()["slot_overflows"]
    _device(enc, oracle, "cut " + name, frames, cap)
    assert enc.stats()["slot_overflows"] == before + 1, enc.stats()


# ------------------------------------------------------------------------------------------------------------------------
# 16-bit, the variants
# ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(pl.mixed_sets()))
def test_mixed_shapes16(enc, oracle, name):
    """Images of one and two, or of two and three tiles in ONE mixed sub-batch (k_lengths_mixed, k_zero_edges_mixed, k_pack_mixed): the
    shorter planes have padding tiles, among them the ones behind a last real tile of five pixels; long codes, a tile boundary
    in a long code's last word, noise.  Host and device entry point; the device call's slots end at the capacity."""
    import torch

    imgs = pl.mixed_sets()[name]
    assert pl.one_bucket(imgs) and len({pl.tiles_of(im) for im in imgs}) == 2
    st = enc.stats()
    _compare(name, enc.compress_images(imgs), imgs, oracle)
    st1 = enc.stats()
    assert st1["submissions"] == st["submissions"] + 1 and st1["slot_overflows"] == st["slot_overflows"], (st, st1)
    dev = [torch.from_numpy(im).cuda() for im in imgs]
    slots = [pl.default_slot(im.nbytes) for im in imgs]
    cap = sum(slots)
    out = _guarded(cap)
    descs = [(t.data_ptr(), im.shape[1], im.shape[0], RGB if im.ndim == 3 else GRAY, D16) for im, t in zip(imgs, dev)]
    offs, lens = enc.compress_images_device(descs, out.data_ptr(), cap)
    host = out.cpu().numpy()
    _check_guard(name, host, cap)
    assert [int(o) for o in offs] == [sum(slots[:i]) for i in range(len(slots))], (name, offs)
    _compare(name + " device", [host[int(o):int(o) + int(n)].tobytes() for o, n in zip(offs, lens)], imgs, oracle)


def _surface(frames, pitch, lead=3, top=1):
    """The same-shaped gray16 frames as windows of one host array of `pitch` samples a row, a margin around each: (array, windows)"""
    h, w = frames[0].shape
    host = np.full((len(frames), h + 2 * top, pitch), 0x5A5A, np.uint16)
    assert lead + w <= pitch
    for i, f in enumerate(frames):
        host[i, top:top + h, lead:lead + w] = f
    return host, host[:, top:top + h, lead:lead + w]


def _surfaces_call(e, oracle, what, frames, pitch, overflow):
    """felics_compress_surfaces_device on pitched gray16 frames: read where they lie (k_lengths_pitched, k_pack_pitched)."""
    import torch

    host, win = _surface(frames, pitch)
    dev = torch.from_numpy(host).cuda()
    n, h, w = win.shape
    off = win.__array_interface__["data"][0] - host.__array_interface__["data"][0]
    desc = ((dev.data_ptr() + off, w, h, GRAY, D16, win.strides[1], win.strides[2], 0), win.strides[0], n)
    slot = pl.default_slot(frames[0].nbytes)
    sizes = [len(_want(oracle, f)) for f in frames]
    assert (max(sizes) > slot) == overflow, (what, slot, sizes)
    cap = n * slot
    out = _guarded(cap)
    s0, o0 = e.surface_stats(), e.stats()["slot_overflows"]
    offs, lens = e.compress_surfaces_device(desc, out.data_ptr(), cap)
    hostout = out.cpu().numpy()
    _check_guard(what, hostout, cap)
    _compare(what, [hostout[int(o):int(o) + int(k)].tobytes() for o, k in zip(offs, lens)], frames, oracle)
    s1 = e.surface_stats()
    assert s1["queued"] == s0["queued"] + 1 and s1["frames_in_place"] == s0["frames_in_place"] + n, (what, s0, s1)
    if overflow:
        assert e.stats()["slot_overflows"] > o0, what
    else:
        assert e.stats()["slot_overflows"] == o0 and [int(o) for o in offs] == [i * slot for i in range(n)], (what, offs)


def test_pitched_surfaces16(enc, oracle):
    """The window, run and shared-word cases as gray16 surfaces at a pitch larger than the row: the frames with one long code, the
    sweep of tile 1's first bit over all 32 positions, and the frames with two long codes, which outgrow their slot (the cut in
    the pitched kernel, then the redo)."""
    windows, runs, sweep = _reach("windows16"), _reach("runs16"), _reach("sweep16")
    gray = [f for f in windows.frames + runs.frames if f.ndim == 2]
    one = [f for f in gray if len(_want(oracle, f)) <= pl.default_slot(f.nbytes)]
    two = [f for f in gray if len(_want(oracle, f)) > pl.default_slot(f.nbytes)]
    assert len(one) >= 8 and len(two) >= 3
    _surfaces_call(enc, oracle, "pitched long codes", one, 96, False)
    _surfaces_call(enc, oracle, "pitched sweep", sweep.frames, 64, False)
    # (with flat frames, so that the capacity of the slots holds the streams placed back to back)
    _surfaces_call(enc, oracle, "pitched, two long codes", two[:3] + one[:1] + [pl.flat(pl.QW, pl.QH)] * 3, 81, True)


def test_views16(enc, oracle):
    """Gray16 views of several shapes cut out of one pitched device surface through felics_compress_views_device (gathered, then one
    mixed sub-batch), placed exactly: the capacity is what the streams need."""
    import torch

    imgs = pl.mixed_sets()["gray-2-3"]
    width = max(im.shape[1] for im in imgs) + 9
    surface = np.full((sum(im.shape[0] + 2 for im in imgs), width), 0x5A5A, np.uint16)
    crops, y = [], 1
    for i, im in enumerate(imgs):
        h, w = im.shape
        surface[y:y + h, 1 + i:1 + i + w] = im
        crops.append(surface[y:y + h, 1 + i:1 + i + w])
        y += h + 2
    dev = torch.from_numpy(surface).cuda()
    base = surface.__array_interface__["data"][0]
    views = [(dev.data_ptr() + c.__array_interface__["data"][0] - base, c.shape[1], c.shape[0], GRAY, D16, c.strides[0], 2, 0) for c in crops]
    cap = sum(_round16(len(_want(oracle, im))) for im in imgs)
    out = _guarded(cap)
    offs, lens = enc.compress_views_device(views, out.data_ptr(), cap)
    host = out.cpu().numpy()
    _check_guard("views", host, cap)
    _back_to_back("views", offs, lens)
    _compare("views", [host[int(o):int(o) + int(n)].tobytes() for o, n in zip(offs, lens)], imgs, oracle)


# ------------------------------------------------------------------------------------------------------------------------
# 8-bit: the remedy path
# ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", pl.NAMES8)
def test_remedy_path8(enc8, oracle, name):
    """The u8 and i16 instantiations (16-bit group totals): flat gray8 and RGB8 frames with a last tile of 5, 18, 31 and 7 pixels, the
    sweeps of tile 1's and the planes' first bit over all 32 positions, and sixteen of the longest 8-bit codes in one group; fixed
    slots (host and device entry point) and exact placement (device entry point)."""
    assert enc8.stats()["two_pass"] == 1
    c = _reach(name)
    for batch in c.batches():
        _compare(name, enc8.compress_batch(batch), batch, oracle)
        _slots(enc8, oracle, name + " slots", batch)
        _exact(enc8, oracle, name + " exact", batch)
    st = enc8.stats()
    assert st["two_pass"] == 1 and st["lookback_fallbacks"] == 0, st
