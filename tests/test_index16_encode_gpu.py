"""The 16-bit encoder's restart index on the GPU: felics_compress_batch_device_indexed16 on every case of index16_common.py and
index16_encode_cases.py -- streams against felics_compress_batch_device's, indexes against felics_index16_build's of those streams,
byte for byte --; batches, passes, the forced chain kernels, a poisoned workspace and a slot overflow; the round trip into
felics_decompress_batch_device_indexed16 without a host copy; the refusals and the two-call pattern; the counts."""
import ctypes as C
import glob
import os

import numpy as np
import pytest

from tests import index16_common as ic
from tests import index16_encode_cases as ec

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
PATTERN = 0x5A
GUARD = 4096
ALL_CASES = {**ic.cases(), **ec.cases()}


@pytest.fixture(scope="module")
def enc():
    import felics_amd

    e = felics_amd.Encoder(0)
    yield e
    e.close()


def _device(frames):
    import torch

    blob = np.ascontiguousarray(np.stack(frames)).view(np.uint8).reshape(-1)
    return torch.from_numpy(blob.copy()).cuda() if blob.size else torch.zeros(64, dtype=torch.uint8, device="cuda")


def _shape(frames):
    h, w = frames[0].shape[:2]
    return w, h, int(frames[0].ndim == 3)


def _plain(enc, frames, cap=None):
    """felics_compress_batch_device of same-shape 16-bit frames: the streams (bytes)"""
    import torch

    w, h, color = _shape(frames)
    cap = cap or len(frames) * (2 * frames[0].nbytes + 4096)
    d_in, d_out = _device(frames), torch.zeros(cap, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    offs, lens = enc.compress_batch_device(d_in.data_ptr(), len(frames), w, h, color, 1, d_out.data_ptr(), cap)
    host = d_out.cpu().numpy()
    return [host[int(o):int(o + n)].tobytes() for o, n in zip(offs, lens)]


def _indexed(enc, frames, seg, idx_cap, cap=None, expect=0):
    """one felics_compress_batch_device_indexed16 call into an index buffer of idx_cap bytes inside a pattern-filled allocation with
    GUARD bytes behind it: (streams, the index buffer's bytes, idx_offsets, idx_lens, idx_total).  Checks the return code and that
    nothing behind idx_cap changed."""
    import torch

    w, h, color = _shape(frames)
    cap = cap or len(frames) * (2 * frames[0].nbytes + 4096)
    d_in, d_out = _device(frames), torch.zeros(cap, dtype=torch.uint8, device="cuda")
    d_idx = torch.full((idx_cap + GUARD,), PATTERN, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    assert d_idx.data_ptr() % 64 == 0
    rc, offs, lens, ioffs, ilens, total = enc.compress_batch_device_indexed16_raw(d_in.data_ptr(), len(frames), w, h, color, d_out.data_ptr(), cap, seg,
                                                                                d_idx.data_ptr(), idx_cap)
    assert rc == expect, (rc, enc_error(enc))
    host, hidx = d_out.cpu().numpy(), d_idx.cpu().numpy()
    assert (hidx[idx_cap:] == PATTERN).all()
    return [host[int(o):int(o + n)].tobytes() for o, n in zip(offs, lens)], hidx[:idx_cap], ioffs, ilens, total


def enc_error(enc):
    from felics_amd import api

    return api.lib().felics_last_error(enc._h).decode()


def _check(enc, frames, seg, plain=None, slack=192, **kw):
    """the call on `frames`: streams = the unindexed call's, every index = the host builder's of its stream, offsets multiples of 64 in
    stream order, idx_total right, the pattern behind the last index unchanged.  Returns the host's indexes."""
    from felics_amd import api

    plain = plain or _plain(enc, frames)
    want = [api.index16_build(s, seg) for s in plain]
    need = sum(len(x) for x in want)
    streams, hidx, ioffs, ilens, total = _indexed(enc, frames, seg, need + slack, **kw)
    assert streams == plain
    assert total == need and [int(n) for n in ilens] == [len(x) for x in want]
    at = 0
    for i, x in enumerate(want):
        assert int(ioffs[i]) == at and at % 64 == 0
        assert hidx[at:at + len(x)].tobytes() == x, (i, seg)
        at += len(x)
    assert (hidx[at:] == PATTERN).all()
    return want


@pytest.fixture(scope="module")
def plain_streams(enc):
    """name -> the unindexed call's stream of every case: computed once, read by the tests below"""
    return {name: _plain(enc, [img]) for name, (img, _) in ALL_CASES.items()}


@pytest.mark.parametrize("name", list(ALL_CASES))
def test_every_case(enc, plain_streams, name):
    """n = 1, every segment size: stream, index, idx_lens and idx_total"""
    img = ALL_CASES[name][0]
    for seg in ic.SEGMENTS:
        _check(enc, [img], seg, plain=plain_streams[name])


def _batch(rgb):
    if rgb:
        return [ic.noise(33, 130, 1, bits, 300 + bits) for bits in (12, 10, 8, 6)] + [ic.ramp(33, 130, 1)]
    return [ic.noise(64, 130, 0, bits, 100 + bits) for bits in (12, 10, 8, 6)] + [ic.ramp(64, 130, 0)]


@pytest.mark.parametrize("rgb", (0, 1))
def test_batches(enc, rgb):
    """3, 4 and 5 frames of one shape and different content: indexes of different lengths one behind the other"""
    frames = _batch(rgb)
    for n in (3, 4, 5):
        want = _check(enc, frames[:n], 4096)
        assert len(set(len(x) for x in want)) == n


@pytest.mark.parametrize("env", ({"FELICS_WIDE_LANE": "0"}, {"FELICS_WIDE_LANE": "1"}, {"FELICS_WIDE_LANE": "7"}, {"FELICS_TEST_PASS_IMAGES": "2"},
                                 {"FELICS_POISON": "1"}), ids=lambda e: "-".join("%s=%s" % kv for kv in e.items()))
def test_forced_variants(env):
    """the same small batches whichever chain kernel gave the events their k, in three passes, on a poisoned workspace"""
    import felics_amd

    os.environ.update(env)
    try:
        with felics_amd.Encoder(0) as e:
            for rgb in (0, 1):
                before = e.index16_emit_stats()
                _check(e, _batch(rgb), 4096)
                after = e.index16_emit_stats()
                assert after["passes"] - before["passes"] == (3 if "FELICS_TEST_PASS_IMAGES" in env else 1)
    finally:
        for k in env:
            del os.environ[k]


def test_slot_overflow(enc):
    """a noise frame that outgrows its fixed slot: the batch is placed exactly (felics_stats counts the overflow), streams and indexes as ever"""
    rng = np.random.default_rng(5)
    frames = [ic.ramp(64, 130, 0), rng.integers(0, 65536, size=(130, 64), dtype=np.uint16), np.full((130, 64), 9, np.uint16), ic.noise(64, 130, 0, 4, 6)]
    plain = _plain(enc, frames)
    assert len(plain[1]) > frames[1].nbytes  # the noise frame expands
    cap = 4 * ((len(plain[1]) - 256) // 16 * 16)  # a slot a little smaller than the noise stream, still above a quarter of the frame
    assert sum((len(s) + 15) // 16 * 16 for s in plain) <= cap and cap // 4 >= frames[0].nbytes // 4
    before = enc.stats()["slot_overflows"]
    _check(enc, frames, 4096, plain=plain, cap=cap)
    assert enc.stats()["slot_overflows"] == before + 1


@pytest.mark.parametrize("rgb", (0, 1))
def test_round_trip_on_the_device(enc, rgb):
    """Encoder.compress_batch_device_indexed16 on a tensor (the two-call pattern inside), its buffers and arrays straight into
    decompress_batch_device_indexed16: the pixels equal the input, every status 0"""
    import torch

    class Frames16:  # (uint16 frames in a byte tensor: not every torch build has a uint16 dtype on the device)
        def __init__(self, tensor, shape):
            self.tensor = tensor
            self.__cuda_array_interface__ = {"shape": shape, "typestr": "<u2", "data": (tensor.data_ptr(), False), "version": 2, "strides": None}

    frames = np.stack(_batch(rgb))
    d_frames = Frames16(_device(list(frames)), frames.shape)
    res = enc.compress_batch_device_indexed16(d_frames, 4096)
    assert all(int(o) % 64 == 0 for o in res.idx_offsets)
    d_px = torch.zeros(frames.nbytes, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    hdr, status = enc.decompress_batch_device_indexed16(res.streams.data_ptr(), res.offsets, res.lens, res.index.data_ptr(), res.idx_offsets,
                                                        res.idx_lens, d_px.data_ptr(), frames.nbytes)
    assert (status == 0).all() and (hdr.width, hdr.height) == (frames.shape[2], frames.shape[1])
    assert (d_px.cpu().numpy().view(np.uint16).reshape(frames.shape) == frames).all()


def test_short_index_buffer(enc):
    """d_index_cap short of idx_total: FELICS_E_BUFFER_TOO_SMALL with the right idx_total, offsets and lens, complete streams, the
    indexes that fit written and nothing behind d_index_cap; a second call with idx_total bytes succeeds"""
    from felics_amd import api

    frames = _batch(0)
    plain = _plain(enc, frames)
    want = [api.index16_build(s, 4096) for s in plain]
    need = sum(len(x) for x in want)
    for short in (64, len(want[4]) + 64, need):  # the last index cut, the last two, no room at all
        streams, hidx, ioffs, ilens, total = _indexed(enc, frames, 4096, need - short, expect=-8)
        assert streams == plain and total == need and [int(n) for n in ilens] == [len(x) for x in want]
        at = 0
        for i, x in enumerate(want):
            assert int(ioffs[i]) == at
            if at + len(x) <= need - short:
                assert hidx[at:at + len(x)].tobytes() == x
            else:
                assert (hidx[at:] == PATTERN).all()  # an index that does not fit is not begun
                break
            at += len(x)
    _check(enc, frames, 4096, plain=plain, slack=0)


def test_refusals(enc):
    """before anything is launched: 8-bit frames, a bad segment_pixels, a misaligned or NULL index buffer, NULL arrays, an outstanding ticket"""
    import torch

    import felics_amd
    from felics_amd import api

    img = ic.noise(64, 130, 0, 10, 1)
    d_in, d_out = _device([img]), torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    d_idx = torch.full((1 << 16,), PATTERN, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    with pytest.raises(felics_amd.FelicsError) as ei:
        enc.compress_batch_device_indexed16(torch.zeros((1, 130, 64), dtype=torch.uint8, device="cuda"), 4096)
    assert ei.value.code == ic.E_UNSUPPORTED
    before = enc.stats()["submissions"]
    raw = lambda seg, idx, cap=(1 << 16) - 64: enc.compress_batch_device_indexed16_raw(d_in.data_ptr(), 1, 64, 130, 0, d_out.data_ptr(), 1 << 16, seg, idx, cap)[0]
    for seg in (0, 4095, 4097, 2048):
        assert raw(seg, d_idx.data_ptr()) == -11
    assert raw(4096, d_idx.data_ptr() + 16) == -11 and raw(4096, d_idx.data_ptr() + 32) == -11 and raw(4096, None) == -11
    a = np.zeros(1, np.uint64)
    u64 = C.POINTER(C.c_uint64)
    ptrs = [a.ctypes.data_as(u64)] * 4
    for hole in range(4):
        args = [None if i == hole else p for i, p in enumerate(ptrs)]
        assert api.lib().felics_compress_batch_device_indexed_wide(enc._h, 1, d_in.data_ptr(), 64, 130, 0, d_out.data_ptr(), 1 << 16, 4096,
                                                                    d_idx.data_ptr(), 1 << 16, *args, None) == -11
    assert raw(4096, d_idx.data_ptr()) == 0  # (idx_total may be NULL; the raw wrapper passes one, the loop above did not get that far)
    ticket = enc.submit_batch_device(d_in.data_ptr(), 1, 64, 130, 0, 1, d_out.data_ptr(), 1 << 16)
    try:
        assert raw(4096, d_idx.data_ptr()) == -11
    finally:
        enc.wait_batch(ticket)
    assert enc.stats()["submissions"] == before + 2  # the good call and the ticket: no refusal launched anything
    assert raw(4096, d_idx.data_ptr()) == 0


def test_suite_original_at_65536(enc):
    """one gray16 original of tests/golden/suite/ at segments of 65 536 pixels, against felics_index16_build"""
    from PIL import Image

    for path in sorted(glob.glob(os.path.join(GOLDEN, "suite", "*.felics"))):
        stream = open(path, "rb").read()
        if stream[4] != 0 or stream[5] != 1:
            continue
        img = np.array(Image.open(path[:-len(".felics")]))
        assert img.dtype == np.uint16
        want = _check(enc, [img], 65536)
        assert ic.Layout16(want[0]).k == (img.size + 65535) // 65536
        return
    raise AssertionError("no gray16 original under tests/golden/suite/")


def test_emit_stats(enc):
    """streams, rows (the sum of the directories' n_rows), bytes and passes of the calls so far"""
    frames = _batch(1)
    before = enc.index16_emit_stats()
    want = _check(enc, frames, 4096)
    after = enc.index16_emit_stats()
    assert after["streams"] - before["streams"] == 5 and after["passes"] - before["passes"] == 1
    assert after["rows_written"] - before["rows_written"] == sum(sum(ic.Layout16(x).n_rows()) for x in want) > 0
    assert after["index_bytes"] - before["index_bytes"] == sum(len(x) for x in want)
