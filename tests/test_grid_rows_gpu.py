"""More same-shape RGB streams in one call than a grid has rows (65 535): the RGB conversion takes the stream from the grid's second
dimension, so every same-shape decode path cuts it into runs of at most 65 535 streams (launch_conv_uniform), each run starting at
its own planes, frames and status words.  65 600 streams of 8 x 1 pixels (the smallest width the lane forms take) from FOUR distinct
frames, stream i being frame i % 4 -- 65 535 is a multiple of 3 and of 5, so a period of 4 shows a run that starts one stream off.
Streams and indexes are built on the host from the four frames; their bytes are replicated on the device."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 65600
W, H = 8, 1
SEGMENT = 4096  # one segment per plane (K = 1)
PROBES = (0, 65534, 65535, 65536, N - 1)


@pytest.fixture(scope="module")
def enc():
    import felics_amd

    e = felics_amd.Encoder(0)
    yield e
    e.close()


def _frames(dtype):
    rng = np.random.default_rng(7)
    hi = 256 if dtype == np.uint8 else 65536
    return [rng.integers(0, hi, size=(H, W, 3)).astype(dtype) for _ in range(4)]


def _replicated(parts, align):
    """the four byte strings in slots of one size (a multiple of `align`), the group of four N / 4 times on the device:
    (device tensor, slot, offsets of the N copies, their lengths)"""
    import torch

    slot = (max(len(p) for p in parts) + align - 1) // align * align
    group = b"".join(p + bytes(slot - len(p)) for p in parts)
    d = torch.from_numpy(np.frombuffer(group, dtype=np.uint8).copy()).cuda().repeat(N // 4)
    d = torch.cat([d, torch.zeros(64, dtype=torch.uint8, device="cuda")])  # (the tests' usual slack behind the last stream)
    lens = np.array([len(p) for p in parts], dtype=np.uint64)[np.arange(N) % 4]
    return d, slot, np.arange(N, dtype=np.uint64) * slot, lens


def _check(status, d_px, frames, guard):
    host = d_px.cpu().numpy()
    assert (host[:guard] == 0xA5).all() and (host[-guard:] == 0xA5).all()
    assert status.shape == (N,) and (status == 0).all(), np.flatnonzero(status)[:8]
    four = np.stack([f.reshape(-1) for f in frames])
    got = host[guard:-guard].view(four.dtype).reshape(N, four.shape[1])
    for i in PROBES:
        assert (got[i] == four[i % 4]).all(), i
    assert (got == four[np.arange(N) % 4]).all()  # every frame against the cycle


def _target(frames):
    import torch

    guard = 256
    total = N * frames[0].nbytes
    d_px = torch.full((guard + total + guard,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    return d_px, guard, total


@pytest.mark.parametrize("lanes", (0, 1))
def test_decompress_batch_device_rgb8(enc, oracle, monkeypatch, lanes):
    """felics_decompress_batch_device, a wave per stream (k_decode8) and 64 streams per wave (k_decode8_lanes)"""
    frames = _frames(np.uint8)
    d_in, _, offs, lens = _replicated([oracle.compress(f) for f in frames], 16)
    d_px, guard, total = _target(frames)
    monkeypatch.setenv("FELICS_TEST_DECODE_LANES", str(lanes))
    before = enc.decode_stats()
    _, status = enc.decompress_batch_device(d_in.data_ptr(), offs, lens, d_px.data_ptr() + guard, total)
    after = enc.decode_stats()
    assert after["lanes8" if lanes else "wave8"] - before["lanes8" if lanes else "wave8"] == N
    _check(status, d_px, frames, guard)


def test_decompress_batch_device_indexed_rgb8(enc, oracle, monkeypatch):
    """felics_decompress_batch_device_indexed, a wave per (stream, plane): the dense indexed finish"""
    from felics_amd import api

    frames = _frames(np.uint8)
    streams = [oracle.compress(f) for f in frames]
    d_in, _, offs, lens = _replicated(streams, 16)
    d_idx, stride, _, _ = _replicated([api.index_build(s, SEGMENT) for s in streams], 16)
    d_px, guard, total = _target(frames)
    monkeypatch.delenv("FELICS_TEST_INDEX_LANES", raising=False)
    before = enc.decode_stats()
    _, status = enc.decompress_batch_device_indexed(d_in.data_ptr(), offs, lens, d_idx.data_ptr(), stride, d_px.data_ptr() + guard, total)
    assert enc.decode_stats()["segments8"] - before["segments8"] == N * 3
    _check(status, d_px, frames, guard)


def test_decompress_batch_device_indexed16_rgb16(enc, oracle, monkeypatch):
    """felics_decompress_batch_device_indexed16 in the passes its tables allow: the path that cut the grid before every path did --
    its arithmetic pinned now that all of them share it"""
    from felics_amd import api

    frames = _frames(np.uint16)
    streams = [oracle.compress(f) for f in frames]
    d_in, _, offs, lens = _replicated(streams, 16)
    d_idx, _, ioffs, ilens = _replicated([api.index16_build(s, SEGMENT) for s in streams], 64)
    d_px, guard, total = _target(frames)
    monkeypatch.delenv("FELICS_TEST_INDEX16_PASS", raising=False)
    before = enc.index16_stats()
    _, status = enc.decompress_batch_device_indexed16(d_in.data_ptr(), offs, lens, d_idx.data_ptr(), ioffs, ilens, d_px.data_ptr() + guard, total)
    assert enc.index16_stats()["segments16"] - before["segments16"] == N * 3
    _check(status, d_px, frames, guard)
