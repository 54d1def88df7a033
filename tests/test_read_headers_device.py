"""felics_read_headers_device: the headers of many streams in device memory, read on the GPU in one launch.

Every status must equal what the host's felics_read_header returns for the stream's first min(len, 14) bytes, and every valid
header must equal the host's.  The CPU test checks the ABI surface; the GPU tests compare code for code over truncations and
mutations, the golden streams, streams of many shapes from one felics_compress_images_device call, and the refusals."""
import ctypes as C
import glob
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
E_INVALID_ARGUMENT = -11


def test_read_headers_abi_surface():
    """The symbol is exported and listed, a NULL context / NULL arrays are refused, the Python method exists."""
    from felics_amd import api

    L = api.lib()
    assert hasattr(L, "felics_read_headers_device")
    assert "felics_read_headers_device" in api.EXPORTS
    offs = (C.c_uint64 * 1)()
    lens = (C.c_uint64 * 1)(14)
    hdrs = (api._CHeader * 1)()
    st = (C.c_int * 1)()
    assert L.felics_read_headers_device(None, 1, C.c_void_p(16), offs, lens, hdrs, st) == E_INVALID_ARGUMENT
    assert L.felics_read_headers_device(None, 0, None, None, None, None, None) == E_INVALID_ARGUMENT
    assert callable(getattr(api.Encoder, "read_headers_device", None))


def _host_header(data):
    """felics_read_header on the host: (code, (color, depth, w, h) or None)."""
    from felics_amd import api

    h = api._CHeader()
    buf = np.frombuffer(bytes(data), dtype=np.uint8)
    rc = api.lib().felics_read_header(buf.ctypes.data if len(buf) else None, len(buf), C.byref(h))
    return rc, ((h.color_type, h.pixel_depth, h.width, h.height) if rc == 0 else None)


def _device_headers(enc, streams):
    """The streams packed into one device buffer at unaligned offsets; felics_read_headers_device over all of them."""
    import torch

    offs, blob = [], bytearray()
    for i, s in enumerate(streams):
        blob += bytes(i % 5)  # (offsets of every alignment)
        offs.append(len(blob))
        blob += s
    d = torch.from_numpy(np.frombuffer(bytes(blob) + bytes(16), dtype=np.uint8).copy()).cuda()
    torch.cuda.synchronize()
    return enc.read_headers_device(d.data_ptr(), offs, [len(s) for s in streams])


def _check(enc, streams):
    hdrs, status = _device_headers(enc, streams)
    assert len(hdrs) == len(streams) == len(status)
    for i, s in enumerate(streams):
        rc, want = _host_header(s)
        assert status[i] == rc, (i, bytes(s[:14]), status[i], rc)
        got = None if hdrs[i] is None else (int(hdrs[i].color_type), int(hdrs[i].pixel_depth), hdrs[i].width, hdrs[i].height)
        assert got == want, (i, got, want)
    return hdrs, status


@pytest.fixture(scope="module")
def enc():
    import felics_amd

    e = felics_amd.Encoder(0)
    yield e
    e.close()


@pytest.mark.gpu
def test_prefixes_and_mutations_match_the_host(enc, oracle):
    """Every prefix length 0..14 of valid streams (gray8, RGB8, gray16, RGB16) and mutations of each of bytes 0..13: code for code
    what felics_read_header says, in one call."""
    rng = np.random.default_rng(21)
    valid = [oracle.compress(rng.integers(0, 256, size=(5, 7), dtype=np.uint8)),
             oracle.compress(rng.integers(0, 256, size=(3, 300, 3), dtype=np.uint8)),
             oracle.compress(rng.integers(0, 65536, size=(9, 2), dtype=np.uint16)),
             oracle.compress(rng.integers(0, 65536, size=(1, 1, 3), dtype=np.uint16))]
    streams = []
    for v in valid:
        streams += [v[:k] for k in range(0, 15)] + [v]
        for pos in range(14):
            for val in (0, 1, 2, 0x46, 0xFF, v[pos] ^ 0x01):
                b = bytearray(v)
                b[pos] = val
                streams.append(bytes(b))
                streams.append(bytes(b[: pos + 1]))  # mutated and cut right behind the mutation
    hdrs, status = _check(enc, streams)
    assert (status == 0).sum() > 0 and (status != 0).sum() > 0
    # every code of felics_read_header occurs
    assert {-1, -5, -6, -7} <= set(int(s) for s in status)


@pytest.mark.gpu
def test_golden_and_mixed_shapes(enc, oracle):
    """The 23 committed .felics streams and 300 streams of random shapes and types encoded in ONE felics_compress_images_device
    call, read back in one call: every header equals the host's and names the shape that was encoded."""
    import torch

    golden = sorted(glob.glob(os.path.join(GOLDEN, "*.felics")) + glob.glob(os.path.join(GOLDEN, "suite", "*.felics")))
    assert len(golden) == 23
    gs = [open(p, "rb").read() for p in golden]
    hdrs, status = _check(enc, gs)
    assert (status == 0).all()
    rng = np.random.default_rng(22)
    imgs = []
    for _ in range(300):
        w, h = int(rng.integers(0, 40)), int(rng.integers(0, 40))
        kind = int(rng.integers(0, 4))
        shape = (h, w) if kind % 2 == 0 else (h, w, 3)
        dt, mx = (np.uint8, 256) if kind < 2 else (np.uint16, 65536)
        imgs.append(rng.integers(0, mx, size=shape).astype(dt))
    frames = [torch.from_numpy(np.ascontiguousarray(im).view(np.uint8).reshape(-1)).cuda() for im in imgs]
    descs = [(f.data_ptr() if im.size else 0, im.shape[1], im.shape[0], int(im.ndim == 3), int(im.dtype == np.uint16))
             for f, im in zip(frames, imgs)]
    cap = sum(im.nbytes * 2 + 96 for im in imgs) + (1 << 16)
    d_out = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    offs, lens = enc.compress_images_device(descs, d_out.data_ptr(), cap)
    hdrs, status = enc.read_headers_device(d_out.data_ptr(), offs, lens)
    assert (status == 0).all()
    for h, (_, w, hh, c, d) in zip(hdrs, descs):
        assert (h.width, h.height, int(h.color_type), int(h.pixel_depth)) == (w, hh, c, d)
    host = d_out.cpu().numpy()
    for i in range(0, 300, 37):
        assert _host_header(host[int(offs[i]): int(offs[i] + lens[i])].tobytes())[1] == (descs[i][3], descs[i][4], descs[i][1], descs[i][2])


@pytest.mark.gpu
def test_refusals_and_empty_calls(enc):
    """n = 0 returns OK; with a ticket outstanding the call returns -11 and puts it in every status."""
    import torch

    import felics_amd
    from felics_amd import api

    hdrs, status = enc.read_headers_device(0, [], [])
    assert hdrs == [] and len(status) == 0
    frames = torch.zeros((2, 64, 64), dtype=torch.uint8, device="cuda")
    out = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    offs, lens = enc.compress_batch_device(frames.data_ptr(), 2, 64, 64, 0, 0, out.data_ptr(), out.numel())
    sub = enc.submit_batch_device(frames.data_ptr(), 2, 64, 64, 0, 0, out.data_ptr() + (1 << 15), 1 << 15)
    try:
        with pytest.raises(api.FelicsError) as ei:
            enc.read_headers_device(out.data_ptr(), offs, lens)
        assert ei.value.code == E_INVALID_ARGUMENT
    finally:
        enc.wait_batch(sub)
    hdrs, status = enc.read_headers_device(out.data_ptr(), offs, lens)
    assert (status == 0).all() and all(h == felics_amd.Header(0, 0, 64, 64) for h in hdrs)
