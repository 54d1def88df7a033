"""16-bit streams decoded 64 to a wave, a lane per stream (k_decode16_lanes), forced with FELICS_TEST_DECODE16_LANES=1 on small
batches: pixels and acceptance against the oracle, and through Encoder.decode_stats() that the streams really took that form."""
import contextlib
import glob
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
VAR = "FELICS_TEST_DECODE16_LANES"


@pytest.fixture(scope="module")
def enc():
    import felics_amd

    e = felics_amd.Encoder(0)
    yield e
    e.close()


@contextlib.contextmanager
def _env(**kv):
    """environment variables for the calls inside (the library reads them per call); None unsets"""
    old = {k: os.environ.get(k) for k in kv}
    try:
        for k, v in kv.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _rows(npix):
    """felics_lanetable.h, dec16l_rows: rows of one plane's table"""
    need = 2 * min(max(npix - 2, 0), 131071)
    if need > 65536:
        return 131071
    rows = 64
    while rows < need:
        rows *= 2
    return rows


def _blob(streams):
    offs, blob = [], bytearray()
    for s in streams:
        offs.append(len(blob))
        blob += s + bytes((-len(s)) % 16)
    return offs, np.frombuffer(bytes(blob) + bytes(16), dtype=np.uint8).copy()


def _decode(enc, streams, shape, guard=0):
    """One same-shape call on u16 streams -> (status, frames, the call's decode_stats delta); a failing call's status comes from
    the exception.  guard: bytes of 0xA5 kept before and behind d_pixels, checked untouched."""
    import felics_amd
    import torch

    n = len(streams)
    offs, blob = _blob(streams)
    d_in = torch.from_numpy(blob).cuda()
    per = int(np.prod(shape)) * 2
    d_px = torch.full((guard + max(per * n, 16) + guard,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    before = enc.decode_stats()
    try:
        _, status = enc.decompress_batch_device(d_in.data_ptr(), offs, [len(s) for s in streams], d_px.data_ptr() + guard, per * n)
    except felics_amd.DecompressionError as e:
        status = e.status
    after = enc.decode_stats()
    host = d_px.cpu().numpy()
    if guard:
        assert (host[:guard] == 0xA5).all() and (host[guard + per * n:][-guard:] == 0xA5).all()
        assert (host[guard + per * n:] == 0xA5).all()
    frames = [host[guard + i * per:guard + (i + 1) * per].view(np.uint16).reshape(shape) for i in range(n)]
    delta = {k: after[k] - before[k] for k in after if k != "lanes16_table_bytes"}
    delta["lanes16_table_bytes"] = after["lanes16_table_bytes"]
    return np.asarray(status), frames, delta


def _only(delta, **want):
    """the call's streams were counted in exactly these forms"""
    forms = ("wave8", "lanes8", "wave16", "lanes16", "host", "undecoded")
    assert {k: delta[k] for k in forms} == {k: want.get(k, 0) for k in forms}, delta
    assert delta["streams"] == sum(want.values()), delta


def _content(h, w, rgb, count, rng):
    """`count` frames: synth.gray16 crops and full-range noise, alternating"""
    from felics_amd import synth

    base = synth.gray16(max(w + 40, 128), max(h + 40, 128), 1)
    out = []
    for i in range(count):
        if i % 2:
            out.append(rng.integers(0, 65536, size=(h, w, 3) if rgb else (h, w), dtype=np.uint16))
        else:
            g = base[i % 37:i % 37 + h, (3 * i) % 31:(3 * i) % 31 + w]
            out.append(np.stack([g, np.roll(g, 3, axis=1), 65535 - g], -1).copy() if rgb else g.copy())
    return out


SHAPES = [(1, 8), (2, 8), (3, 9), (7, 13), (33, 96), (64, 64)]


@pytest.mark.parametrize("rgb", [False, True], ids=["gray16", "rgb16"])
def test_shapes_counts_and_the_split(enc, oracle, rgb):
    """Every shape as 1, 63, 64 and 65 streams per call (a partial wave, a full one, a second wave with one lane): pixels against
    the sources and the oracle's decoder, all streams counted in lanes16 -- and the shapes the form does not take, (5, 7) (W < 8)
    and (0, 5), in wave16 under the same switch."""
    rng = np.random.default_rng(31 + rgb)
    with _env(**{VAR: "1"}):
        for h, w in SHAPES:
            shape = (h, w, 3) if rgb else (h, w)
            imgs = _content(h, w, rgb, 6, rng)
            streams = [oracle.compress(im) for im in imgs]
            for s, im in zip(streams, imgs):
                assert (oracle.decompress(s) == im).all()
            for n in (1, 63, 64, 65):
                status, back, d = _decode(enc, [streams[i % 6] for i in range(n)], shape)
                assert (status == 0).all(), (h, w, n, status)
                for i, b in enumerate(back):
                    assert (b == imgs[i % 6]).all(), (h, w, n, i)
                _only(d, lanes16=n)
                assert d["lanes16_table_bytes"] == n * (3 if rgb else 1) * _rows(h * w) * 64
        for h, w in [(5, 7), (0, 5)]:
            shape = (h, w, 3) if rgb else (h, w)
            imgs = [rng.integers(0, 65536, size=shape, dtype=np.uint16) for _ in range(3)]
            status, back, d = _decode(enc, [oracle.compress(im) for im in imgs], shape)
            assert (status == 0).all() and all((b == im).all() for b, im in zip(back, imgs))
            _only(d, wave16=3)
            assert d["lanes16_table_bytes"] == 0


# one shape on either side of every switch of dec16l_rows (pixel counts 34 | 35, 66 | 67, ... 32 770 | 32 771: the last one is the
# switch to the dense table), W >= 8 and rows the LDS of the wave form would hold
SWITCH_SHAPES = [((4, 8), (4, 9)), ((8, 8), (4, 17)), ((13, 10), (12, 11)), ((3, 86), (20, 13)), ((2, 257), (4, 129)),
                 ((2, 513), (4, 257)), ((2, 1025), (4, 513)), ((2, 2049), (4, 1025)), ((2, 4097), (4, 2049)), ((2, 8193), (4, 4097)),
                 ((10, 3277), (129, 256)), ((128, 256), (129, 256))]


def test_the_table(enc, oracle):
    """What the hashed table must hold: full-range noise at 64 x 64 (about 3 800 contexts in 8 192 rows), noise on either side of
    every switch of the sizing rule up to the dense table, frames of sixteen contexts all congruent modulo 4096, and rgb16 noise
    (Co / Cg contexts above 65 535, negative samples)."""
    rng = np.random.default_rng(41)
    with _env(**{VAR: "1"}):
        imgs = [rng.integers(0, 65536, size=(64, 64), dtype=np.uint16) for _ in range(3)]
        status, back, d = _decode(enc, [oracle.compress(im) for im in imgs], (64, 64))
        assert (status == 0).all() and all((b == im).all() for b, im in zip(back, imgs))
        _only(d, lanes16=3)
        assert d["lanes16_table_bytes"] == 3 * 512 * 1024
        for pair in SWITCH_SHAPES:
            below, above = _rows(pair[0][0] * pair[0][1]), _rows(pair[1][0] * pair[1][1])
            assert pair == SWITCH_SHAPES[-1] or above == 131071 or above == 2 * below, pair
            assert pair != SWITCH_SHAPES[-1] or (below, above) == (65536, 131071)
            for h, w in pair:
                imgs = [rng.integers(0, 65536, size=(h, w), dtype=np.uint16) for _ in range(2)]
                status, back, d = _decode(enc, [oracle.compress(im) for im in imgs], (h, w))
                assert (status == 0).all(), (h, w, status)
                assert all((b == im).all() for b, im in zip(back, imgs)), (h, w)
                _only(d, lanes16=2)
                assert d["lanes16_table_bytes"] == 2 * _rows(h * w) * 64, (h, w)
        imgs = [(rng.integers(0, 16, size=(48, 40)) * 4096).astype(np.uint16) for _ in range(3)]
        status, back, d = _decode(enc, [oracle.compress(im) for im in imgs], (48, 40))
        assert (status == 0).all() and all((b == im).all() for b, im in zip(back, imgs))
        _only(d, lanes16=3)
        imgs = [rng.integers(0, 65536, size=(40, 56, 3), dtype=np.uint16) for _ in range(3)]
        imgs.append(np.stack([imgs[0][..., 0], 65535 - imgs[0][..., 0], imgs[1][..., 2] & 1], -1).copy())  # Co / Cg at both ends
        status, back, d = _decode(enc, [oracle.compress(im) for im in imgs], (40, 56, 3))
        assert (status == 0).all() and all((b == im).all() for b, im in zip(back, imgs))
        _only(d, lanes16=4)


def test_long_codes_beside_ordinary_streams(enc, oracle):
    """A frame of 9s with 60 samples of 65 535, behind one sample of 10 that teaches context 0 k = 0 (so the first of them is a unary
    run of 65 525 ones at k = 0, read by lane_rice_long: asserted from the oracle's trace), and the quiet frame in one wave with
    62 ordinary streams: the other lanes wait on the long runs and come out unharmed."""
    from felics_amd import synth
    from tests.decode_cases import longest_run_at_k0

    rng = np.random.default_rng(12)
    quiet = np.full((40, 300), 9, np.uint16)
    spikes = quiet.copy()
    spikes[rng.integers(0, 40, 60), rng.integers(0, 300, 60)] = 65535
    spikes[0, :8] = 9
    spikes[0, 3] = 10
    assert longest_run_at_k0(spikes) >= 65525
    base = synth.gray16(640, 360, 2)
    imgs = [spikes, quiet] + [base[3 * i:3 * i + 40, 5 * i:5 * i + 300].copy() for i in range(62)]
    with _env(**{VAR: "1"}):
        status, back, d = _decode(enc, [oracle.compress(im) for im in imgs], (40, 300))
    assert (status == 0).all()
    assert all((b == im).all() for b, im in zip(back, imgs))
    _only(d, lanes16=64)


def test_two_calls_find_fresh_tables(enc, oracle):
    """Two calls in a row on one context with different content of one shape (the second finds the first one's rows: another
    epoch), then the golden 16-bit files of 256 x 256 (the dense table) twice."""
    from PIL import Image

    rng = np.random.default_rng(43)
    with _env(**{VAR: "1"}):
        for _ in range(2):
            imgs = _content(50, 70, False, 5, rng)
            imgs = [np.roll(im, int(rng.integers(1, 9)), axis=1) for im in imgs]
            status, back, d = _decode(enc, [oracle.compress(im) for im in imgs], (50, 70))
            assert (status == 0).all() and all((b == im).all() for b, im in zip(back, imgs))
            _only(d, lanes16=5)
        seen = 0
        for p in sorted(glob.glob(os.path.join(GOLDEN, "*.tiff.felics"))):
            img = np.array(Image.open(p[:-len(".felics")]))
            if img.dtype != np.uint16 or img.shape != (256, 256):
                continue
            seen += 1
            stream = open(p, "rb").read()
            for _ in range(2):
                status, back, d = _decode(enc, [stream, stream], (256, 256))
                assert (status == 0).all() and (back[0] == img).all() and (back[1] == img).all(), p
                _only(d, lanes16=2)
                assert d["lanes16_table_bytes"] == 2 * 131071 * 64
        assert seen >= 1


def test_corrupt_streams_in_one_wave(enc, oracle):
    """One wave of 64 streams: truncated, a bad colour byte, 0xFF from byte 30 on, another shape, 13 bytes, 24 single-bit flips, good
    ones around them.  Nonzero status wherever the oracle rejects, the oracle's pixels where both accept, the good frames intact,
    nothing written outside d_pixels, and the same streams accepted as by the wave form."""
    from felics_amd import synth

    rng = np.random.default_rng(12)
    img = synth.gray16(640, 360, 0)[:50, :70].copy()
    good = oracle.compress(img)
    other = oracle.compress(synth.gray16(640, 360, 0)[:51, :70].copy())
    bad = [good[: len(good) // 2], good[:4] + b"\x07" + good[5:], good[:30] + b"\xff" * (len(good) - 30), other, good[:13]]
    flips = []
    for _ in range(24):
        b = bytearray(good)
        b[int(rng.integers(14, len(b)))] ^= 1 << int(rng.integers(0, 8))
        flips.append(bytes(b))
    streams = [good] + bad + flips
    streams += [good] * (64 - len(streams))
    with _env(**{VAR: "1"}):
        status, back, d = _decode(enc, streams, (50, 70), guard=64)
    _only(d, lanes16=64)
    with _env(**{VAR: "0"}):
        status_wave, _, d_wave = _decode(enc, streams, (50, 70), guard=64)
    _only(d_wave, wave16=64)
    assert ((status == 0) == (status_wave == 0)).all(), (status, status_wave)
    assert status[1] == -1 and status[2] == -5 and status[4] == -4 and status[5] == -1
    rejected = 0
    for i, s in enumerate(streams):
        try:
            want = oracle.decompress(s)
            accepted = want.shape == img.shape and want.dtype == np.uint16
        except Exception:
            accepted = False
        if s is good:
            assert accepted and status[i] == 0 and (back[i] == img).all(), i
        if not accepted:
            rejected += 6 <= i < 30
            assert status[i] != 0, i
        elif status[i] == 0:
            assert (back[i] == want).all(), i
    assert rejected == 24  # (the oracle rejects every flip of this seed)


def test_mixed_call(enc, oracle):
    """felics_decompress_images_device: 70 gray16 of 9 x 13 (one wave + 6 a wave each), 64 rgb16 of 8 x 8 (one wave), 3 gray16 of
    20 x 20, 10 gray8 and a stream with a bad signature in one call."""
    import felics_amd
    import torch

    rng = np.random.default_rng(44)
    imgs = [im for im in _content(9, 13, False, 70, rng)] + _content(8, 8, True, 64, rng) + _content(20, 20, False, 3, rng)
    imgs += [rng.integers(0, 256, size=(11, 17), dtype=np.uint8) for _ in range(10)]
    order = rng.permutation(len(imgs))
    imgs = [imgs[i] for i in order]
    streams = [oracle.compress(im) for im in imgs]
    streams.insert(40, b"XLCS" + streams[0][4:])
    imgs.insert(40, None)
    offs, blob = _blob(streams)
    d_in = torch.from_numpy(blob).cuda()
    cap = sum((im.nbytes + 15) // 16 * 16 for im in imgs if im is not None)
    d_px = torch.full((cap + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    before = enc.decode_stats()
    with _env(**{VAR: "1"}), pytest.raises(felics_amd.DecompressionError) as ei:
        enc.decompress_images_device(d_in.data_ptr(), offs, [len(s) for s in streams], d_px.data_ptr(), cap)
    after = enc.decode_stats()
    status, po = ei.value.status, ei.value.pix_offsets
    host = d_px.cpu().numpy()
    assert (host[cap:] == 0xA5).all()
    at = 0
    for i, im in enumerate(imgs):
        assert po[i] % 16 == 0 and po[i] == at, i
        if im is None:
            assert status[i] == -7  # FELICS_E_INVALID_SIGNATURE
            continue
        assert status[i] == 0, i
        got = host[int(po[i]):int(po[i]) + im.nbytes].view(im.dtype).reshape(im.shape)
        assert (got == im).all(), (i, im.shape)
        at += (im.nbytes + 15) // 16 * 16
    d = {k: after[k] - before[k] for k in after}
    assert (d["lanes16"], d["wave16"], d["undecoded"], d["wave8"] + d["lanes8"], d["host"], d["streams"]) == (128, 9, 1, 10, 0, 148), d
    assert after["lanes16_table_bytes"] == max(64 * _rows(9 * 13), 64 * 3 * _rows(64)) * 64


def test_passes(enc, oracle):
    """FELICS_TEST_DECODE16_LANES_PASS=64: 130 streams in three passes (64, 64 and 2 streams) over one pass's tables, in the
    same-shape call and 128 + 2 in the mixed one."""
    import torch

    rng = np.random.default_rng(45)
    imgs = _content(12, 20, False, 130, rng)
    streams = [oracle.compress(im) for im in imgs]
    with _env(**{VAR: "1", "FELICS_TEST_DECODE16_LANES_PASS": "64"}):
        status, back, d = _decode(enc, streams, (12, 20))
        assert (status == 0).all() and all((b == im).all() for b, im in zip(back, imgs))
        _only(d, lanes16=130)
        assert d["lanes16_table_bytes"] == 64 * _rows(240) * 64
        offs, blob = _blob(streams)
        d_in = torch.from_numpy(blob).cuda()
        d_px = torch.zeros(130 * 480, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        before = enc.decode_stats()
        po, _, status = enc.decompress_images_device(d_in.data_ptr(), offs, [len(s) for s in streams], d_px.data_ptr(), d_px.numel())
        after = enc.decode_stats()
    host = d_px.cpu().numpy()
    assert (status == 0).all()
    for i, im in enumerate(imgs):
        assert (host[int(po[i]):int(po[i]) + 480].view(np.uint16).reshape(12, 20) == im).all(), i
    assert (after["lanes16"] - before["lanes16"], after["wave16"] - before["wave16"]) == (128, 2)
    assert after["lanes16_table_bytes"] == 64 * _rows(240) * 64


def test_default_choice(enc, oracle):
    """Without the switch 64 small streams are below any threshold and keep the wave form, as before; from the measured threshold on
    (if the measurement found one) the same-shape call takes the lane form by itself."""
    from felics_amd import api

    rng = np.random.default_rng(46)
    imgs = _content(8, 8, False, 6, rng)
    streams = [oracle.compress(im) for im in imgs]
    with _env(**{VAR: None}):
        status, back, d = _decode(enc, [streams[i % 6] for i in range(64)], (8, 8))
        assert (status == 0).all() and all((b == imgs[i % 6]).all() for i, b in enumerate(back))
        _only(d, wave16=64)
        n = api.decode16_lanes_min_streams(0)
        assert n > 64 and api.decode16_lanes_min_streams(1) > 64
        if n <= 8192:
            status, back, d = _decode(enc, [streams[i % 6] for i in range(n)], (8, 8))
            assert (status == 0).all() and all((b == imgs[i % 6]).all() for i, b in enumerate(back))
            _only(d, lanes16=n)
