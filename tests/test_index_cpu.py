"""Restart index, host side (no GPU): felics_index_size, felics_index_build and felics_decompress_indexed against felics_decompress,
the original pixels and a decoder model written here from the format's description; the refusals; index_fuzz under sanitizers."""
import ctypes as C
import glob
import io
import json
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import index_common as ic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
CSRC = os.path.join(ROOT, "felics_amd", "csrc")
FUZZ = os.path.join(ROOT, "felics_amd", "_build", "asan", "index_fuzz")

NEW_SYMBOLS = ("felics_index_size", "felics_index_build", "felics_decompress_indexed", "felics_decompress_batch_device_indexed",
               "felics_compress_batch_device_indexed", "felics_get_index_stats")


@pytest.fixture(scope="module")
def api():
    from felics_amd import api as a

    a.lib()
    return a


@pytest.fixture(scope="module")
def cases(oracle):
    """(w, h, rgb) -> [(image, oracle stream)]: computed once, read by every test"""
    out = {}
    for w, h in ic.SHAPES:
        for rgb in (0, 1):
            out[(w, h, rgb)] = [(im, oracle.compress(im)) for im in ic.images(w, h, rgb, 2)]
    return out


def test_abi_surface(api):
    L = api.lib()
    for name in NEW_SYMBOLS:
        assert hasattr(L, name) and name in api.EXPORTS, name
    for name in ("index_size", "index_build", "decompress_indexed"):
        assert callable(getattr(api, name))
    assert callable(api.Encoder.decompress_batch_device_indexed) and callable(api.Encoder.compress_batch_device_indexed)
    assert L.felics_compress_batch_device_indexed(None, 1, None, 1, 1, 0, 0, None, 0, 4096, None, 0, None, None) == -11
    assert L.felics_strerror(ic.E_INVALID_INDEX) and b"index" in L.felics_strerror(ic.E_INVALID_INDEX)
    assert api.INDEX_GRANULE == ic.GRANULE and api.E_INVALID_INDEX == ic.E_INVALID_INDEX
    # felics_get_index_stats refuses NULL before anything touches a device, and never writes more than it is given
    st = api._CIndexStats(7, 7)
    assert L.felics_get_index_stats(None, C.byref(st), C.sizeof(st)) == -11 and (st.streams, st.segments8) == (7, 7)
    assert L.felics_decompress_batch_device_indexed(None, 1, None, None, None, None, 0, None, 0, None, None) == -11


def test_index_size_formula(api):
    for w, h in ic.SHAPES + [(3840, 2160), (1, 1), (2, 1), (70000, 3)]:
        for color in (0, 1):
            for seg in ic.SEGMENTS + (4096 * 32, 4096 * 128):
                assert api.index_size(w, h, color, 0, seg) == ic.index_size(w, h, color, seg), (w, h, color, seg)
            assert api.index_size(w, h, color, 1, 4096) == 0  # 16-bit images have no index
            for seg in (0, 4095, 6000):
                assert api.index_size(w, h, color, 0, seg) == 0
    # the figures of the format's description: ~10.8 KB per gray 4K checkpoint, 689 KB per frame at K = 64
    assert ic.index_size(3840, 2160, 0, 4096 * 32) == 64 + 64 * 10768 and 688e3 < ic.index_size(3840, 2160, 0, 4096 * 32) < 690e3
    assert ic.index_size(0, 5, 1, 4096) == 64


def test_roundtrip_all_shapes(api, cases, oracle):
    for (w, h, rgb), pairs in cases.items():
        for img, stream in pairs:
            plain = api.decompress_bytes(stream)
            for seg in ic.SEGMENTS:
                index = api.index_build(stream, seg)
                assert len(index) == ic.index_size(w, h, rgb, seg)
                out = api.decompress_indexed(stream, index)
                assert out.shape == img.shape and (out == img).all() and (out == plain).all(), (w, h, rgb, seg)


def test_roundtrip_golden_streams(api):
    """the committed 8-bit streams of tests/golden/ (written by the reference's encoder)"""
    from PIL import Image

    seen = 0
    for path in sorted(glob.glob(os.path.join(GOLDEN, "*.felics"))):
        stream = open(path, "rb").read()
        if stream[5] != 0:
            continue
        img = np.array(Image.open(path[:-len(".felics")]))
        for seg in ic.SEGMENTS:
            out = api.decompress_indexed(stream, api.index_build(stream, seg))
            assert out.dtype == img.dtype and out.shape == img.shape and (out == img).all(), (path, seg)
        seen += 1
    pins = json.load(open(os.path.join(GOLDEN, "pins.json")))["files"]
    assert seen == sum(1 for f in pins.values() if f["dtype"] == "uint8") >= 5


# ---- the format, from its description: a plain decoder that snapshots at every granule --------------------------------------

class _Bits:
    """reads of at most 57 bits: the 8 bytes at the bit position hold them, so a read costs the same anywhere in the stream"""

    def __init__(self, data):
        self.data, self.total, self.pos = bytes(data) + bytes(8), 8 * len(data), 0

    def get(self, n):
        assert self.pos + n <= self.total
        at, skip = self.pos >> 3, self.pos & 7
        assert skip + n <= 64
        self.pos += n
        return (int.from_bytes(self.data[at:at + 8], "big") >> (64 - skip - n)) & ((1 << n) - 1)


def _model_checkpoints(stream):
    """Decodes an 8-bit stream and returns (per plane: list of (p0, bit_offset, table copy, plane samples so far)), last event per
    context and plane, plane_end_bit, planes) with a snapshot at every multiple of GRANULE."""
    color = stream[4]
    w, h = struct.unpack(">II", stream[6:14])
    npix, planes, nrows = w * h, (3 if color else 1), (511 if color else 256)
    br = _Bits(stream)
    br.pos = 112
    snaps, lasts, ends, samples = [], [], [], []
    for _ in range(planes):
        start = br.pos
        raw = [br.get(32), br.get(32)]
        raw = [r - (1 << 32) if r >> 31 else r for r in raw]
        p, table, last, snap = [0] * npix, [[0] * 6 for _ in range(nrows)], {}, []
        x = y = 0
        for i in range(npix):
            if i % ic.GRANULE == 0:
                snap.append((i, start if i == 0 else br.pos, [row[:] for row in table]))
            if i < 2:
                p[i] = raw[i]
            else:
                if x > 0 and y > 0:
                    a, b = p[i - 1], p[i - w]
                elif y == 0:
                    a, b = p[i - 1], p[i - 2]
                elif y >= 2:
                    a, b = p[i - w], p[i - 2 * w]
                else:
                    a, b = p[i - w], p[i - w + 1]
                lo, hi = min(a, b), max(a, b)
                ctx = hi - lo
                if br.get(1):  # in range: phased-in binary code of p - lo
                    n = ctx + 1
                    m = n.bit_length() - 1
                    right, left = (2 << m) - n, n - (1 << m)
                    r = br.get(m)
                    if r >= right:
                        r = (r - right) * 2 + right + br.get(1)
                    p[i] = lo + (r + left) % n
                else:
                    above = br.get(1)
                    row = table[ctx]
                    k = max(range(6), key=lambda kk: (-row[kk], kk))  # smallest counter, ties to the largest k
                    q = 0
                    while br.get(1):
                        q += 1
                    e = (q << k) + br.get(k)
                    for kk in range(6):
                        row[kk] += (e >> kk) + 1 + kk
                    if min(row) > 1024:
                        row[:] = [v >> 1 for v in row]
                    last[ctx] = i
                    p[i] = hi + e + 1 if above else lo - e - 1
            x += 1
            if x == w:
                x, y = 0, y + 1
        snaps.append(snap)
        lasts.append(last)
        ends.append(br.pos)
        samples.append(p)
    return (color, w, h), snaps, lasts, ends, samples


def _model_index(model, seg):
    (color, w, h), snaps, lasts, ends, samples = model
    planes, nctx, fmt = (3, 512, "<h") if color else (1, 256, "<B")
    k = (w * h + seg - 1) // seg
    out = bytearray(b"FLCX" + struct.pack("<HBBIIII", 1, color, 0, w, h, seg, k) + struct.pack("<3Q", *(ends + [0, 0])[:3]) + bytes(16))
    for c in range(planes):
        for j in range(k):
            p0, bit, table = snaps[c][j * seg // ic.GRANULE]
            assert p0 == j * seg
            cp = bytearray(struct.pack("<Q", bit))
            for ctx in range(nctx):
                live = j > 0 and ctx < len(table) and lasts[c].get(ctx, -1) >= p0  # canonical: zeros unless an event is still to come
                cp += struct.pack("<6H", *(table[ctx] if live else [0] * 6))
            for t in range(p0 - 2 * w, p0):
                cp += struct.pack(fmt, samples[c][t] if t >= 0 else 0)
            cp += bytes((-len(cp)) % 16)
            out += cp
    return bytes(out)


def test_index_bytes_equal_the_model(api, cases):
    """felics_index_build's bytes against the model above, gray and RGB, on the shapes of at most three tiles."""
    checked = 0
    for (w, h, rgb), pairs in cases.items():
        if w * h > 3 * ic.GRANULE:
            continue
        img, stream = pairs[0]
        model = _model_checkpoints(stream)
        for c in range(3 if rgb else 1):
            if w * h:
                assert len(model[4][c]) == w * h
        for seg in ic.SEGMENTS:
            got, want = api.index_build(stream, seg), _model_index(model, seg)
            assert len(got) == len(want) and got == want, (w, h, rgb, seg, next(i for i in range(min(len(got), len(want))) if got[i] != want[i]))
            checked += 1
    assert checked == 2 * 2 * sum(1 for w, h in ic.SHAPES if w * h <= 3 * ic.GRANULE)


MODEL_FRAMES = [(4096, 132, 0, (0, 1, 130, 131)), (1000, 541, 0, (0, 65, 131)), (1000, 271, 1, (0, 1, 66))]
MODEL_SEGMENTS = (4096, 4096 * 9, 65536)


@pytest.mark.parametrize("w,h,rgb,loud", MODEL_FRAMES, ids=lambda v: str(v).replace(" ", ""))
def test_index_bytes_equal_the_model_past_64_checkpoints(api, oracle, w, h, rgb, loud):
    """felics_index_build's bytes against the model on banded frames of more than 64 checkpoints and of 9 and 16 tiles per segment
    (K = 132, 133 and 67 at 4096): the builder is what the encoder's index is held against at these sizes (test_index_large_gpu.py).
    The model decodes each frame once."""
    stream = oracle.compress(ic.banded(w, h, rgb, loud))
    model = _model_checkpoints(stream)
    for seg in MODEL_SEGMENTS:
        got, want = api.index_build(stream, seg), _model_index(model, seg)
        assert ic.Layout(got).k == (w * h + seg - 1) // seg
        d = ic.first_difference(got, want)
        assert len(got) == len(want) and d is None, (w, h, rgb, seg, d, ic.where_in_index(want, d))


def test_banded_frames_silence_contexts(api, oracle):
    """The content of test_index_large_gpu.py does what it is there for, measured on felics_index_build's rows alone: between two
    loud intervals at least MEASURE_MIN contexts hold one non-zero row over the whole gap (the state of their first later record),
    and as many go from a non-zero row to zeros behind the last loud interval.  A frame on which these were 0 would let an index
    writer pass that never carries a find across its chunks of 64 intervals.  Prints the counts."""
    seen = 0
    for w, h, seg_tiles, plans in ic.LARGE:
        for rgb in (0, 1):
            for plan in plans:
                stream = oracle.compress(ic.banded(w, h, rgb, plan))
                for st in seg_tiles:
                    rows = ic.state_rows(api.index_build(stream, st * ic.GRANULE))
                    assert not rows[:, 0].any()  # segment 0 starts on a zeroed table
                    todo = ic.measures(w, h, st, plan)
                    for what, least in todo:
                        got = ic.measure(rows, what)
                        print("%d x %d %s seg_tiles %d loud %s: %s = %d" % (w, h, "RGB" if rgb else "gray", st, plan, what, got))
                        assert got >= least, (w, h, rgb, st, plan, what, got)
                        seen += 1
                    assert todo or tuple(plan) == (0, 8)  # (everything loud in interval 0: only beside the other plan of its shape)
    assert seen == 2 * 20


# ---- refusals ----------------------------------------------------------------------------------------------------------------

def _raw_decode(api, stream, index, cap):
    """felics_decompress_indexed into a buffer with guard bytes: (code, the buffer)"""
    s = np.frombuffer(stream, np.uint8)
    i = np.frombuffer(index, np.uint8)
    out = np.full(cap + 64, 0xA5, np.uint8)
    rc = api.lib().felics_decompress_indexed(s.ctypes.data, len(s), i.ctypes.data if len(i) else None, len(i), out.ctypes.data + 32, cap, None)
    assert (out[:32] == 0xA5).all() and (out[32 + cap:] == 0xA5).all()
    return rc, out[32:32 + cap]


def test_refusals(api, cases, oracle):
    for rgb in (0, 1):
        img, stream = cases[(100, 100, rgb)][0]
        index = api.index_build(stream, 4096)
        rc, px = _raw_decode(api, stream, index, img.size)
        assert rc == 0 and (px.reshape(img.shape) == img).all()
        bad = ic.corruptions(index)
        assert ("co_300" in bad) == bool(rgb)
        for name, idx in bad.items():
            rc, _ = _raw_decode(api, stream, idx, img.size)
            assert rc == ic.E_INVALID_INDEX, (rgb, name, rc)
        # the index of another stream of the same shape: refused where the lengths differ, and never a crash
        other = cases[(100, 100, rgb)][1][1]
        if len(other) != len(stream):
            assert _raw_decode(api, stream, api.index_build(other, 4096), img.size)[0] == ic.E_INVALID_INDEX
        # a short output buffer, a bad segment size
        assert _raw_decode(api, stream, index, img.size - 1)[0] == -8
        need = C.c_size_t(0)
        s = np.frombuffer(stream, np.uint8)
        assert api.lib().felics_index_build(s.ctypes.data, len(s), 6000, None, 0, C.byref(need)) == -11
        assert api.lib().felics_index_build(s.ctypes.data, len(s), 4096, None, 0, C.byref(need)) == -8 and need.value == len(index)
        # bytes behind the last code: not a stream an index can describe
        longer = np.frombuffer(stream + b"\0", np.uint8)
        buf = np.zeros(len(index), np.uint8)
        assert api.lib().felics_index_build(longer.ctypes.data, len(longer), 4096, buf.ctypes.data, len(buf), C.byref(need)) == -11
    # 16-bit streams have no index
    s16 = oracle.compress(np.arange(70 * 70, dtype=np.uint16).reshape(70, 70))
    s = np.frombuffer(s16, np.uint8)
    need = C.c_size_t(0)
    assert api.lib().felics_index_build(s.ctypes.data, len(s), 4096, None, 0, C.byref(need)) == ic.E_UNSUPPORTED
    rc, _ = _raw_decode(api, s16, api.index_build(cases[(64, 65, 0)][0][1], 4096), 70 * 70 * 2)
    assert rc == ic.E_UNSUPPORTED
    # a bad stream gives its own error
    _, good = cases[(64, 65, 0)][0]
    s = np.frombuffer(good[:-5], np.uint8)
    buf = np.zeros(1 << 16, np.uint8)
    assert api.lib().felics_index_build(s.ctypes.data, len(s), 4096, buf.ctypes.data, len(buf), C.byref(need)) == -1
    with pytest.raises(api.DecompressionError):
        api.index_build(b"NOPE" + good[4:], 4096)


# ---- sanitizers --------------------------------------------------------------------------------------------------------------

def test_index_fuzz_under_sanitizers(tmp_path, api, cases):
    r = subprocess.run(["make", "-C", CSRC, "asan"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    d = tmp_path / "corpus"
    d.mkdir()
    rng = np.random.default_rng(99)
    n = headers = 0

    def put(stream, index=None):
        nonlocal n, headers
        (d / ("%04d.felics" % n)).write_bytes(stream)
        if index is not None:
            (d / ("%04d.felics.idx" % n)).write_bytes(index)
        n += 1
        try:  # a stream with a valid header has the region calls' plan made for its shape
            api.read_header(io.BytesIO(stream))
            headers += 1
        except api.DecompressionError:
            pass

    seeds = [cases[k][0][1] for k in ((64, 65, 0), (100, 100, 1), (1, 9000, 0), (4097, 1, 1), (4096, 3, 0), (0, 5, 1), (2048, 5, 1))]
    seeds.append(open(os.path.join(GOLDEN, "6.1.01.tiff.felics"), "rb").read())
    seeds.append(open(os.path.join(GOLDEN, "lena_color_256.tif.felics"), "rb").read())
    for stream in seeds:
        index = api.index_build(stream, 4096)
        put(stream, index)
        for cut in (0, 13, 14, 22, len(stream) // 2, len(stream) - 1):
            put(stream[:cut], index)
        for _ in range(12):  # a good index beside a mutated stream
            b = bytearray(stream)
            for _ in range(int(rng.integers(1, 4))):
                b[int(rng.integers(0, 14 if rng.random() < 0.2 else len(b)))] ^= 1 << int(rng.integers(0, 8))
            put(bytes(b), index)
        for _ in range(12):  # a mutated index beside a good stream
            b = bytearray(index)
            for _ in range(int(rng.integers(1, 4))):
                b[int(rng.integers(0, min(72, len(b)) if rng.random() < 0.5 else len(b)))] ^= 1 << int(rng.integers(0, 8))
            put(stream, bytes(b))
        if len(index) > 64:
            for name, idx in ic.corruptions(index).items() if ic.Layout(index).k >= 2 else ():
                put(stream, idx)
        put(stream[:6] + struct.pack(">II", 65535, 65535) + stream[14:200], index)  # forged dimensions
        put(stream[:22] + b"\xff" * 4096, index)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:allocator_may_return_null=1:max_allocation_size_mb=2048",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([FUZZ, str(d)], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-6000:])
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-6000:]
    assert "index_fuzz: %d files" % n in r.stdout
    assert 0 < headers < n and "index_fuzz: region plans of %d streams with a valid header" % headers in r.stdout, r.stdout[-2000:]
