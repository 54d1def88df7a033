"""Restart index of 16-bit streams, host side (no GPU): felics_index16_size_max, felics_index16_build and felics_decompress_indexed16
against the original pixels, felics_decompress and a builder and a segment decoder written here from the format's description
alone; the proof that every case of index16_common.py reaches the edge it is there for; the refusals; index_fuzz --index16 under
sanitizers."""
import ctypes as C
import glob
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import index16_common as ic

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
CSRC = os.path.join(ROOT, "felics_amd", "csrc")
FUZZ = os.path.join(ROOT, "felics_amd", "_build", "asan", "index_fuzz")

NEW_SYMBOLS = ("felics_index_wide_size_max", "felics_index_wide_build", "felics_decompress_indexed_wide", "felics_decompress_batch_device_indexed_wide",
               "felics_get_index_wide_stats")
SLOTS = 512  # rows the kernel's LDS cache holds, direct-mapped by context % SLOTS


@pytest.fixture(scope="module")
def api():
    from felics_amd import api as a

    a.lib()
    return a


@pytest.fixture(scope="module")
def cases(oracle):
    """name -> (frame, oracle stream): computed once, read by every test"""
    return {name: (img, oracle.compress(img)) for name, (img, _) in ic.cases().items()}


@pytest.fixture(scope="module")
def models(cases):
    """name -> the model's decode of the stream (every case: the largest has 32 256 pixels)"""
    return {name: _model_decode(stream) for name, (_, stream) in cases.items()}


def test_abi_surface(api):
    L = api.lib()
    for name in NEW_SYMBOLS:
        assert hasattr(L, name) and name in api.EXPORTS, name
    for name in ("index16_size_max", "index16_build", "decompress_indexed16"):
        assert callable(getattr(api, name))
    assert callable(api.Encoder.decompress_batch_device_indexed16) and callable(api.Encoder.index16_stats)
    st = api._CIndex16Stats(7, 7, 7, 7, 7)
    assert C.sizeof(st) == 40
    assert L.felics_get_index_wide_stats(None, C.byref(st), C.sizeof(st)) == -11 and (st.streams, st.table_bytes) == (7, 7)
    assert L.felics_decompress_batch_device_indexed_wide(None, 1, None, None, None, None, None, None, None, 0, None, None) == -11


# ---- the format, from its description: a plain decoder that keeps what a builder needs, a builder, a segment decoder -----------------

class _Bits:
    """MSB-first reads; unary runs of any length"""

    def __init__(self, data):
        self.total, self.pos = 8 * len(data), 0
        self.data = bytes(data) + bytes(8)

    def get(self, n):
        assert self.pos + n <= self.total
        at, skip = self.pos >> 3, self.pos & 7
        assert skip + n <= 64
        self.pos += n
        return (int.from_bytes(self.data[at:at + 8], "big") >> (64 - skip - n)) & ((1 << n) - 1) if n else 0

    def unary(self):
        q = 0
        while True:
            at, skip = self.pos >> 3, self.pos & 7
            word = (int.from_bytes(self.data[at:at + 8], "big") << skip) & ((1 << 64) - 1) | ((1 << skip) - 1)
            ones = 64 - (word ^ ((1 << 64) - 1)).bit_length()  # leading ones of the 64 - skip bits at the position
            ones = min(ones, 64 - skip)
            if ones < 64 - skip:
                self.pos += ones + 1
                assert self.pos <= self.total
                return q + ones
            q += ones
            self.pos += ones
            assert self.pos < self.total


def _neighbours(p, i, x, y, w):
    if x > 0 and y > 0:
        return p[i - 1], p[i - w]
    if y == 0:
        return p[i - 1], p[i - 2]
    if y >= 2:
        return p[i - w], p[i - 2 * w]
    return p[i - w], p[i - w + 1]


def _walk(br, p, table, w, i0, i1, on_event=None):
    """decompress_channel's loop over pixels [i0, i1) of plane p (a list; the samples in front are in it), table: context -> fifteen
    counters (absent = zeros).  on_event(i, ctx, e, k, halved)."""
    x, y = (i0 % w, i0 // w) if w else (0, 0)
    for i in range(i0, i1):
        a, b = _neighbours(p, i, x, y, w)
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
            row = table.setdefault(ctx, [0] * 15)
            k = max(range(15), key=lambda kk: (-row[kk], kk))  # smallest counter, ties to the largest k
            e = (br.unary() << k) + br.get(k)
            for kk in range(15):
                row[kk] += (e >> kk) + 1 + kk
            halved = min(row) > 1024
            if halved:
                row[:] = [v >> 1 for v in row]
            if on_event:
                on_event(i, ctx, e, k, halved)
            p[i] = hi + e + 1 if above else lo - e - 1
        x += 1
        if x == w:
            x, y = 0, y + 1


def _model_decode(stream):
    """Decodes a 16-bit stream once: per plane the samples, the events (pixel, context, operand, k, halved), the bit position and a
    copy of the table at every multiple of GRANULE, the plane's first and last bit."""
    color, depth = stream[4], stream[5]
    assert depth == 1
    w, h = struct.unpack(">II", stream[6:14])
    npix, planes = w * h, (3 if color else 1)
    br = _Bits(stream)
    br.pos = 112
    out = []
    for _ in range(planes):
        start = br.pos
        raw = [br.get(32), br.get(32)]
        raw = [r - (1 << 32) if r >> 31 else r for r in raw]
        p, table, events, snaps = [0] * npix, {}, [], []
        p[:2] = raw[:npix]
        for g0 in range(0, npix, ic.GRANULE):
            snaps.append((start if g0 == 0 else br.pos, {c: r[:] for c, r in table.items()}))
            _walk(br, p, table, w, max(g0, 2), min(npix, g0 + ic.GRANULE), lambda *ev: events.append(ev))
        out.append({"p": p, "events": events, "snaps": snaps, "start": start, "end": br.pos})
    assert (br.pos + 7) // 8 == len(stream)
    return {"color": color, "w": w, "h": h, "planes": out}


def _model_index(model, seg):
    """the index of §1 from the model's decode"""
    color, w, h, pl = model["color"], model["w"], model["h"], model["planes"]
    planes, sb, fmt = (3, 4, "<i") if color else (1, 2, "<H")
    npix = w * h
    k = (npix + seg - 1) // seg
    win_base = ic.up(64 + 32 * planes * k, 64)
    win_bytes = ic.up(2 * w * sb, 16)
    rows_base = ic.up(win_base + planes * k * win_bytes, 64)
    directory, windows, rows = bytearray(), bytearray(), bytearray()
    for c in range(planes):
        last = {}
        for i, ctx, *_ in pl[c]["events"]:
            last[ctx] = i
        for j in range(k):
            p0 = j * seg
            bit, table = pl[c]["snaps"][p0 // ic.GRANULE]
            # canonical form: an event in front of p0 (it is in the table) and one at or behind it
            live = sorted(ctx for ctx in table if j > 0 and last[ctx] >= p0)
            directory += struct.pack("<QQI", bit, rows_base + len(rows), len(live)) + bytes(12)
            for ctx in live:
                rows += struct.pack("<15I", *table[ctx]) + struct.pack("<I", ctx)
            win = b"".join(struct.pack(fmt, pl[c]["p"][t] if t >= 0 else 0) for t in range(p0 - 2 * w, p0))
            windows += win + bytes(win_bytes - len(win))
    ends = [q["end"] for q in pl] + [0, 0]
    head = b"FLCX" + struct.pack("<HBBIIII", 2, color, 1, w, h, seg, k) + struct.pack("<3Q", *ends[:3]) + struct.pack("<Q", rows_base + len(rows)) + bytes(8)
    out = head + bytes(directory)
    out += bytes(win_base - len(out)) + bytes(windows)
    out += bytes(rows_base - len(out)) + bytes(rows)
    return out


def _model_segment(stream, index, lay, c, j, on_event=None):
    """segment (c, j) decoded from its checkpoint alone: (its samples, the bit position it ends on)"""
    w, npix = lay.w, lay.w * lay.h
    bit, _, _ = lay.get(c, j)
    ctxs, counters = ic.rows_of(index, lay, c, j)
    table = {int(ctx): [int(v) for v in row] for ctx, row in zip(ctxs, counters)}
    p0, p1 = j * lay.seg, min(npix, (j + 1) * lay.seg)
    fmt = "<%di" % (2 * w) if lay.color else "<%dH" % (2 * w)
    win = struct.unpack_from(fmt, index, lay.window(c, j))
    p = [None] * npix
    for t in range(max(p0 - 2 * w, 0), p0):
        p[t] = win[t - (p0 - 2 * w)]
    br = _Bits(stream)
    br.pos = bit
    if j == 0:
        raw = [br.get(32), br.get(32)]
        p[:2] = [r - (1 << 32) if r >> 31 else r for r in raw][:npix]
    _walk(br, p, table, w, max(p0, 2), p1, on_event)
    return p[p0:p1], br.pos


def test_index_bytes_equal_the_model(api, cases, models):
    """felics_index_wide_build's bytes against the model's, every case at every segment size"""
    for name, (img, stream) in cases.items():
        for seg in ic.SEGMENTS:
            got, want = api.index16_build(stream, seg), _model_index(models[name], seg)
            d = next((i for i in range(min(len(got), len(want))) if got[i] != want[i]), None)
            assert len(got) == len(want) and d is None, (name, seg, len(got), len(want), d)


def test_model_decoder_from_every_checkpoint(api, cases):
    """the model's segment decoder, started at every checkpoint of felics_index16_build's index, reproduces the planes the oracle
    coded and ends on the next checkpoint's bit"""
    for name, (img, stream) in cases.items():
        index = api.index16_build(stream, 4096)
        lay = ic.Layout16(index)
        want = ic.planes_of(img)
        for c in range(lay.planes):
            for j in range(lay.k):
                got, end = _model_segment(stream, index, lay, c, j)
                assert got == [int(v) for v in want[c][j * 4096:(j + 1) * 4096]], (name, c, j)
                assert end == (lay.get(c, j + 1)[0] if j + 1 < lay.k else lay.plane_end[c]), (name, c, j)


# ---- round trips -----------------------------------------------------------------------------------------------------------------

def _two_call(api, stream, seg):
    """the two-call size pattern, by hand: (index, the size the first call named)"""
    L = api.lib()
    s = np.frombuffer(stream, np.uint8)
    need = C.c_size_t(0)
    assert L.felics_index_wide_build(s.ctypes.data, len(s), seg, None, 0, C.byref(need)) == -8
    size = need.value
    buf = np.full(size + 64, 0xA5, np.uint8)
    assert L.felics_index_wide_build(s.ctypes.data, len(s), seg, buf.ctypes.data, size - 1, C.byref(need)) == -8 and need.value == size
    assert (buf == 0xA5).all()  # a short buffer is not written to
    assert L.felics_index_wide_build(s.ctypes.data, len(s), seg, buf.ctypes.data, size, C.byref(need)) == 0 and need.value == size
    assert (buf[size:] == 0xA5).all()
    return buf[:size].tobytes(), size


def test_roundtrip_all_cases(api, cases):
    for name, (img, stream) in cases.items():
        plain = api.decompress_bytes(stream)
        h, w = img.shape[:2]
        for seg in ic.SEGMENTS:
            index, size = _two_call(api, stream, seg)
            assert index == api.index16_build(stream, seg)
            assert 64 <= size <= api.index16_size_max(w, h, img.ndim == 3, seg) and size % 64 == 0, (name, seg, size)
            lay = ic.Layout16(index)
            assert (lay.version, lay.depth, lay.k, lay.total) == (2, 1, (w * h + seg - 1) // seg, size)
            out = api.decompress_indexed16(stream, index)
            assert out.dtype == np.uint16 and out.shape == img.shape and (out == img).all() and (out == plain).all(), (name, seg)


def test_size_max(api):
    assert api.index16_size_max(0, 5, 0, 4096) == 64 and api.index16_size_max(5, 0, 1, 4096) == 64
    for bad in (0, 4095, 6000):
        assert api.index16_size_max(64, 64, 0, bad) == 0
    assert api.index16_size_max(65536, 65536, 0, 4096) == 0 and api.index16_size_max(64, 64, 2, 4096) == 0
    # 64 x 130 gray at 4096: K = 3, rows <= min(p0 - 2, npix - p0, 65 536) = 4094 and 128
    assert api.index16_size_max(64, 130, 0, 4096) == ic.up(ic.up(64 + 96, 64) + 3 * 256, 64) + 64 * (4094 + 128)
    # the figure of the issue: a dense state per checkpoint would be 7.9 MB
    assert 131071 * 15 * 4 == 7864260


def test_roundtrip_golden_16bit(api):
    """the committed 16-bit streams: aerial.tiff, heightmap.tiff and the gray16 originals of tests/golden/suite/, at 65 536"""
    from PIL import Image

    paths = [os.path.join(GOLDEN, n) for n in ("aerial.tiff.felics", "heightmap.tiff.felics")]
    paths += sorted(glob.glob(os.path.join(GOLDEN, "suite", "*.felics")))
    seen = 0
    for path in paths:
        stream = open(path, "rb").read()
        if stream[5] != 1:
            continue
        img = np.array(Image.open(path[:-len(".felics")]))
        index = api.index16_build(stream, 65536)
        assert len(index) <= api.index16_size_max(img.shape[1], img.shape[0], img.ndim == 3, 65536)
        out = api.decompress_indexed16(stream, index)
        assert out.dtype == img.dtype and out.shape == img.shape and (out == img).all(), path
        seen += 1
    assert seen >= 3


# ---- every case reaches its edge -----------------------------------------------------------------------------------------------

def _segment_events(stream, index, lay, c, j):
    ev = []
    _model_segment(stream, index, lay, c, j, lambda *e: ev.append(e))
    return ev


def test_cases_reach_their_edges(api, cases):
    idx = {name: api.index16_build(stream, 4096) for name, (_, stream) in cases.items()}
    lay = {name: ic.Layout16(b) for name, b in idx.items()}
    # a checkpoint behind segment 0 with no rows; row counts of every residue modulo 4; more than 512 rows
    flat = lay["flat"]
    assert flat.k == 3 and flat.n_rows() == [0, 0, 0]
    counts = [n for name in ("noise12", "noise11", "noise10", "noise9", "alias", "banded") for n in lay[name].n_rows() if n]
    print("row counts:", counts)
    assert {n % 4 for n in counts} == {0, 1, 2, 3} and max(lay["noise12"].n_rows()) > SLOTS
    # segment 0 never has rows
    assert all(L.get(c, 0)[2] == 0 for L in lay.values() for c in range(L.planes) if L.k)
    # a chroma checkpoint holding a context >= 65 536
    ch = lay["chroma"]
    top = [int(ic.rows_of(idx["chroma"], ch, c, 1)[0].max(initial=0)) for c in (1, 2)]
    print("largest chroma contexts:", top)
    assert ch.k == 2 and max(top) >= 65536 and int(ic.rows_of(idx["chroma"], ch, 0, 1)[0].max(initial=0)) < 65536
    # alias: two contexts of one cache slot, both with rows, taking turns; a row first used behind >= 512 events of other contexts; a
    # halving of a loaded row
    al, stream = lay["alias"], cases["alias"][1]
    ctxs = set(int(v) for v in ic.rows_of(idx["alias"], al, 0, 1)[0])
    ev = _segment_events(stream, idx["alias"], al, 0, 1)
    order = [e[1] for e in ev]
    turns, late, halved = 0, 0, 0
    for a in ctxs:
        if a not in order:  # (its next event is in segment 2)
            continue
        first = order.index(a)
        late = max(late, sum(1 for o in order[:first] if o != a))
        for b in ctxs:
            if a < b and a % SLOTS == b % SLOTS:
                seq = [o for o in order if o in (a, b)]
                turns = max(turns, sum(1 for u, v in zip(seq, seq[1:]) if u != v))
    halved = sum(1 for e in ev if e[4] and e[1] in ctxs)
    print("alias: turns %d, events in front of a row's first use %d, halvings of loaded rows %d" % (turns, late, halved))
    assert turns >= 2 and late >= SLOTS and halved >= 1
    # spikes: Rice codes of more than 32 and of about 65 000 bits inside segment 1, from loaded rows
    sp, stream = lay["spikes"], cases["spikes"][1]
    rows1 = set(int(v) for v in ic.rows_of(idx["spikes"], sp, 0, 1)[0])
    bits = sorted((e[2] >> e[3]) + 1 + e[3] for e in _segment_events(stream, idx["spikes"], sp, 0, 1) if e[1] in rows1)
    print("spikes: longest Rice codes", bits[-3:])
    assert bits[-1] >= 65000 and any(32 < b < 1000 for b in bits)
    # banded: the later checkpoints hold fewer rows than the earlier ones, down to none
    bd = lay["banded"].n_rows()
    print("banded rows:", bd)
    assert bd[1] > SLOTS and bd[1] > bd[2] and bd[-1] == 0
    # the shapes: where p0 stands
    assert lay["100x100"].k == 3 and 4096 % 100 == 96 and lay["4096x3"].k == 3 and lay["4100x3"].k == 4 and lay["64x64"].k == 1
    assert lay["64x65"].k == 2 and lay["1x5000"].k == 2 and lay["empty_0x5"].k == 0 and len(idx["empty_0x5"]) == 64
    assert lay["16128x2"].w == 16128


# ---- refusals ----------------------------------------------------------------------------------------------------------------

def _raw_decode(api, stream, index, cap):
    """felics_decompress_indexed_wide into a buffer with guard bytes: (code, the buffer)"""
    s = np.frombuffer(stream, np.uint8)
    i = np.frombuffer(index, np.uint8)
    out = np.full(cap + 64, 0xA5, np.uint8)
    rc = api.lib().felics_decompress_indexed_wide(s.ctypes.data, len(s), i.ctypes.data if len(i) else None, len(i), out.ctypes.data + 32, cap, None)
    assert (out[:32] == 0xA5).all() and (out[32 + cap:] == 0xA5).all()
    return rc, out[32:32 + cap]


def test_refusals(api, cases, oracle):
    for name in ("100x100", "100x100_rgb"):
        img, stream = cases[name]
        index = api.index16_build(stream, 4096)
        rc, px = _raw_decode(api, stream, index, img.nbytes)
        assert rc == 0 and (px.view(np.uint16).reshape(img.shape) == img).all()
        bad = ic.corruptions(index)
        assert ("co_sample_70000" in bad) == (img.ndim == 3) and len(bad) >= 23
        for what, b in bad.items():
            rc, _ = _raw_decode(api, stream, b, img.nbytes)
            assert rc == ic.E_INVALID_INDEX, (name, what, rc)
        assert _raw_decode(api, stream, index, img.nbytes - 1)[0] == -8
        need = C.c_size_t(0)
        s = np.frombuffer(stream, np.uint8)
        assert api.lib().felics_index_wide_build(s.ctypes.data, len(s), 6000, None, 0, C.byref(need)) == -11
        longer = np.frombuffer(stream + b"\0", np.uint8)  # bytes behind the last code
        buf = np.zeros(len(index), np.uint8)
        assert api.lib().felics_index_wide_build(longer.ctypes.data, len(longer), 4096, buf.ctypes.data, len(buf), C.byref(need)) == -11
    # a version-1 index of an 8-bit stream of the same shape beside a 16-bit stream; an 8-bit stream
    img, stream = cases["100x100"]
    s8 = oracle.compress((img >> 8).astype(np.uint8))
    v1 = api.index_build(s8, 4096)
    assert _raw_decode(api, stream, v1, img.nbytes)[0] == ic.E_INVALID_INDEX
    assert _raw_decode(api, s8, api.index16_build(stream, 4096), img.nbytes)[0] == ic.E_UNSUPPORTED
    need = C.c_size_t(0)
    s = np.frombuffer(s8, np.uint8)
    assert api.lib().felics_index_wide_build(s.ctypes.data, len(s), 4096, None, 0, C.byref(need)) == ic.E_UNSUPPORTED
    with pytest.raises((api.FelicsError, api.DecompressionError)):
        api.index16_build(s8, 4096)
    # a bad stream gives its own error
    s = np.frombuffer(stream[:-5], np.uint8)
    buf = np.zeros(1 << 16, np.uint8)
    assert api.lib().felics_index_wide_build(s.ctypes.data, len(s), 4096, buf.ctypes.data, len(buf), C.byref(need)) == -1
    with pytest.raises(api.DecompressionError):
        api.index16_build(b"NOPE" + stream[4:], 4096)
    # the version-1 calls keep refusing 16-bit streams
    assert api.index_size(100, 100, 0, 1, 4096) == 0
    assert api.lib().felics_index_build(np.frombuffer(stream, np.uint8).ctypes.data, len(stream), 4096, None, 0, C.byref(need)) == ic.E_UNSUPPORTED


# ---- sanitizers --------------------------------------------------------------------------------------------------------------

def test_index16_fuzz_under_sanitizers(tmp_path, api, cases):
    r = subprocess.run(["make", "-C", CSRC, "asan"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    d = tmp_path / "corpus"
    d.mkdir()
    rng = np.random.default_rng(77)
    n = 0

    def put(stream, index=None):
        nonlocal n
        (d / ("%04d.felics" % n)).write_bytes(stream)
        if index is not None:
            (d / ("%04d.felics.idx" % n)).write_bytes(index)
        n += 1

    for name in ("100x100_rgb", "1x5000", "empty_rgb_5x0", "chroma", "alias", "spikes"):
        stream = cases[name][1]
        index = api.index16_build(stream, 4096)
        put(stream, index)
        for cut in (0, 13, 14, 22, len(stream) // 2, len(stream) - 1):
            put(stream[:cut], index)
        for _ in range(6):  # a good index beside a mutated stream
            b = bytearray(stream)
            for _ in range(int(rng.integers(1, 4))):
                b[int(rng.integers(0, 14 if rng.random() < 0.2 else len(b)))] ^= 1 << int(rng.integers(0, 8))
            put(bytes(b), index)
        for _ in range(6):  # a mutated index beside a good stream
            b = bytearray(index)
            for _ in range(int(rng.integers(1, 4))):
                b[int(rng.integers(0, min(128, len(b)) if rng.random() < 0.5 else len(b)))] ^= 1 << int(rng.integers(0, 8))
            put(stream, bytes(b))
        lay = ic.Layout16(index)
        if lay.k >= 2 and lay.get(0, 1)[2] >= 2:
            for b in ic.corruptions(index).values():
                put(stream, b)
        put(stream[:6] + struct.pack(">II", 65535, 65535) + stream[14:200], index)  # forged dimensions
        put(stream[:22] + b"\xff" * 4096, index)
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0:allocator_may_return_null=1:max_allocation_size_mb=2048",
               UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([FUZZ, "--index16", str(d)], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-6000:])
    assert "AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-6000:]
    assert "index_fuzz --index16: %d files" % n in r.stdout
