"""What the tests of the 16-bit restart index share (test_index16_cpu.py, test_index16_gpu.py): the cases -- each a frame plus the edge
it is meant to reach --, the layout of a version-2 index written out from the format's description in include/felics.h, and the
corruptions both files refuse.  That a case reaches its edge is shown in test_index16_cpu.py, from the built index and the model."""
import struct

import numpy as np

E_UNSUPPORTED = -10
E_INVALID_INDEX = -12
GRANULE = 4096
SEGMENTS = (4096, 8192, 3 * 4096)
ROW = 64


def noise(w, h, rgb, bits, seed):
    """uniform noise of `bits` bits: contexts repeat (a few thousand of them), so checkpoints hold hundreds of rows"""
    rng = np.random.default_rng(seed)
    return rng.integers(0, 1 << bits, size=(h, w, 3) if rgb else (h, w), dtype=np.uint16)


def ramp(w, h, rgb):
    smooth = ((np.add.outer(np.arange(h), np.arange(w)) * 37) % 65536).astype(np.uint16)
    return np.stack([smooth, smooth[::-1], 65535 - smooth], -1).copy() if rgb else smooth


def chosen(w, h, values, seed):
    """every sample one of a few values: a handful of contexts with many events each"""
    rng = np.random.default_rng(seed)
    return np.array(values, np.uint16)[rng.integers(0, len(values), size=(h, w))]


# the values of `chosen` frames whose contexts 100 and 612 are equal modulo 512 (the LDS cache's slots) and both have events
ALIAS = (30500, 31000, 31100, 31612, 32000)


def _alias():
    """64 x 130: rows 0-31 ALIAS content, rows 32-95 noise in steps of 8 (contexts that are multiples of 8: none of ALIAS's), rows 96
    on ALIAS content again.  At p0 = 4096 (row 64) ALIAS's contexts have rows; their first event of segment 1 comes behind 2048
    pixels of noise, far more than 512 events of other contexts, and from there contexts 100 and 612 take turns in one cache slot;
    with some 200 events each they are halved inside the segment."""
    f = chosen(64, 130, ALIAS, 11)
    f[32:96] = noise(64, 64, 0, 9, 12) * 8
    return f


def _spikes():
    """64 x 130 of samples 0 / 1 (context 0 and 1 learn k = 0) with two spikes in segment 1: +45 (a Rice code of more than 32 bits) and
    full scale (a unary run of about 65 000 bits)."""
    f = chosen(64, 130, (0, 1), 21)
    f[80, 20] = 45
    f[100, 40] = 65535
    return f


def _chroma():
    """33 x 130 RGB16, R and B from four values at both ends of the range: Co differences beyond 65 535 with samples outside them"""
    rng = np.random.default_rng(31)
    ends = np.array((0, 1000, 64535, 65535), np.uint16)
    f = np.zeros((130, 33, 3), np.uint16)
    f[..., 0] = ends[rng.integers(0, 4, (130, 33))]
    f[..., 1] = 32768
    f[..., 2] = ends[rng.integers(0, 4, (130, 33))]
    return f


def _banded():
    """64 x 260: loud top (12-bit noise, rows 0-129), flat bottom: the later checkpoints hold fewer rows than the earlier ones"""
    f = np.full((260, 64), 2000, np.uint16)
    f[:130] = noise(64, 130, 0, 12, 41)
    return f


def _rgb_noise_top(w, h):
    f = noise(w, h, 1, 10, 51)
    f[h // 2:] = ramp(w, h, 1)[h // 2:]
    return f


def cases():
    """name -> (frame, what it is for); built once per test module"""
    out = {
        "empty_0x5": (np.zeros((5, 0), np.uint16), "K = 0: the header alone"),
        "empty_rgb_5x0": (np.zeros((0, 5, 3), np.uint16), "K = 0, three planes"),
        "1x1": (np.full((1, 1), 777, np.uint16), "one raw sample"),
        "2x1": (np.array([[5, 65535]], np.uint16), "the two raw samples and nothing else"),
        "1x5000": (noise(1, 5000, 0, 8, 1), "W = 1: the first-column rule everywhere, a window of two samples"),
        "64x64": (noise(64, 64, 0, 10, 2), "K = 1"),
        "64x65": (noise(64, 65, 0, 10, 3), "a last segment of 64 pixels"),
        "100x100": (noise(100, 100, 0, 10, 4), "p0 = 4096 stands at x0 = 96, mid-block"),
        "100x100_rgb": (noise(100, 100, 1, 10, 5), "the same with three planes"),
        "4096x3": (noise(4096, 3, 0, 10, 6), "x0 = 0 at every checkpoint: the 2 W-back rule"),
        "4100x3": (noise(4100, 3, 0, 10, 7), "W > segment: segments start mid-row"),
        "33x130_rgb": (_rgb_noise_top(33, 130), "RGB16, an odd width"),
        "16128x2": (noise(16128, 2, 0, 10, 8), "the widest row the LDS takes"),
        "ramp_100x100_rgb": (ramp(100, 100, 1), "smooth content: few events, few rows"),
        "flat": (np.full((130, 64), 1234, np.uint16), "no event at all: checkpoints with n_rows = 0"),
        "noise12": (noise(64, 130, 0, 12, 9), "more than 512 rows in a checkpoint; row counts of every residue modulo 4 with the cases below"),
        "noise11": (noise(64, 130, 0, 11, 10), "row counts of other residues"),
        "noise10": (noise(64, 130, 0, 10, 13), "row counts of other residues"),
        "noise9": (noise(64, 130, 0, 9, 14), "row counts of other residues"),
        "chroma": (_chroma(), "a chroma checkpoint holding a context >= 65 536"),
        "alias": (_alias(), "two contexts of one cache slot taking turns; a row first used behind 512 other events; a halving of a loaded row"),
        "spikes": (_spikes(), "Rice codes of more than 32 and of about 65 000 bits inside segment 1"),
        "banded": (_banded(), "later checkpoints hold fewer rows than earlier ones: the dropping rule"),
    }
    return out


def planes_of(img):
    """The planes the encoder codes: the frame itself, or Y / Co / Cg of an RGB frame (the division truncates towards zero)."""
    if img.ndim == 2:
        return [img.astype(np.int64).ravel()]
    r, g, b = (img[..., i].astype(np.int64).ravel() for i in range(3))
    co = r - b
    t = b + np.trunc(co / 2).astype(np.int64)
    cg = g - t
    return [t + np.trunc(cg / 2).astype(np.int64), co, cg]


def up(v, m):
    return (v + m - 1) // m * m


class Layout16:
    """where the fields of a version-2 index lie, from the header alone; the directory read out"""

    def __init__(self, index):
        assert index[:4] == b"FLCX"
        self.version, self.color, self.depth, self.w, self.h, self.seg, self.k = struct.unpack_from("<HBBIIII", index, 4)
        self.plane_end = struct.unpack_from("<3Q", index, 24)
        self.total = struct.unpack_from("<Q", index, 48)[0]
        self.planes, self.sample = (3, 4) if self.color else (1, 2)
        self.win_base = up(64 + 32 * self.planes * self.k, 64)
        self.win_bytes = up(2 * self.w * self.sample, 16)
        self.rows_base = up(self.win_base + self.planes * self.k * self.win_bytes, 64)
        self.entries = [struct.unpack_from("<QQI", index, self.entry(c, j)) for c in range(self.planes) for j in range(self.k)]

    def entry(self, c, j):
        return 64 + 32 * (c * self.k + j)

    def get(self, c, j):
        """(bit_offset, rows_off, n_rows)"""
        return self.entries[c * self.k + j]

    def window(self, c, j):
        return self.win_base + (c * self.k + j) * self.win_bytes

    def n_rows(self):
        return [e[2] for e in self.entries]


def rows_of(index, lay, c, j):
    """checkpoint (c, j)'s rows: (contexts, counters n x 15)"""
    _, off, n = lay.get(c, j)
    a = np.frombuffer(index, "<u4", n * 16, off).reshape(n, 16)
    return a[:, 15].astype(np.int64), a[:, :15].astype(np.int64)


def corruptions(index):
    """name -> corrupted copy of a valid version-2 index with K >= 2 whose checkpoint (0, 1) holds at least two rows (RGB for the chroma
    cases): each must be refused with E_INVALID_INDEX.  Every one is caught by a check the code makes BEFORE the read it guards."""
    lay = Layout16(index)
    assert lay.k >= 2 and lay.get(0, 1)[2] >= 2

    def patched(pos, data):
        b = bytearray(index)
        b[pos:pos + len(data)] = data
        return bytes(b)

    bit1, off1, n1 = lay.get(0, 1)
    e1 = lay.entry(0, 1)
    ctx0, ctx1 = (struct.unpack_from("<I", index, off1 + 64 * r + 60)[0] for r in (0, 1))
    last = lay.entry(lay.planes - 1, lay.k - 1)
    fmt = "<i" if lay.color else "<H"
    out = {
        "magic": patched(0, b"FLCS"),
        "version_1": patched(4, struct.pack("<H", 1)),
        "depth_0": patched(7, b"\0"),
        "width": patched(8, struct.pack("<I", lay.w + 1)),
        "height": patched(12, struct.pack("<I", lay.h + 1)),
        "segment_pixels": patched(16, struct.pack("<I", lay.seg + GRANULE)),
        "K": patched(20, struct.pack("<I", lay.k + 1)),
        "total_plus_64": patched(48, struct.pack("<Q", lay.total + 64)),
        "total_minus_64": patched(48, struct.pack("<Q", lay.total - 64)),
        "reserved": patched(63, b"\1"),
        "bit_offset_plus_1": patched(e1, struct.pack("<Q", bit1 + 1)),  # the end check of segment (0, 0)
        "bit_offset_minus_1": patched(e1, struct.pack("<Q", bit1 - 1)),
        "rows_off_plus_64": patched(e1 + 8, struct.pack("<Q", off1 + 64)),
        "rows_off_misaligned": patched(e1 + 8, struct.pack("<Q", off1 + 4)),
        "rows_off_past_the_end": patched(last + 8, struct.pack("<Q", lay.total + 64)),
        "n_rows_plus_1": patched(e1 + 16, struct.pack("<I", n1 + 1)),
        "n_rows_minus_1": patched(e1 + 16, struct.pack("<I", n1 - 1)),
        "n_rows_at_j0": patched(lay.entry(0, 0) + 16, struct.pack("<I", 1)),
        "contexts_swapped": patched(off1 + 60, struct.pack("<I", ctx1))[:off1 + 124] + struct.pack("<I", ctx0) + index[off1 + 128:],
        "contexts_equal": patched(off1 + 124, struct.pack("<I", ctx0)),
        "context_out_of_range": patched(off1 + 64 * (n1 - 1) + 60, struct.pack("<I", 65536)),
        "truncated": index[:-64],
        "appended": index + bytes(64),
    }
    if lay.color:
        # (plane 0 is Y: below zero is out of its range; plane 1 is Co: 131 071 is no context, 70 000 no sample)
        out["y_sample_negative"] = patched(lay.window(0, 1) + 4 * (2 * lay.w - 1), struct.pack(fmt, -1))
        out["co_sample_70000"] = patched(lay.window(1, 1) + 4 * (2 * lay.w - 1), struct.pack(fmt, 70000))
        _, offc, nc = lay.get(1, 1)
        if nc:
            out["co_context_131071"] = patched(offc + 64 * (nc - 1) + 60, struct.pack("<I", 131071))
    return out


def pack(blobs, align=64):
    """blobs back to back, each at a multiple of `align`: (bytes, offsets, lens)"""
    offs, out = [], bytearray()
    for b in blobs:
        offs.append(len(out))
        out += b
        out += bytes((-len(out)) % align)
    return bytes(out) + bytes(align), offs, [len(b) for b in blobs]
