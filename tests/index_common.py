"""What the restart-index tests share (test_index_cpu.py, test_index_gpu.py): the shapes and their images, the layout of an index
written out from the format's description in include/felics.h, and the corruptions both files refuse."""
import struct

import numpy as np

E_UNSUPPORTED = -10
E_INVALID_INDEX = -12
GRANULE = 4096
SEGMENTS = (4096, 12288)

# (W, H): what each covers is in the comment behind it
SHAPES = [
    (64, 64),      # 4096 pixels: K = 1
    (64, 65),      # K = 2 at segment 4096, last segment 64 pixels
    (100, 100),    # x0 = 96: mid-block start, x0 & 63 = 32
    (1, 9000),     # first-column rule everywhere, window of 2 samples
    (2, 5000),
    (4097, 1),     # row-0 rule across a boundary
    (5000, 3),     # segments starting in the first row
    (8200, 2),
    (4096, 3),     # x0 = 0 on every boundary: (0, y0 - 2) out of the window
    (2048, 5),
    (0, 5), (5, 0),  # empty images
    (512, 256),    # S1 content: halvings before the later checkpoints
]


def ramp(w, h, rgb):
    """the smooth ramp of test_gpu_decode.py"""
    smooth = (np.add.outer(np.arange(h), np.arange(w)) // 2 % 256).astype(np.uint8)
    return np.stack([smooth, smooth[::-1], 255 - smooth], -1).copy() if rgb else smooth


def images(w, h, rgb, n=3):
    """n frames of different content for a shape: noise, the ramp, synth S1 (512 x 256: S1 first)"""
    from felics_amd import synth

    rng = np.random.default_rng(w * 7919 + h * 31 + rgb)
    shape = (h, w, 3) if rgb else (h, w)
    if w == 0 or h == 0:
        return [np.zeros(shape, np.uint8) for _ in range(n)]
    s1 = [synth.rgb8(w, h, f) if rgb else synth.gray8(w, h, f, "S1") for f in range(2)]
    noise = rng.integers(0, 256, size=shape, dtype=np.uint8)
    kinds = [s1[0], noise, ramp(w, h, rgb), s1[1]] if (w, h) == (512, 256) else [noise, ramp(w, h, rgb), s1[0], s1[1]]
    return kinds[:n]


def index_size(w, h, color, seg):
    """the formula of include/felics.h, written out"""
    planes, nctx, sample = (3, 512, 2) if color else (1, 256, 1)
    k = (w * h + seg - 1) // seg
    cp = (8 + nctx * 6 * 2 + 2 * w * sample + 15) // 16 * 16
    return 64 + planes * k * cp


class Layout:
    """where the fields of an index lie"""

    def __init__(self, index):
        assert index[:4] == b"FLCX"
        self.version, self.color, self.depth, self.w, self.h, self.seg, self.k = struct.unpack_from("<HBBIIII", index, 4)
        self.plane_end = struct.unpack_from("<3Q", index, 24)
        self.planes, self.nctx, self.sample = (3, 512, 2) if self.color else (1, 256, 1)
        self.win_off = 8 + self.nctx * 12
        self.cp = (self.win_off + 2 * self.w * self.sample + 15) // 16 * 16

    def at(self, c, j):
        return 64 + (c * self.k + j) * self.cp


def corruptions(index):
    """name -> corrupted copy of a valid index with K >= 2 (RGB for the Co sample): each must be refused with E_INVALID_INDEX"""
    lay = Layout(index)
    assert lay.k >= 2

    def patched(pos, data):
        b = bytearray(index)
        b[pos:pos + len(data)] = data
        return bytes(b)

    off1 = struct.unpack_from("<Q", index, lay.at(0, 1))[0]
    out = {
        "magic": patched(0, b"FLCS"),
        "version": patched(4, struct.pack("<H", 2)),
        "size": index + bytes(16),
        "short": index[:-16],
        "width": patched(8, struct.pack("<I", lay.w + 1)),
        "offset_beyond": patched(lay.at(lay.planes - 1, lay.k - 1), struct.pack("<Q", lay.plane_end[lay.planes - 1] + 4096)),
        "offset_plus_1": patched(lay.at(0, 1), struct.pack("<Q", off1 + 1)),  # the end check of segment (0, 0)
    }
    if lay.color:
        # a Co sample of 300: the last window sample of plane 1, segment 1
        out["co_300"] = patched(lay.at(1, 1) + lay.win_off + 2 * (2 * lay.w - 1), struct.pack("<h", 300))
    return out


def pack_streams(streams, align=16):
    """streams back to back, each at a multiple of `align`: (blob, offsets, lens)"""
    offs, blob = [], bytearray()
    for s in streams:
        offs.append(len(blob))
        blob += s
        blob += bytes((-len(blob)) % align)
    return bytes(blob) + bytes(16), offs, [len(s) for s in streams]
