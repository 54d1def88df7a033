"""What the restart-index tests share (test_index_cpu.py, test_index_gpu.py, test_index_large_gpu.py): the shapes and their images,
the layout of an index written out from the format's description in include/felics.h, the corruptions both files refuse, banded
frames (contexts that fall silent for many checkpoints) with the measures that show they do, and the calls that run the encoder's
index writer and the indexed decoder between guard bytes."""
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


# ---- banded frames: contexts that are silent for many checkpoint intervals -----------------------------------------------------

def banded(w, h, rgb, loud, seed=5):
    """The raster cut into tiles of GRANULE pixels: a tile in `loud` is uniform noise 0..255, every other one noise in 126..129.  A
    context with a large difference has events in the loud tiles only, so at the checkpoints between two of them its row is the
    state of its first later record, and zeros behind the last one."""
    c = 3 if rgb else 1
    rng = np.random.default_rng(seed)
    quiet = rng.integers(126, 130, (w * h, c), np.uint8)
    noise = rng.integers(0, 256, (w * h, c), np.uint8)
    tile = np.arange(w * h) // GRANULE
    out = np.where(np.isin(tile, sorted(loud))[:, None], noise, quiet)
    return out.reshape((h, w, 3) if rgb else (h, w))


def state_rows(index):
    """the state rows of an index: planes x K x nctx x 6 (u16)"""
    lay = Layout(index)
    buf = np.frombuffer(index, np.uint8)
    out = np.zeros((lay.planes, lay.k, lay.nctx, 6), np.uint16)
    for c in range(lay.planes):
        for j in range(lay.k):
            at = lay.at(c, j) + 8
            out[c, j] = buf[at:at + lay.nctx * 12].view("<u2").reshape(lay.nctx, 6)
    return out


def held(rows, a, b):
    """contexts (over all planes) whose row is non-zero and identical at all checkpoints a + 1 .. b"""
    span = rows[:, a + 1:b + 1]
    return int((span[:, 0].any(-1) & (span == span[:, :1]).all((1, 3))).sum())


def dropped(rows, last):
    """contexts non-zero at checkpoint `last` and zero at every later one"""
    return int((rows[:, last].any(-1) & ~rows[:, last + 1:].any((1, 3))).sum())


# The shapes at which the encoder's index writer is tested (test_index_large_gpu.py), and whose content test_index_cpu.py measures:
# (W, H, tiles of GRANULE pixels per segment, the plans of loud tiles).  What each row reaches is in the comment behind it.
LARGE = [
    (4096, 132, (1,), [(0, 1, 130, 131), (0, 1), (0, 63, 64, 127, 128)]),  # K = 132: three chunks of 64 intervals, finds in lanes 63 and 0
    (1000, 541, (1,), [(0, 65, 131), (0, 132)]),        # K = 133: a last chunk of 5, x0 != 0 on the boundaries, a last tile of 328 pixels
    (1000, 541, (9, 17), [(0, 7, 8, 35, 70, 132)]),     # K = 15, 8: last intervals of 7 and 14 tiles, first loud tile at offsets 7, 8, 13
    (4096, 594, (9,), [(0, 8, 592, 593), (0, 8)]),      # K = 66: two chunks of intervals of two groups of eight
    (1000, 1100, (16, 32), [(0, 3, 100, 268)]),         # K = 17, 9: the command-line tools' default segment and the profiles'
]
MEASURE_MIN = 32  # a condition on the content, not a measurement: the reference alone gives 74 and more where it applies


def measures(w, h, seg_tiles, plan):
    """What a plan is there to show, as [("held", a, b) | ("dropped", last), the least count]: every gap of two or more checkpoints
    between loud intervals holds rows, and rows are dropped behind the last loud interval unless it is interval 0 or the last one.
    (0, 132) of 1000 x 541 ends in a loud tile of 328 pixels: few contexts have an event there, so the condition is 4.)"""
    k = (w * h + seg_tiles * GRANULE - 1) // (seg_tiles * GRANULE)
    loud = sorted({t // seg_tiles for t in plan})
    least = 4 if (w, h, seg_tiles, tuple(plan)) == (1000, 541, 1, (0, 132)) else MEASURE_MIN
    out = [(("held", a, b), least) for a, b in zip(loud, loud[1:]) if b - a >= 2]
    if 0 < loud[-1] < k - 1:
        out.append((("dropped", loud[-1]), least))
    return out


def measure(rows, what):
    return held(rows, *what[1:]) if what[0] == "held" else dropped(rows, what[1])


def first_difference(a, b):
    """the first offset at which two byte strings differ (the shorter one's length if one is a prefix of the other), None if equal"""
    if a == b:
        return None
    n = min(len(a), len(b))
    d = np.flatnonzero(np.frombuffer(a, np.uint8, n) != np.frombuffer(b, np.uint8, n))
    return int(d[0]) if d.size else n


def where_in_index(ref, off):
    """what the byte at `off` of an index laid out like `ref` belongs to"""
    lay = Layout(ref)
    if off < 64:
        return "header byte %d" % off
    c, j = divmod((off - 64) // lay.cp, lay.k)
    o = (off - 64) % lay.cp
    if o < 8:
        what = "bit offset"
    elif o < lay.win_off:
        what = "context %d, counter %d" % ((o - 8) // 12, (o - 8) % 12 // 2)
    else:
        what = "window sample %d" % ((o - lay.win_off) // lay.sample)
    return "plane %d, checkpoint %d of %d, %s" % (c, j, lay.k, what)


# ---- the encoder's index writer and the indexed decoder between guard bytes ----------------------------------------------------

class Encoded:
    """What felics_compress_batch_device_indexed left of frames of one shape: .streams and .indexes as bytes, and the device buffers
    themselves (.d_out, .d_idx behind .guard bytes, .offs, .lens, .isize) for a decoder that takes them as they lie."""


def encode_indexed(e, imgs, seg, d_out_cap=None, full=False):
    """frames of one shape -> (streams, indexes) as bytes, through felics_compress_batch_device_indexed; guard bytes around both.
    full: the Encoded instead."""
    import torch

    from felics_amd import api

    n = len(imgs)
    h, w = imgs[0].shape[:2]
    rgb = int(imgs[0].ndim == 3)
    isize = api.index_size(w, h, rgb, 0, seg)
    d_in = torch.from_numpy(np.stack(imgs)).cuda()
    cap = d_out_cap if d_out_cap is not None else n * ((imgs[0].size * 5 // 4 + 64 + 15) // 16 * 16)
    guard = 256
    d_out = torch.full((guard + cap + guard,), 0x5A, dtype=torch.uint8, device="cuda")
    d_idx = torch.full((guard + n * isize + guard,), 0x5A, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    offs, lens = e.compress_batch_device_indexed(d_in.data_ptr(), n, w, h, rgb, 0, d_out.data_ptr() + guard, cap, seg,
                                                 d_idx.data_ptr() + guard, n * isize)
    out, idx = d_out.cpu().numpy(), d_idx.cpu().numpy()
    for buf, size in ((out, cap), (idx, n * isize)):
        assert (buf[:guard] == 0x5A).all() and (buf[guard + size:] == 0x5A).all()
    streams = [out[guard + int(o):guard + int(o) + int(ln)].tobytes() for o, ln in zip(offs, lens)]
    indexes = [idx[guard + i * isize:guard + (i + 1) * isize].tobytes() for i in range(n)]
    if not full:
        return streams, indexes
    r = Encoded()
    r.streams, r.indexes, r.d_out, r.d_idx, r.guard, r.offs, r.lens, r.isize = streams, indexes, d_out, d_idx, guard, offs, lens, isize
    return r


def decode_indexed(enc, streams, indexes, frame_bytes, guard=0, expect=None):
    """streams + their indexes -> (status, frames as uint8 rows, the guard bytes intact).  expect: the code the call must raise."""
    import pytest
    import torch

    import felics_amd

    n = len(streams)
    blob, offs, lens = pack_streams(streams)
    stride = max((max(len(i) for i in indexes) + 15) // 16 * 16, 64)
    iblob = b"".join(i + bytes(stride - len(i)) for i in indexes)
    d_in = torch.from_numpy(np.frombuffer(blob, dtype=np.uint8).copy()).cuda()
    d_idx = torch.from_numpy(np.frombuffer(iblob, dtype=np.uint8).copy()).cuda()
    total = frame_bytes * n
    d_px = torch.full((guard + max(total, 16) + guard,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    args = (d_in.data_ptr(), offs, lens, d_idx.data_ptr(), stride, d_px.data_ptr() + guard, total)
    if expect is None:
        _, status = enc.decompress_batch_device_indexed(*args)
    else:
        with pytest.raises(felics_amd.FelicsError) as ei:
            enc.decompress_batch_device_indexed(*args)
        assert ei.value.code == expect
        status = ei.value.status
    host = d_px.cpu().numpy()
    if guard:
        assert (host[:guard] == 0xA5).all() and (host[guard + max(total, 16):] == 0xA5).all()
    return status, [host[guard + i * frame_bytes:guard + (i + 1) * frame_bytes] for i in range(n)]
