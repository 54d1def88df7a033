"""What the tests of felics_compress_views_device_indexed16 share (test_index16_views_encode_cpu.py, test_index16_views_encode_gpu.py):
the mixed cases -- the smallest shapes that share a bucket and still differ in K --, the bucket and cut rules restated from
bucket_images' comment, and the Surface both files describe views with.  That the cases reach their edges is shown in the CPU file."""
import numpy as np

from tests import index16_common as ic
from tests import index16_encode_cases as ec

SORT_TILE = 4096
SEG_CYCLE = (4096, 8192, 12288, 0)  # per-view segments cycle through these; 0: the view gets no index

# gray16, one bucket (3 to 4 sort tiles).  96 x 128 is a whole number of segments at 4096: the last checkpoint's segment is full.
GRAY_SHAPES = ((100, 150), (64, 130), (96, 128), (50, 170))
# RGB16, one bucket (2 to 3 tiles)
RGB_SHAPES = ((33, 130), (40, 150), (48, 200))
# a second gray bucket (5 tiles): straddle3 (64 x 260) beside a 70 x 240 frame
SECOND_SHAPE = (70, 240)


def tiles(w, h):
    return (w * h + SORT_TILE - 1) // SORT_TILE


def checkpoints(w, h, seg):
    return (w * h + seg - 1) // seg if seg else 0


def _content(w, h, rgb, k):
    """frame k of a case: noise of 12, 10 and 8 bits, so every frame has rows at every checkpoint behind the first and no two
    indexes of a case have one length"""
    return ic.noise(w, h, rgb, (12, 10, 8)[k % 3], 700 + 31 * k + w)


def mixed_gray():
    """twelve views, the four shapes three times over in a rotating order (not the bucket order: the largest shape comes first), so that
    with segments cycling through SEG_CYCLE every shape meets 4096, and 100 x 150 meets 12 288 beside two smaller shapes:
    K = 3 beside K = 4 at 4096, K = 1 beside K = 2 at 12 288.  -> (frames, segments)"""
    frames = []
    for rep in range(3):
        for s in range(4):
            w, h = GRAY_SHAPES[(s + rep) % 4]
            frames.append(_content(w, h, 0, len(frames)))
    return frames, [SEG_CYCLE[i % 4] for i in range(len(frames))]


def mixed_rgb():
    """nine views, shape i % 3 and segment i % 4: 33 x 130 meets 4096 and 12 288, 40 x 150 meets 8192 and 4096, 48 x 200 all three.
    -> (frames, segments)"""
    frames = [_content(*RGB_SHAPES[i % 3], 1, i) for i in range(9)]
    return frames, [SEG_CYCLE[i % 4] for i in range(len(frames))]


def second_bucket():
    return [ec.cases()["straddle3"][0], ic.noise(*SECOND_SHAPE, 0, 10, 77)], [4096, 8192]


# ---- bucket_images, restated from its comment ----------------------------------------------------------------------------------------

def buckets(shapes):
    """images of ONE depth and colour (zero-sized ones left out), as indexes into `shapes`: sorted by sort tiles T (stable), a bucket
    holds T_min .. ceil(1.25 T_min).  -> the buckets in order, each a list of indexes in table order"""
    order = sorted((i for i, (w, h) in enumerate(shapes) if w * h), key=lambda i: tiles(*shapes[i]))
    out = []
    while order:
        lim = (5 * tiles(*shapes[order[0]]) + 3) // 4
        take = [i for i in order if tiles(*shapes[i]) <= lim]
        out.append(take)
        order = order[len(take):]
    return out


def sub_batches(shapes, segs, planes, cps_cap):
    """the buckets cut where the checkpoints of the images that ask for an index would outgrow cps_cap, at least one image per
    sub-batch (no other bound bites at these sizes)"""
    out = []
    for b in buckets(shapes):
        cur, cps = [], 0
        for i in b:
            add = planes * checkpoints(*shapes[i], segs[i])
            if cur and cps + add > cps_cap:
                out.append(cur)
                cur, cps = [], 0
            cur.append(i)
            cps += add
        out.append(cur)
    return out


def shape_of(img):
    return (img.shape[1], img.shape[0])


class Surface:
    """A host array and its copy in device memory; view(v) turns a numpy view of the host array into the library's view tuple."""

    def __init__(self, host, upload=True):
        import torch

        self.host = np.ascontiguousarray(host)
        src = self.host if upload else np.zeros_like(self.host)
        # (uint16 frames travel as bytes: not every torch build has a uint16 dtype on the device)
        self.dev = torch.from_numpy(src.view(np.uint8).reshape(-1).copy()).cuda() if src.size else torch.zeros(64, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        self.base = self.host.__array_interface__["data"][0]

    def view(self, v):
        from felics_amd import api

        h, w = v.shape[:2]
        color, depth = int(v.ndim == 3), int(v.dtype == np.uint16)
        if h * w == 0:
            return (0, w, h, color, depth, 0, 0, 0)
        off = v.__array_interface__["data"][0] - self.base
        t = (self.dev.data_ptr() + off, w, h, color, depth, v.strides[0], v.strides[1], v.strides[2] if v.ndim == 3 else 0)
        lo, hi = api.view_extent(t)
        assert off + lo >= 0 and off + hi <= self.host.nbytes, (lo, hi, off)  # the caller's bounds check
        return t


def dense(img):
    s = Surface(img)
    return (s, s.host)
