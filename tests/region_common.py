"""What the region tests share (test_region_cpu.py, test_region_gpu.py): the windows asked of every shape of index_common.SHAPES and
the planner written out by marking pixels."""
import numpy as np

E_INVALID_ARGUMENT = -11
E_BUFFER_TOO_SMALL = -8

# (W, H) -> windows (x, y, w, h), each the smallest at which one branch of the walk can go wrong (segments of 4096 pixels)
FIXED = {
    (100, 100): [
        (33, 40, 31, 3),     # inside one 64-lane block, unaligned; its segment starts mid-block at x0 = 96
        (90, 40, 10, 2),     # straddles the boundary at pixel 4096 in mid-row
        (0, 0, 100, 100),    # the full decode
    ],
    (8200, 2): [
        (5000, 0, 100, 2),   # needs segments {1, 3} and not 2: a plan with a hole
        (4100, 1, 50, 1),    # segment 3 only
    ],
    (4096, 3): [
        (0, 1, 4096, 1),     # exactly one segment, x0 = 0: the (0, y0 - 2) rule
        (4000, 0, 96, 3),    # every segment, an early stop in the last one
    ],
    (1, 9000): [(0, 4090, 1, 20)],                      # the first-column rule across a boundary
    (2, 5000): [(0, 4090, 1, 20), (1, 4090, 1, 20)],
    (4097, 1): [(4090, 0, 7, 1)],                       # the row-0 rule across a boundary
    (5000, 3): [(4090, 0, 7, 1), (4000, 0, 200, 1)],
    (512, 256): [(100, 100, 200, 50)],                  # S1 content: halvings in front of the checkpoint
    (64, 64): [(10, 10, 5, 5)],                         # K = 1: the walk stops early in the only segment
}


def edges(w, h):
    """windows touching each edge of a w x h image, and the empty ones (anywhere inside, the far corner included)"""
    if w == 0 or h == 0:
        return [(0, 0, 0, 0), (w, h, 0, 0), (0, 0, w, h)]
    return [(0, 0, w, 1), (0, h - 1, w, 1), (0, 0, 1, h), (w - 1, 0, 1, h), (w - 1, h - 1, 1, 1),
            (0, 0, 0, 0), (w, h, 0, 0), (0, 0, w, 0), (w // 2, h // 2, 0, 1)]


def random_regions(w, h, n, seed):
    """n seeded windows inside a w x h image: mostly small, a quarter of them as wide as the image allows"""
    if w == 0 or h == 0:
        return []
    rng = np.random.default_rng(seed * 1000003 + w * 7919 + h)
    out = []
    for k in range(n):
        x, y = int(rng.integers(0, w)), int(rng.integers(0, h))
        ww = w - x if k % 4 == 0 else int(rng.integers(1, min(w - x, 300) + 1))
        hh = int(rng.integers(1, min(h - y, 40) + 1))
        out.append((x, y, ww, hh))
    return out


def all_regions(w, h, n_random, seed=1):
    return FIXED.get((w, h), []) + edges(w, h) + random_regions(w, h, n_random, seed)


def needed_by_marking(w, h, seg, region):
    """the segments that hold a pixel of the region: mark its pixels, divide by segment_pixels"""
    x, y, rw, rh = region
    mark = np.zeros((h, w), dtype=bool)
    mark[y:y + rh, x:x + rw] = True
    return sorted(set((np.flatnonzero(mark.reshape(-1)) // seg).tolist()))


def crop(img, region):
    x, y, rw, rh = region
    return img[y:y + rh, x:x + rw]
