"""Regions of 16-bit streams through the version-2 restart index, host side (no GPU): the ABI surface, the host model
felics_decompress_region_indexed16 against numpy crops of the originals and against felics_decompress_indexed16, what a region's
checks cover under every corruption of index16_common (the expectation worked out from the format, see _damaged), the refusals."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import index16_common as ic
from tests import region_common as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("felics_decompress_region_indexed_wide", "felics_decompress_regions_device_indexed_wide", "felics_get_region_wide_stats")
SHAPES = ((100, 100), (4096, 3), (8200, 2), (1, 9000), (2, 5000), (4097, 1), (5000, 3), (64, 64), (64, 65))
GUARD = 32


@pytest.fixture(scope="module")
def api():
    from felics_amd import api as a

    a.lib()
    return a


def shape_cases(shapes=SHAPES):
    for w, h in shapes:
        for rgb in (0, 1):
            for seg in (ic.SEGMENTS if (w, h) in ((100, 100), (8200, 2)) else ic.SEGMENTS[:1]):
                yield w, h, rgb, seg


def raw_region(api, stream, index, region, cap=None, hdr=None):
    """felics_decompress_region_indexed_wide into a buffer with guard bytes, which must stay intact: (code, the crop's bytes)"""
    s = np.frombuffer(stream, np.uint8)
    i = np.frombuffer(index, np.uint8)
    planes = 3 if stream[4] else 1
    size = region[2] * region[3] * planes * 2
    cap = size if cap is None else cap
    out = np.full(GUARD + size + GUARD, 0xA5, np.uint8)
    reg = api._CRegion(0, *region)
    code = api.lib().felics_decompress_region_indexed_wide(s.ctypes.data if len(s) else None, len(s), i.ctypes.data if len(i) else None, len(i),
                                                           C.byref(reg), out.ctypes.data + GUARD, cap, hdr)
    assert (out[:GUARD] == 0xA5).all() and (out[GUARD + min(cap, size):] == 0xA5).all(), region
    return code, out[GUARD:GUARD + size]


def test_abi_surface(api, tmp_path):
    """the three symbols are exported and bound, their aliases compile, a NULL context is refused"""
    L = api.lib()
    for name in SYMBOLS:
        assert hasattr(L, name) and name in api.EXPORTS, name
    assert callable(api.decompress_region_indexed16)
    assert callable(api.Encoder.decompress_regions_device_indexed16) and callable(api.Encoder.region16_stats)
    st = api._CRegion16Stats(7, 7, 7, 7, 7, 7)
    assert C.sizeof(st) == 48
    assert L.felics_get_region_wide_stats(None, C.byref(st), C.sizeof(st)) == -11 and (st.regions, st.passes) == (7, 7)
    assert L.felics_decompress_regions_device_indexed_wide(None, 1, None, None, None, None, None, None, 1, None, None, 0, None, None, None) == -11
    b = np.zeros(64, np.uint8)
    assert L.felics_decompress_region_indexed_wide(b.ctypes.data, 64, b.ctypes.data, 64, None, b.ctypes.data, 64, None) == -11
    src = tmp_path / "alias.c"
    src.write_text('#include "felics.h"\n'
                   "int f(felics_ctx *c, const uint8_t *p, const uint64_t *a, const felics_region *r, void *o, felics_region16_stats *s) {\n"
                   "    return felics_decompress_region_indexed16(p, 1, p, 1, r, o, 0, 0)\n"
                   "         + felics_decompress_regions_device_indexed16(c, 1, p, a, a, p, a, a, 1, r, o, 0, 0, 0, 0)\n"
                   "         + felics_get_region16_stats(c, s, sizeof *s);\n"
                   "}\n")
    for cc, std in (("cc", "-std=c99"), ("c++", "-std=c++11")):
        subprocess.run([cc, std, "-Wall", "-Werror", "-x", "c" if cc == "cc" else "c++", "-c", str(src), "-I", os.path.join(ROOT, "include"),
                        "-o", str(tmp_path / "alias.o")], check=True)


@pytest.mark.parametrize("w,h,rgb,seg", list(shape_cases()))
def test_host_model_crops(api, oracle, w, h, rgb, seg):
    """every fixed, edge and empty window and six random ones: the crop is the numpy crop of the original, the guard bytes around it
    stay as they were"""
    img = ic.noise(w, h, rgb, 10, 1000 + w + h)
    stream = oracle.compress(img)
    index = api.index16_build(stream, seg)
    for region in rc.all_regions(w, h, 6):
        code, got = raw_region(api, stream, index, region)
        want = rc.crop(img, region)
        assert code == 0 and (got.view(np.uint16).reshape(want.shape) == want).all(), (w, h, rgb, seg, region)
        assert (api.decompress_region_indexed16(stream, index, *region) == want).all()


@pytest.mark.parametrize("name", list(ic.cases()))
def test_full_frame_is_the_indexed_decode(api, oracle, name):
    """the full-frame region of every case of index16_common (alias, spikes, chroma, banded and the empties among them) is
    felics_decompress_indexed16's frame"""
    img = ic.cases()[name][0]
    stream = oracle.compress(img)
    index = api.index16_build(stream, 4096)
    h, w = img.shape[:2]
    full = api.decompress_indexed16(stream, index)
    hdr = api._CHeader()
    code, got = raw_region(api, stream, index, (0, 0, w, h), hdr=C.byref(hdr))
    assert code == 0 and (hdr.width, hdr.height, hdr.pixel_depth) == (w, h, 1)
    assert (got.view(np.uint16).reshape(img.shape) == full).all() and (full == img).all(), name


# ---- corruption: which windows a damaged index still serves -------------------------------------------------------------------------
#
# Worked out from the format (include/felics.h "Restart index: 16-bit streams"), not from the code: a region call checks the two
# headers and then, for every segment it needs and every plane, that segment's directory entry, rows and window.  A directory entry's
# row chain ends where its SUCCESSOR's rows_off says, so a wrong rows_off damages its own entry and the one in front of it.

HEADER = ("magic", "version_1", "depth_0", "width", "height", "segment_pixels", "K", "total_plus_64", "total_minus_64", "reserved", "truncated",
          "appended")


def _damaged(what, planes, k):
    """the (plane, segment) pairs whose own checks the corruption fails"""
    last = (planes - 1, k - 1)
    return {
        "rows_off_plus_64": {(0, 0), (0, 1)},      # (0, 0)'s chain no longer ends at (0, 1)'s rows_off; (0, 1)'s not at (0, 2)'s
        "rows_off_misaligned": {(0, 0), (0, 1)},
        "n_rows_plus_1": {(0, 1)},                 # (0, 1)'s chain overshoots (0, 2)'s rows_off; (0, 0) reads rows_off only
        "n_rows_minus_1": {(0, 1)},
        "contexts_swapped": {(0, 1)},
        "contexts_equal": {(0, 1)},
        "context_out_of_range": {(0, 1)},
        "y_sample_negative": {(0, 1)},             # window (0, 1)
        "n_rows_at_j0": {(0, 0)},
        "rows_off_past_the_end": {last, (last[0], last[1] - 1)},  # the last entry and its predecessor's chain end
        "co_sample_70000": {(1, 1)},               # window (1, 1): plane 1 is walked for every needed segment
        "co_context_131071": {(1, 1)},
    }[what]


def _windows(w, h):
    """name -> window of a K = 3 frame cut every 4096 pixels, and the edge of the plan it stands for"""
    if (w, h) == (64, 130):  # segment 0 = rows 0-63, 1 = rows 64-127, 2 = rows 128-129
        return {"in_2": (0, 128, 64, 2), "in_1": (10, 70, 20, 5), "early_0": (10, 10, 5, 5), "end_of_0": (0, 63, 64, 1), "both_01": (5, 60, 10, 8),
                "empty": (0, 0, 0, 0), "full": (0, 0, 64, 130)}
    # 100 x 100: pixel 4096 is (96, 40), pixel 8192 is (92, 81)
    return {"in_2": (0, 83, 100, 10), "in_1": (10, 70, 20, 5), "early_0": (10, 10, 5, 5), "end_of_0": (0, 40, 96, 1), "both_01": (90, 40, 10, 2),
            "empty": (0, 0, 0, 0), "full": (0, 0, 100, 100)}


@pytest.mark.parametrize("name", ("noise12", "100x100_rgb"))
def test_checks_cover_the_needed_segments_only(api, oracle, name):
    img = ic.cases()[name][0]
    stream = oracle.compress(img)
    index = api.index16_build(stream, 4096)
    lay = ic.Layout16(index)
    h, w = img.shape[:2]
    assert lay.k == 3 and lay.get(0, 1)[2] >= 2
    wins = _windows(w, h)
    needs = {n: rc.needed_by_marking(w, h, 4096, win) if win[2] * win[3] else [] for n, win in wins.items()}
    assert needs["in_2"] == [2] and needs["in_1"] == [1] and needs["early_0"] == [0] and needs["end_of_0"] == [0] and needs["both_01"] == [0, 1]
    # how far segment 0 is walked: to the pixel behind the region's last one, or to its end at 4096
    last = {n: (win[1] + win[3] - 1) * w + win[0] + win[2] for n, win in wins.items() if win[2] * win[3]}
    assert last["early_0"] < 4096 <= last["end_of_0"]
    bad = ic.corruptions(index)
    assert len(bad) >= (25 if lay.color else 23)
    for what, b in bad.items():
        for n, win in wins.items():
            code, got = raw_region(api, stream, b, win)
            exact = code == 0 and (got.view(np.uint16).reshape(rc.crop(img, win).shape) == rc.crop(img, win)).all()
            if what in HEADER:  # checked for every region, the empty one too
                assert code == ic.E_INVALID_INDEX, (what, n)
            elif what.startswith("bit_offset"):
                # checkpoint (0, 1) moved by a bit: segment (0, 0) no longer ends on it, which only a walk to its end finds out;
                # segment (0, 1) itself then starts off its codes, and what that decodes to is not the format's to say
                if 0 in needs[n] and last[n] >= 4096:
                    assert code == ic.E_INVALID_INDEX, (what, n)  # (plane 0, segment 0) is the first item
                elif 1 not in needs[n]:
                    assert exact, (what, n, code)
            else:
                hit = any((c, j) in _damaged(what, lay.planes, lay.k) for c in range(lay.planes) for j in needs[n])
                if hit:
                    assert code == ic.E_INVALID_INDEX, (what, n)
                else:
                    assert exact, (what, n, code)
    # the issue's own list, spelled out: a window wholly in segment 2 is served, one that needs (0, 1) is refused
    for what in ("rows_off_plus_64", "n_rows_plus_1", "contexts_swapped", "context_out_of_range"):
        assert raw_region(api, stream, bad[what], wins["in_2"])[0] == 0 and raw_region(api, stream, bad[what], wins["in_1"])[0] == ic.E_INVALID_INDEX
        assert raw_region(api, stream, bad[what], wins["both_01"])[0] == ic.E_INVALID_INDEX
    # the last directory entry: gray -- (0, 2) and, through its chain end, (0, 1): every window but those inside segment 0;
    # RGB -- (2, 2) and (2, 1): the same windows, refused when plane 2 is reached
    for n in wins:
        want = ic.E_INVALID_INDEX if set(needs[n]) & {1, 2} else 0
        assert raw_region(api, stream, bad["rows_off_past_the_end"], wins[n])[0] == want, n


def test_refusals(api, oracle):
    img = ic.noise(100, 100, 1, 10, 5)
    stream = oracle.compress(img)
    index = api.index16_build(stream, 4096)
    for region in ((0, 0, 101, 1), (99, 99, 1, 2), (0xFFFFFFFF, 0, 2, 1), (1, 0, 0xFFFFFFFF, 1), (0, 0xFFFFFFFF, 1, 2)):  # (the last three wrap in 32 bits)
        s = np.frombuffer(stream, np.uint8)
        i = np.frombuffer(index, np.uint8)
        reg = api._CRegion(0, *region)
        out = np.zeros(64, np.uint8)
        assert api.lib().felics_decompress_region_indexed_wide(s.ctypes.data, len(s), i.ctypes.data, len(i), C.byref(reg), out.ctypes.data, 64,
                                                               None) == rc.E_INVALID_ARGUMENT, region
    with pytest.raises(api.FelicsError) as ei:
        api.decompress_region_indexed16(stream, index, 0xFFFFFFFF, 0, 2, 1)
    assert ei.value.code == rc.E_INVALID_ARGUMENT
    code, got = raw_region(api, stream, index, (5, 5, 10, 10), cap=599)  # a short cap: nothing written
    assert code == rc.E_BUFFER_TOO_SMALL and (got == 0xA5).all()
    code, got = raw_region(api, stream, index, (5, 5, 10, 10), cap=600)
    assert code == 0 and (got.view(np.uint16).reshape(10, 10, 3) == img[5:15, 5:15]).all()
    # an 8-bit stream (beside either kind of index); a version-1 index beside the 16-bit stream
    img8 = (img >> 8).astype(np.uint8)
    s8 = oracle.compress(img8)
    v1 = api.index_build(s8, 4096)
    for idx in (index, v1):
        assert raw_region(api, s8, idx, (5, 5, 10, 10))[0] == ic.E_UNSUPPORTED
    for region in ((5, 5, 10, 10), (0, 0, 0, 0)):
        assert raw_region(api, stream, v1, region)[0] == ic.E_INVALID_INDEX
    # the 8-bit region model keeps refusing the 16-bit stream
    with pytest.raises(api.FelicsError) as ei:
        api.decompress_region_indexed(stream, index, 5, 5, 10, 10)
    assert ei.value.code == ic.E_UNSUPPORTED
