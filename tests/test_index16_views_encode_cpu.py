"""felics_compress_views_device_indexed16, host side (no GPU): the new symbols; and the proof, from felics_index16_build of the oracle's
streams and the bucket rule restated in index16_views_encode_cases.py, that the mixed cases of test_index16_views_encode_gpu.py reach
the edges the table-driven index kernels branch on."""
import ctypes as C
import os
import subprocess

import pytest

from tests import index16_common as ic
from tests import index16_views_encode_cases as vc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def api():
    from felics_amd import api as a

    a.lib()
    return a


@pytest.fixture(scope="module")
def built(api, oracle):
    """case -> (frames, segments, the index of every frame's stream at its own segment (None for 0), the same at 4096)"""
    out = {}
    for name, (frames, segs) in (("gray", vc.mixed_gray()), ("rgb", vc.mixed_rgb())):
        streams = [oracle.compress(f) for f in frames]
        own = [api.index16_build(s, seg) if seg else None for s, seg in zip(streams, segs)]
        out[name] = (frames, segs, own, [api.index16_build(s, 4096) for s in streams])
    return out


def test_abi_surface(api, tmp_path):
    """the two symbols are exported, bound and in EXPORTS, their aliases compile, a NULL context is refused"""
    L = api.lib()
    for name in ("felics_compress_views_device_indexed_wide", "felics_get_index_view_wide_emit_stats"):
        assert hasattr(L, name) and name in api.EXPORTS, name
    for method in ("compress_views_device_indexed16", "compress_arrays_device_indexed16", "compress_views_device_indexed16_raw", "index16_view_emit_stats"):
        assert callable(getattr(api.Encoder, method)), method
    st = api._CIndex16ViewEmitStats(*([7] * 7))
    assert C.sizeof(st) == 56
    assert L.felics_get_index_view_wide_emit_stats(None, C.byref(st), C.sizeof(st)) == -11 and (st.views, st.redone) == (7, 7)
    assert L.felics_compress_views_device_indexed_wide(None, 1, None, None, None, None, 0, None, 0, None, None, None, None, None) == -11
    src = tmp_path / "alias.c"
    src.write_text('#include "felics.h"\n'
                   "int f(felics_ctx *c, const felics_view *v, const uint32_t *g, uint64_t *a, felics_index16_view_emit_stats *s) {\n"
                   "    return felics_compress_views_device_indexed16(c, 0, v, g, 0, 0, 0, 0, 0, a, a, a, a, a) + felics_get_index16_view_emit_stats(c, s, sizeof *s);\n"
                   "}\n")
    for cc, std in (("cc", "-std=c99"), ("c++", "-std=c++11")):
        subprocess.run([cc, std, "-Wall", "-Werror", "-x", "c" if cc == "cc" else "c++", "-c", str(src), "-I", os.path.join(ROOT, "include"),
                        "-o", str(tmp_path / "alias.o")], check=True)


def test_the_shapes_share_a_bucket():
    """the gray shapes form one bucket and so do the RGB ones; straddle3 and the 70 x 240 frame form a second gray bucket; neither call
    hands its views over in bucket order"""
    assert [vc.tiles(w, h) for w, h in vc.GRAY_SHAPES] == [4, 3, 3, 3] and [vc.tiles(w, h) for w, h in vc.RGB_SHAPES] == [2, 2, 3]
    assert 96 * 128 % 4096 == 0
    for frames, _ in (vc.mixed_gray(), vc.mixed_rgb()):
        shapes = [vc.shape_of(f) for f in frames]
        b = vc.buckets(shapes)
        assert len(b) == 1 and sorted(b[0]) == list(range(len(frames))) and b[0] != list(range(len(frames)))
        assert len(set(shapes)) >= 3
    second = [vc.shape_of(f) for f in vc.second_bucket()[0]]
    assert second == [(64, 260), vc.SECOND_SHAPE]
    both = vc.buckets(list(vc.GRAY_SHAPES) + second)
    assert [sorted(x) for x in both] == [[0, 1, 2, 3], [4, 5]]


@pytest.mark.parametrize("case", ("gray", "rgb"))
def test_one_sub_batch_holds_different_k(built, case):
    """K = 3 beside K = 4 (gray; RGB: 2 beside 3) at 4096 and K = 1 beside K = 2 at 12 288, all in one sub-batch"""
    frames, segs, own, _ = built[case]
    ks = {seg: {ic.Layout16(x).k for x, s in zip(own, segs) if s == seg} for seg in (4096, 12288)}
    assert ks[4096] == ({3, 4} if case == "gray" else {2, 3}), ks
    assert ks[12288] == {1, 2} if case == "gray" else ks[12288] == {1}, ks
    assert len(vc.sub_batches([vc.shape_of(f) for f in frames], segs, 3 if case == "rgb" else 1, 1 << 30)) == 1
    if case == "gray":  # ... and a cap of five checkpoints cuts the bucket, once into a pass of one shape
        cut = vc.sub_batches([vc.shape_of(f) for f in frames], segs, 1, 5)
        assert len(cut) > 2 and any(len({vc.shape_of(frames[i]) for i in c}) == 1 for c in cut)


@pytest.mark.parametrize("case", ("gray", "rgb"))
def test_every_image_has_rows(built, case):
    """every image has a checkpoint with n_rows > 0 at 4096, and at its own segment wherever that gives it a second checkpoint"""
    _, segs, own, at4096 = built[case]
    for x in at4096:
        assert max(ic.Layout16(x).n_rows()) > 0
    for x, seg in zip(own, segs):
        if seg and ic.Layout16(x).k >= 2:
            assert max(ic.Layout16(x).n_rows()) > 0


@pytest.mark.parametrize("case", ("gray", "rgb"))
def test_neighbouring_planes_share_a_context_with_a_row(built, case):
    """in table order, the last plane of one image and the first plane of the next (two images, other K and segment) hold a row of one
    context: a writer that took the plane boundary for a chain's continuation, or one plane's K for the other's, would differ here"""
    frames, segs, own, _ = built[case]
    order = vc.buckets([vc.shape_of(f) for f in frames])[0]
    found = 0
    for a, b in zip(order, order[1:]):
        if not (segs[a] and segs[b]):
            continue
        la, lb = ic.Layout16(own[a]), ic.Layout16(own[b])
        last = set().union(*[set(ic.rows_of(own[a], la, la.planes - 1, j)[0]) for j in range(la.k)])
        first = set().union(*[set(ic.rows_of(own[b], lb, 0, j)[0]) for j in range(lb.k)])
        if last & first and (la.k, la.seg) != (lb.k, lb.seg):
            found += 1
    assert found >= 1


@pytest.mark.parametrize("case", ("gray", "rgb"))
def test_the_indexes_have_different_lengths(built, case):
    """no two indexes of the sub-batch have one length: an index written to another one's place cannot pass"""
    _, segs, own, _ = built[case]
    lens = [len(x) for x in own if x is not None]
    assert len(lens) == sum(1 for s in segs if s) and len(set(lens)) == len(lens), lens
