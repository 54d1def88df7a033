"""Restart index, lane form (64 segments per wave), what can be checked without a GPU: the export of its threshold, the grown
felics_index_stats and the wrapper's view of both."""
import ctypes as C
import inspect
import re

import pytest


@pytest.fixture(scope="module")
def api():
    from felics_amd import api as a

    a.lib()
    return a


def test_threshold_export(api):
    """felics_index_lanes_min_items: 0xFFFFFFFF (no call takes the lane form by itself) or at least one wave's 64 items"""
    L = api.lib()
    assert hasattr(L, "felics_index_lanes_min_items") and "felics_index_lanes_min_items" in api.EXPORTS
    for color in (0, 1):
        v = api.index_lanes_min_items(color)
        assert v == L.felics_index_lanes_min_items(color)
        assert v == 0xFFFFFFFF or 64 <= v < 0xFFFFFFFF, (color, v)


def test_index_stats_refuses_null_and_writes_nothing(api):
    L = api.lib()
    st = api._CIndexStats(7, 7, 7, 7)
    assert L.felics_get_index_stats(None, C.byref(st), C.sizeof(st)) == -11
    assert (st.streams, st.segments8, st.lane_segments8, st.lane_passes) == (7, 7, 7, 7)


def test_index_stats_fields_in_header_order(api):
    """api._CIndexStats against the struct as include/felics.h declares it: four uint64_t, the two new ones at the end"""
    import os

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    text = open(os.path.join(root, "include", "felics.h")).read()
    body = re.search(r"typedef struct felics_index_stats \{(.*?)\} felics_index_stats;", text, re.S).group(1)
    declared = re.findall(r"uint64_t\s+(\w+)\s*;", body)
    assert declared == ["streams", "segments8", "lane_segments8", "lane_passes"]
    assert [n for n, _ in api._CIndexStats._fields_] == declared
    assert all(t is C.c_uint64 for _, t in api._CIndexStats._fields_) and C.sizeof(api._CIndexStats) == 32


def test_decode_stats_names_the_new_keys(api):
    """(no device here: the keys as Encoder.decode_stats writes them)"""
    src = inspect.getsource(api.Encoder.decode_stats)
    for key in ("segments8", "lane_segments8", "lane_passes"):
        assert 'out["%s"]' % key in src, key
    assert callable(api.index_lanes_min_items)
