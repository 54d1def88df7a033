"""The 16-bit encoder's restart index, host side (no GPU): the new symbols; and the proof, from felics_index16_build's bytes and a
model of the row rule written from the pixels alone (index16_encode_cases.py), that the cases of test_index16_encode_gpu.py reach the
edges the row kernel branches on -- each with a nearly right rule that must give other bytes."""
import ctypes as C
import os
import subprocess

import pytest

from tests import index16_common as ic
from tests import index16_encode_cases as ec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEG = 4096


@pytest.fixture(scope="module")
def api():
    from felics_amd import api as a

    a.lib()
    return a


@pytest.fixture(scope="module")
def built(api, oracle):
    """name -> (frame, index at SEG of the oracle's stream), for the new cases and the ones of index16_common the proofs name"""
    frames = {name: img for name, (img, _) in ec.cases().items()}
    frames.update({name: ic.cases()[name][0] for name in ("noise12", "noise10", "alias", "flat", "chroma")})
    return {name: (img, api.index16_build(oracle.compress(img), SEG)) for name, img in frames.items()}


def test_abi_surface(api, tmp_path):
    """the two symbols are exported and bound, their aliases compile, a NULL context is refused"""
    L = api.lib()
    for name in ("felics_compress_batch_device_indexed_wide", "felics_get_index_wide_emit_stats"):
        assert hasattr(L, name) and name in api.EXPORTS, name
    assert callable(api.Encoder.compress_batch_device_indexed16) and callable(api.Encoder.index16_emit_stats)
    st = api._CIndex16EmitStats(7, 7, 7, 7)
    assert C.sizeof(st) == 32
    assert L.felics_get_index_wide_emit_stats(None, C.byref(st), C.sizeof(st)) == -11 and (st.streams, st.passes) == (7, 7)
    assert L.felics_compress_batch_device_indexed_wide(None, 1, None, 8, 8, 0, None, 0, 4096, None, 0, None, None, None, None, None) == -11
    src = tmp_path / "alias.c"
    src.write_text('#include "felics.h"\n'
                   "int f(felics_ctx *c, uint64_t *a, felics_index16_emit_stats *s) {\n"
                   "    return felics_compress_batch_device_indexed16(c, 0, 0, 1, 1, 0, 0, 0, 4096, 0, 0, a, a, a, a, a) + felics_get_index16_emit_stats(c, s, sizeof *s);\n"
                   "}\n")
    for cc, std in (("cc", "-std=c99"), ("c++", "-std=c++11")):
        subprocess.run([cc, std, "-Wall", "-Werror", "-x", "c" if cc == "cc" else "c++", "-c", str(src), "-I", os.path.join(ROOT, "include"),
                        "-o", str(tmp_path / "alias.o")], check=True)


@pytest.mark.parametrize("name", list(ec.cases()) + ["noise12", "noise10", "alias", "flat", "chroma"])
def test_the_model_gives_the_builders_rows(built, name):
    """the row rule of the issue, replayed from the pixels: n_rows of every entry and every row's bytes equal felics_index16_build's"""
    img, index = built[name]
    counts, blob = ec.rows_model(img, SEG)
    want_counts, want_blob = ec.rows_of_index(index)
    assert counts == want_counts and blob == want_blob


def _differs(img, index, rule):
    """a nearly right rule gives other rows than the builder's"""
    counts, blob = ec.rows_model(img, SEG, rule)
    want_counts, want_blob = ec.rows_of_index(index)
    return counts != want_counts or blob != want_blob


def test_a_gap_straddles_three_checkpoints(built):
    """(a) checkpoints 1, 2 and 3 hold identical, non-empty rows; a rule that writes the first straddled checkpoint only gives other bytes"""
    img, index = built["straddle3"]
    lay = ic.Layout16(index)
    assert lay.k == 5 and ec.edges(img, SEG)["straddle3"]
    rows = [ic.rows_of(index, lay, 0, j) for j in (1, 2, 3)]
    assert len(rows[0][0]) >= 3
    for ctxs, counters in rows[1:]:
        assert (ctxs == rows[0][0]).all() and (counters == rows[0][1]).all()
    assert _differs(img, index, "first")


def test_an_event_exactly_at_p0(built):
    """(b) a context whose first event of a segment stands exactly at p0 has a row there; with > for >= it has none"""
    for name in ("noise10", "alias"):
        img, index = built[name]
        ctx, n = ec.edges(img, SEG)["at_p0"]
        chain = ec.chains_of(ec.events_of(img)[0])[ctx]
        j = chain[n][0] // SEG
        assert chain[n][0] == j * SEG and ctx in ic.rows_of(index, ic.Layout16(index), 0, j)[0]
        assert _differs(img, index, "gt")


def test_a_last_event_at_p0_minus_1(built):
    """(c) a context whose last event is at p0 - 1 has no row at p0; a rule that keeps every context with an event in front of p0 gives
    other bytes"""
    for name in ("noise12", "noise10"):
        img, index = built[name]
        ctx, p0 = ec.edges(img, SEG)["ends_before_p0"]
        assert ctx not in ic.rows_of(index, ic.Layout16(index), 0, p0 // SEG)[0]
        assert _differs(img, index, "live")


def test_crossings_in_lane_0_and_lane_63(built):
    """(d) crossing events whose index in their chain is = 0 and = 63 mod 64, in chains of several hundred events; the counters after
    the event instead of before it give other bytes"""
    for name, key in (("few_a", "lane0"), ("few_b", "lane63")):
        img, index = built[name]
        got = ec.edges(img, SEG)
        assert got[key] and got["chains_over_300"], (name, got)
        ctx, n = got[key]
        assert n % 64 == (0 if key == "lane0" else 63) and n >= 63
        assert len(ec.chains_of(ec.events_of(img)[0])) <= 8  # a handful of contexts
        assert _differs(img, index, "after")


def test_halvings_at_a_crossing(built):
    """(e) a halving on the event immediately before a crossing event; two halvings in the 64-event block that holds a crossing"""
    img, index = built["big_a"]
    ctx, n = ec.edges(img, SEG)["halve_before"]
    chain = ec.chains_of(ec.events_of(img)[0])[ctx]
    assert chain[n - 1][4] and chain[n][2] == [v >> 1 for v in (a + (chain[n - 1][1] >> k) + 1 + k for k, a in enumerate(chain[n - 1][2]))]
    assert _differs(img, index, "after")
    img, index = built["big_b"]
    ctx, n = ec.edges(img, SEG)["two_halvings"]
    chain = ec.chains_of(ec.events_of(img)[0])[ctx]
    assert sum(1 for c in chain[n // 64 * 64:n // 64 * 64 + 64] if c[4]) >= 2
    assert _differs(img, index, "after")


def test_chroma_and_row_counts(built):
    """(f) a chroma row with a context >= 65 536; (g) a checkpoint with more than 512 rows and checkpoints with none"""
    img, index = built["chroma"]
    lay = ic.Layout16(index)
    assert max(int(ic.rows_of(index, lay, c, j)[0].max(initial=0)) for c in (1, 2) for j in range(lay.k)) >= 65536
    assert max(ic.Layout16(built["noise12"][1]).n_rows()) > 512
    assert set(ic.Layout16(built["flat"][1]).n_rows()) == {0}
