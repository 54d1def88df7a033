"""The corpus of decode_cases.py, checked on the CPU: the estimator model gives the oracle's k for every Rice event, the corpus
reaches every edge of REQUIRED under the committed placement -- so test_decode_edges_gpu.py, which decodes these streams at those
addresses, is known to exercise those branches --, the threshold and tie edges are sensitive to the rule they are about, and the
library's host decoder agrees with the oracle on every corpus stream and every corrupt variant."""
import numpy as np
import pytest

from tests import decode_cases as dc


@pytest.mark.parametrize("kind", dc.KINDS)
def test_model_reproduces_the_traced_k(kind):
    frames = dc.of_kind(kind)
    assert frames
    for f in frames:
        dc.model_matches_trace(f)
        assert len(f.model()) == (3 if kind.startswith("rgb") else 1)


def test_corpus_holds_the_three_case_modules():
    from tests import chain_cases, pack_layout, wide_cases

    want = sum(len(mod.case(n).frames) for mod in (pack_layout, wide_cases, chain_cases) for n in mod.NAMES)
    old = [f for f in dc.corpus() if not f.case.startswith("new:")]
    assert len(old) == want and len({f.key for f in dc.corpus()}) == len(dc.corpus())
    assert max(f.w * f.h for f in dc.corpus()) <= 65536
    # the frames no GPU form takes (rows wider than k_decode16's LDS holds): the two of wide_cases' "starts", and no new one
    assert [f.key for f in dc.corpus() if not f.on_gpu] == ["wide:starts[0]", "wide:starts[1]"]


def test_placement_gives_every_stream_every_address():
    for f in dc.corpus():
        assert sorted(dc.placement(f.case, f.index, r) for r in dc.ROTATIONS) == [0, 1, 2, 3], f.key
    frames = dc.corpus()[:9]
    for rot in dc.ROTATIONS:
        blob, offs, lens = dc.place(frames, [bytes([i]) * (20 + i) for i in range(9)], rot)
        assert [o & 3 for o in offs] == [dc.placement(f.case, f.index, rot) for f in frames]
        assert all(a + n <= b for a, n, b in zip(offs, lens, offs[1:])) and offs[-1] + lens[-1] + 16 == len(blob)
        assert all(blob[o:o + n] == bytes([i]) * n for i, (o, n) in enumerate(zip(offs, lens)))


def test_grids_by_hand():
    """A stream at a multiple of 4: its payload starts two bytes into a dword, so bit 112 lies at bit 16 of grid p14; at address 2 the
    payload is aligned.  total_dw: 256 payload bytes behind a skew of 2 are 65 dwords."""
    assert [dc.shift_of("p14", a) for a in range(4)] == [16 - 112, 24 - 112, -112, 8 - 112]
    assert [dc.shift_of("s", a) for a in range(4)] == [0, 8, 16, 24]
    assert dc.total_dw("p14", 0, 14 + 256) == 65 and dc.total_dw("p14", 2, 14 + 256) == 64 and dc.total_dw("s", 3, 253) == 64


def test_required_is_reached():
    miss = dc.missing(dc.corpus())
    assert not miss, "not reached (kind, reader, address, edge): %s" % miss
    # every name of REQUIRED is one reached() can give
    known = set().union(*(dc.reached(f, a) for f in dc.corpus() for a in range(4)))
    assert set().union(*dc.REQUIRED.values()) <= known


@pytest.mark.parametrize("kind", dc.KINDS)
def test_threshold_edges_are_sensitive(oracle, kind):
    """For an update that leaves the minimum at exactly 1024 (exactly 1025): the context's events replayed by the oracle's own
    estimator with the threshold at 1024 give the traced k, and with 1023 (1025) another sequence."""
    nk = dc.NK[kind]
    for name, _, thr in dc.THRESHOLD_EDGES:
        frame = next(f for f in dc.of_kind(kind) if f.on_gpu and name in dc.reached(f, 0))
        found = False
        for p, mdl in enumerate(frame.model()):
            _, ctx, ev, tk = frame.events(p)
            for x in np.unique(ctx[(mdl["mn"] == 1024) | (mdl["mn"] == 1025)]):
                es, true = ev[ctx == x], tk[ctx == x].tolist()
                if name not in dc.threshold_edges(es, nk, true):
                    continue
                found = True
                seqs = {}
                for at in (1024, thr):
                    est = oracle.estimator(0, list(range(nk)), at)
                    seqs[at] = []
                    for e in es:
                        seqs[at].append(est.get_k(0))
                        est.update(0, int(e))
                assert seqs[1024] == true and seqs[thr] != true, (frame.key, p, int(x), name)
        assert found, (kind, name)


@pytest.mark.parametrize("kind", dc.KINDS)
def test_ties_are_sensitive(kind):
    """A tie between counters that are not zero where the smallest k instead of the largest changes the code's length."""
    frame = next(f for f in dc.of_kind(kind) if f.on_gpu and "est:tie" in dc.reached(f, 0))
    hits = 0
    for p, mdl in enumerate(frame.model()):
        _, _, ev, tk = frame.events(p)
        i = np.flatnonzero((mdl["small"] != mdl["k"]) & ((ev >> mdl["small"]) + mdl["small"] != (ev >> mdl["k"]) + mdl["k"]))
        assert (mdl["k"][i] == tk[i]).all() and (mdl["small"][i] < tk[i]).all()
        hits += len(i)
    assert hits


def _both(api, oracle, stream):
    """(the host decoder's pixels or its code, the oracle's pixels or None)"""
    import felics_amd

    try:
        got = api.decompress_bytes(stream)
    except felics_amd.DecompressionError as e:
        got = e.code
    try:
        want = oracle.decompress(stream)
    except Exception:
        want = None
    return got, want


@pytest.mark.parametrize("kind", dc.KINDS)
def test_host_decoder_and_oracle_on_the_corpus(oracle, kind):
    from felics_amd import api

    for f in dc.of_kind(kind):
        stream = oracle.compress(f.img)
        assert len(stream) == f.layout().total_bytes(), f.key
        got, want = _both(api, oracle, stream)
        assert want is not None and (want == f.img).all() and want.dtype == f.img.dtype, f.key
        assert not isinstance(got, int) and got.dtype == f.img.dtype and (got == f.img).all(), f.key


@pytest.mark.parametrize("kind", dc.KINDS)
def test_host_decoder_and_oracle_on_the_variants(oracle, kind):
    """Both accept or both reject every variant, with the same pixels where they accept; the tails are rejected with the one code
    their operand asks for: -2 just above the bound, -3 above 2^32."""
    from felics_amd import api

    frames = dc.variant_frames(kind)
    assert frames
    for f in frames:
        stream = oracle.compress(f.img)
        for a in range(4):
            names = set()
            for name, v in dc.variants(f, stream, a):
                names.add(name)
                got, want = _both(api, oracle, v)
                assert isinstance(got, int) == (want is None), (f.key, a, name, got)
                if want is not None:
                    assert (got == want).all(), (f.key, a, name)
                if name.startswith("tail"):
                    assert got == (-3 if name == "tail-2^32" else -2), (f.key, name, got)
                if name.startswith("cut"):
                    assert want is None and got == -1, (f.key, name, got)
            assert names >= {"cut-1", "cut-run", "cut-chunk-p14", "cut-chunk-s", "tail-limit"} | ({"tail-2^32"} if dc.depth_of(kind) == 16 else set()), names
