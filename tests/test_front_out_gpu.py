"""k_front's out stage at its edges (tests/front_out_cases.py; the CPU suite proves that the frames reach them): every frame of the
corpus through the same-shape call, the mixed-shape call and a pitched view (a surface one pixel wider than the frame), gray8 and
RGB8, every stream byte-compared with the CPU oracle -- there is no tolerance anywhere.  The workspace is poisoned before every
submission (FELICS_POISON), so a slot the stage should have written and did not shows as garbage downstream.  No redo of any kind
happens except where a case forces one: the two frames with a tile past the default cap, and the test contexts below."""
import os

import numpy as np
import pytest

from tests import front_out_cases as fo

pytestmark = pytest.mark.gpu


def _encoder(**env):
    import felics_amd

    env = dict(env, FELICS_POISON="1")  # (read when the context is created)
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return felics_amd.Encoder(0)
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


@pytest.fixture(scope="module")
def corpus(oracle):
    """[(name, frame, the oracle's stream)], computed once for the whole file."""
    return [(name, f, oracle.compress(f)) for name, (f, _) in fo.frames().items()]


def _same(got, want, names, what):
    assert len(got) == len(want)
    for g, w, name in zip(got, want, names):
        if g != w:
            n = min(len(g), len(w))
            diff = next((j for j in range(n) if g[j] != w[j]), n)
            raise AssertionError("%s, %s: differs from the oracle at byte %d (sizes %d vs %d)" % (what, name, diff, len(g), len(w)))


def _same_shape(e, chosen, what):
    groups = {}
    for name, f, want in chosen:
        groups.setdefault((f.shape, name in fo.OVERFLOWING), []).append((name, f, want))
    for group in groups.values():
        _same(e.compress_batch([f for _, f, _ in group]), [w for _, _, w in group], [n for n, _, _ in group], what)


def _mixed(e, chosen, what):
    _same(e.compress_images([f for _, f, _ in chosen]), [w for _, _, w in chosen], [n for n, _, _ in chosen], what)


def _pitched(e, chosen, what):
    import torch

    views = []
    for i, (_, f, _) in enumerate(chosen):
        h, w = f.shape[:2]
        surface = torch.full((h, w + 1) + f.shape[2:], 37 + i % 200, dtype=torch.uint8, device="cuda")  # (rows w + 1 pixels apart)
        surface[:, :w] = torch.from_numpy(f).cuda()
        views.append(surface[:, :w])
    cap = sum(2 * v.numel() + 4096 for v in views)
    d_out = torch.empty(cap, dtype=torch.uint8, device="cuda")
    offs, lens = e.compress_arrays_device(views, d_out.data_ptr(), cap)
    torch.cuda.synchronize()
    host = d_out.cpu().numpy()
    _same([host[int(o):int(o) + int(l)].tobytes() for o, l in zip(offs, lens)], [w for _, _, w in chosen], [n for n, _, _ in chosen], what)


CALLS = {"same-shape": _same_shape, "mixed": _mixed, "pitched": _pitched}
QUIET = ("scatter_fallbacks", "tile_overflows", "lookback_fallbacks")


@pytest.mark.parametrize("call", sorted(CALLS))
def test_corpus_without_a_redo(corpus, call):
    """Every frame whose tiles fit the default cap: equal streams, and nothing was redone."""
    e = _encoder()
    try:
        CALLS[call](e, [c for c in corpus if c[0] not in fo.OVERFLOWING], call)
        st = e.stats()
        assert all(st[k] == 0 for k in QUIET), st
    finally:
        e.close()


@pytest.mark.parametrize("call", sorted(CALLS))
def test_tiles_past_the_default_cap(corpus, call):
    """The frames with a tile past the default cap -- one record past it, and the fullest tiles a plane can hold (7920 of 7936 slots,
    11744 of 11776) --, each alone in a context of its own: exactly one overflow, the frame again at the worst-case cap, equal streams."""
    for c in corpus:
        if c[0] in fo.OVERFLOWING:
            e = _encoder()
            try:
                CALLS[call](e, [c], call)
                st = e.stats()
                assert st["tile_overflows"] == 1 and st["scatter_fallbacks"] == 0 and st["lookback_fallbacks"] == 0, (c[0], st)
            finally:
                e.close()


def _edge_frames(corpus):
    """One frame an edge, gray8 and RGB8: what the forced cases run."""
    pick = ("runs_16_32", "runs_16_32_co", "slots_4080", "slots_4096", "slots_4096_co", "slots_4112_in_run", "slots_4112_between_co", "one_61x67",
            "constant_64x64", "noise_80x60", "noise_rgb_64x65", "cap_fits_0", "cap_co_fits_0")
    by = {c[0]: c for c in corpus}
    return [by[n] for n in pick]


@pytest.mark.parametrize("call", sorted(CALLS))
def test_ranks_from_ballots(corpus, call):
    """FELICS_SCATTER=ballot: the other rank form's instantiations, equal streams, no redo."""
    e = _encoder(FELICS_SCATTER="ballot")
    try:
        CALLS[call](e, _edge_frames(corpus), call + ", ballots")
        st = e.stats()
        assert all(st[k] == 0 for k in QUIET), st
    finally:
        e.close()


def _one_batch(corpus, kind):
    """The made-to-order frames of one type."""
    pick = {"gray8": ("runs_16_32", "slots_4080", "slots_4096", "slots_4112_in_run", "slots_4112_between", "cap_fits_0", "worst_case"),
            "rgb8": ("runs_16_32_co", "slots_4080_co", "slots_4096_co", "slots_4112_in_run_co", "slots_4112_between_co", "cap_co_fits_0", "worst_case_co")}[kind]
    by = {c[0]: c for c in corpus}
    return [by[n] for n in pick]


def _forced(corpus, kind, env, counter):
    """Every made-to-order frame alone in a context of its own under `env` (a batch of several frames is cut into sub-batches, each
    with a redo of its own): equal streams, `counter` exactly 1, the other two 0."""
    for c in _one_batch(corpus, kind):
        if counter != "tile_overflows" and c[0] in fo.OVERFLOWING:
            continue  # (the fullest tiles overflow the default cap by themselves: theirs is the forced-cap case)
        e = _encoder(**{env: "1"})
        try:
            _same_shape(e, [c], env)
            st = e.stats()
            assert all(st[k] == (1 if k == counter else 0) for k in QUIET), (c[0], st)
        finally:
            e.close()


@pytest.mark.parametrize("kind", ["gray8", "rgb8"])
def test_forced_order_violation_is_one_fallback(corpus, kind):
    """FELICS_TEST_SCATTER_ORDER: k_front reports a violation whatever it produced -- exactly one fallback, equal streams."""
    _forced(corpus, kind, "FELICS_TEST_SCATTER_ORDER", "scatter_fallbacks")


@pytest.mark.parametrize("kind", ["gray8", "rgb8"])
def test_forced_small_cap_is_one_overflow(corpus, kind):
    """FELICS_TEST_TILE_CAP: the first attempt runs with a tiny cap -- one overflow, the batch again at the worst-case cap."""
    _forced(corpus, kind, "FELICS_TEST_TILE_CAP", "tile_overflows")
