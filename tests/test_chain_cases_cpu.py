"""The cases of chain_cases.py, checked on the CPU: every case reaches what it claims (from the oracle's trace and the model of the
tile-local layout alone), the plain Python replay of the estimator gives the oracle's k for every chain of every case, and every
mutated replay a case names changes a k of its chain behind the place it is aimed at -- so test_chain_replay_gpu.py, which
byte-compares these frames with the oracle, would fail on kernels that halved at >= 1024, or an event late, or broke ties the
other way, or took two events in the other order, or counted a short record's padding, or lost a window's carry or a slice's
chain_state.  The whole file takes about 5 s, the trace and the checks of `enum_chunk` (16.8 MPix) 0.7 s of them."""
import numpy as np
import pytest

from tests import chain_cases as cc


@pytest.mark.parametrize("name", cc.NAMES + cc.LARGE)
def test_premises(name):
    c = cc.case(name)
    assert c.claims and c.target, name
    cc.premises(c)


@pytest.mark.parametrize("name", cc.NAMES + cc.LARGE)
def test_mutated_rules_show_in_the_target_chain(name):
    cc.sensitivity(cc.case(name))


@pytest.mark.parametrize("name", cc.NAMES + cc.LARGE)
def test_replay_equals_oracle(name):
    cc.replay_matches_oracle(cc.case(name))


def test_every_rule_and_every_slice_count_has_a_case():
    cases = [cc.case(n) for n in cc.NAMES]
    assert {r for c in cases for r in c.rules} == set(cc.RULES) - {"reset"}
    assert all(any(claim[0] in ("reset-shows", "slice-resets") for claim in c.claims) for c in cases + [cc.case(n) for n in cc.LARGE])
    assert tuple(c.name for c in cases if c.overflows) == cc.OVERFLOWING
    assert set(cc.SLICE_COUNTS) <= {ns for c in cases for ns in c.slices}
    assert all(f.size < 40000 for c in cases for f in c.frames[:1] if not c.rgb) and all(f.size < 3 * 40000 for c in cases for f in c.frames[:1])


def test_chain_frame8_gives_the_wanted_events():
    """9000 values in 0 .. 119 at context 3: the second row's events are exactly those, in order, all of context 3, in tiles 2, 3 and 4
    of five; every other event is a by-product in the first row (some of context 3 too: in front of the made-to-order ones in raster
    order, so the chain's tail is the list)."""
    es = np.random.default_rng(1).integers(0, 120, size=9000)
    w = 9002
    ev = cc.events(cc.chain_frame8([(3, es)], w).astype(np.int32), w, 2)
    second = ev["pix"] >= w
    assert (ev["pix"][second] == w + 2 + np.arange(9000)).all() and (ev["ctx"][second] == 3).all()
    assert ev["val"][second].tolist() == es.tolist()
    assert cc.Chain(ev, cc.run_table(ev, 256), 3).es[-9000:].tolist() == es.tolist()
    assert np.bincount(ev["pix"][second] // cc.TILE).tolist() == [0, 0, 3 * cc.TILE - w - 2, cc.TILE, 9000 - (3 * cc.TILE - w - 2) - cc.TILE]


def test_replay_rules_on_a_worked_example():
    """By hand: e = 1 leaves counters 0 and 1 tied at 2, so the next k is 1 (0 with ties to the smallest); 1025 events of e = 0 lift
    counter 0 to 1025, the first halving (one earlier at >= 1024), and the next comes 513 events later; a record of one event
    padded to 16 halves in its padding; a state zeroed in front of record 1 gives k = 5 there."""
    assert cc.replay([1, 0]) == [5, 1] and cc.replay([1, 0], "small") == [0, 0]
    for rule, want in (("true", [1024, 1537]), ("ge", [1023, 1535]), ("late", [1025, 1538]), ("none", [])):
        hv = cc.halvings_of(np.zeros(1600, np.int64), rule=rule)
        assert hv[:2] == want, (rule, hv)
    sizes = [cc.REC] * 96 + [1, cc.REC]  # (slot 1024 is the first of record 64; slot 1537 the second of record 96, which holds one event)
    assert cc.halvings_of(np.zeros(1553, np.int64), rule="pad", recs=sizes) == [1024, -1 - 96]
    assert cc.replay([0] * 40, "reset", at=1, recs=[cc.REC, cc.REC, 8])[15:18] == [0, 5, 0]


def test_layout_model_on_a_worked_example():
    """Runs of 0, 17, 0, 40 and 16 events in five tiles: records (1, 16) (1, 1) (3, 16) (3, 16) (3, 8) (4, 16); under five slices the
    chain has records in slices 1, 3 and 4; event 17 is event 0 of the first record of slice 3; two slices are [0, 2) and [2, 5)."""
    row = np.array([0, 17, 0, 40, 16])
    assert cc.chain_records(row) == [(1, 16), (1, 1), (3, 16), (3, 16), (3, 8), (4, 16)]
    assert cc.launch_records(row, 5) == [0, 2, 0, 3, 1] and cc.launch_records(row, 2) == [2, 4] and cc.launch_records(row, 12).count(0) == 9
    assert cc.locate(row, 17, 5) == (3, 0, 0, 0, 16) and cc.locate(row, 16, 5) == (1, 0, 1, 0, 1) and cc.locate(row, 57, 1) == (0, 0, 5, 0, 16)
    assert cc.first_record_of_slices(row, 5) == [2, 5] and cc.first_record_of_slices(row, 2) == [2] and cc.slice_bounds(5, 12)[:5] == [0, 0, 0, 1, 1]
    assert cc.tile_slots(np.array([[0, 17, 0, 40, 16], [1, 0, 0, 16, 0]])).tolist() == [16, 32, 0, 64, 16]
