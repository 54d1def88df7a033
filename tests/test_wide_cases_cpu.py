"""The cases of wide_cases.py, checked on the CPU: every case reaches the edges it claims (from the oracle's trace alone), the plain
Python replay of the estimator gives the oracle's k for every chain of every case, and every case aimed at a replay rule tells that
rule from its mutation -- so test_wide_replay_gpu.py, which byte-compares these frames with the oracle, would fail on a kernel
that halved at >= 1024, or an event late, or broke ties the other way, or sorted the events unstably."""
import numpy as np
import pytest

from tests import wide_cases as wc


@pytest.mark.parametrize("name", wc.NAMES)
def test_premises(name):
    c = wc.case(name)
    assert c.edges, name
    wc.premises(c)


@pytest.mark.parametrize("name", wc.NAMES)
def test_replay_equals_oracle(name):
    wc.replay_matches_oracle(wc.case(name))


def test_every_edge_has_a_case():
    claimed = {e for n in wc.NAMES for e in wc.case(n).edges}
    assert claimed == set(wc.EDGES), (sorted(set(wc.EDGES) - claimed), sorted(claimed - set(wc.EDGES)))


def test_single_chain_and_checkerboard_halvings():
    """The halvings worked out by hand for the plain constructions; their values never change, so no rule shows in their k (which
    is why the replay rules are pinned by the `dense` case instead)."""
    for frame, want in ((0, [1024, 1537]), (2, [341, 512, 683])):
        ev = wc.case("single").trace()[frame]
        assert len(ev["chain_len"]) == 1 and ev["chain_len"][0] == 1600
        hv = []
        wc.replay(ev["val"], halvings=hv)
        assert hv[:len(want)] == want, hv
    ev = wc.case("checker").trace()[0]
    assert ev["chain_ctx"].tolist() == [0] and ev["chain_len"].tolist() == [2457]
    hv = []
    wc.replay(ev["val"], halvings=hv)
    assert hv[:3] == [56, 85, 114], hv
    assert wc.replay(ev["val"], "late") == wc.replay(ev["val"])


def test_mutated_rules_show_in_the_target_chain():
    """Every mutation of the replay changes a k of the dense chain behind its first event, each late halving the limits aim at
    changes one by itself, and exchanging two neighbours of the few-level chain does."""
    c = wc.case("dense")
    es, k = c.target_values()
    true = wc.replay(es)
    assert true == k.tolist()
    for rule in wc.RULES:
        got = wc.replay(es, rule)
        assert got[0] == true[0] or rule == "small"
        assert got[1:] != true[1:], rule
    hv = c.target_halvings()
    aimed = [h for h in hv if h in c.limits]
    assert aimed and all(wc.late_shows(es, h) for h in aimed), (aimed, c.limits)
    assert wc.stability_pair(wc.case("levels")) is not None


def test_replay_rules_on_a_worked_example():
    """Two events by hand: e = 1 leaves counters 0 and 1 tied at 2, so the next k is 1 (0 with ties to the smallest); 1025 events of
    e = 0 lift counter 0 to 1025, the first halving (one earlier at >= 1024)."""
    assert wc.replay([1, 0]) == [14, 1] and wc.replay([1, 0], "small") == [0, 0]
    for rule, want in (("true", [1024]), ("ge", [1023]), ("late", [1025]), ("none", [])):
        hv = []
        wc.replay(np.zeros(1030, np.int64), rule, halvings=hv)
        assert hv[:1] == want, (rule, hv)
