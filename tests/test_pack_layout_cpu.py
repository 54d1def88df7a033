"""The cases of pack_layout.py, checked on the CPU with the oracle alone: the layout model gives the oracle's stream length for every
frame, and every case reaches exactly the edges of the two-pass pack it claims -- window boundaries, runs, shared words, plane and
tile alignments, the slot cut -- so test_two_pass_pack.py, which byte-compares these frames with the oracle on the GPU, is known to
exercise those branches.  Nothing here imports the library under test."""
import numpy as np
import pytest

from tests import pack_layout as pl


@pytest.mark.parametrize("name", pl.NAMES)
def test_model_total_is_the_oracle_length(oracle, name):
    c = pl.case(name)
    for i, (f, L) in enumerate(zip(c.frames, c.layouts())):
        assert L.total_bytes() == len(oracle.compress(f)), (name, i, f.shape)
        assert L.tiles[0][0][0] == 0 and L.tiles[-1][-1][1] == L.total_bits
        flat = [x for p in range(L.nplanes) for x in L.tiles[p]]
        assert all(a[1] == b[0] for a, b in zip(flat, flat[1:])) and all(lo < hi for lo, hi in flat), (name, i)  # back to back, none empty


@pytest.mark.parametrize("name", pl.NAMES)
def test_case_reaches_what_it_claims(name):
    c = pl.case(name)
    got = c.reached()
    assert c.edges and got == c.edges, (name, "not reached", sorted(c.edges - got), "reached and not claimed", sorted(got - c.edges))


def test_every_edge_has_a_case():
    for names in (pl.NAMES, pl.NAMES16):
        claimed = set().union(*(pl.case(n).edges for n in names))
        missing = set(pl.EDGES) - claimed
        assert missing == (set() if names is pl.NAMES else {"u16:group-max"}), sorted(missing)
    # the 8-bit instantiations see every edge of the shared words and both sweeps too
    claimed8 = set().union(*(pl.case(n).edges for n in pl.NAMES8))
    assert claimed8 >= set(pl.SWEEP_EDGES_RGB) | set(pl.SHARED_EDGES) | {"u16:group-max"}


def test_flat_layout_by_hand(oracle):
    """The figures worked out by hand: a flat gray16 frame of 4096 + r pixels has a tile 0 of 112 + 64 + 4094 = 4270 bits and a tile 1
    of r bits from bit 14 of a word; in the flat RGB16 frame of 4101 pixels planes 1 and 2 start at bits 19 and 22 and all three last
    tiles lie in one word."""
    for w, h, r in ((3, 1367, 5), (11, 374, 18), (4127, 1, 31)):
        L = pl.layout(oracle, pl.flat(w, h))
        assert [hi - lo for lo, hi in L.tiles[0]] == [4270, r] and L.start_bit(0, 1) == 14
        assert L.in_one_word(0, 1) == (r <= 18)
    L = pl.layout(oracle, pl.flat(3, 1367, rgb=True))
    assert [L.plane_lo[p] & 31 for p in (1, 2)] == [19, 22]
    assert all(L.in_one_word(p, 1) for p in range(3))
    assert L.words(0, 0)[1] == L.words(0, 1)[0] == L.words(1, 0)[0]  # three tiles write that word


def test_long_codes_by_hand(oracle):
    """The trace of the long codes: the gray16 spike is an event of context 0 (or 1) coded with k = 0, 64 537 (64 536) bits; the Co
    sample of the RGB16 frames is value 131 069 in context 0, 2^17 bits with k = 0 -- its run begins in window 0 of its tile,
    covers window 1 and ends in window 2 -- and 65 538 bits with k = 1, remainder 1."""
    L = pl.layout(oracle, pl.quiet16(pl.QW, pl.QH, spikes=[(1602, 0), (1606, 1)]))
    a, b = L.long_codes(0)
    assert (a, b) == (1602, 1606) and a // 16 == b // 16
    assert [(int(L.ctx[0][i]), int(L.k[0][i]), int(L.nbits[0][i])) for i in (a, b)] == [(0, 0, 64537), (1, 0, 64536)]
    c = pl.case("chroma16")
    for L, (k, nbits) in zip(c.layouts(), ((0, 1 << 17), (1, 65538))):
        (i,) = L.long_codes(1)
        assert (int(L.ctx[1][i]), int(L.val[1][i]), int(L.k[1][i]), int(L.nbits[1][i])) == (0, 131069, k, nbits)
    L = c.layouts()[0]
    rs, re = L.run(1, L.long_codes(1)[0])
    assert (L.window_of(1, 0, rs), L.window_of(1, 0, re - 1)) == (0, 2) and L.windows(1, 0) == 3


def test_longest_group_of_eight_bit_codes(oracle):
    """Sixteen chroma codes of 497 .. 512 bits (value 509, k = 0: the longest an 8-bit sample has) in one thread's group: the largest
    group total of the frame, 7 800 bits and more, and far below the 65 536 a 16-bit group total could not hold."""
    img, at = pl.chroma8_longest()
    L = pl.layout(oracle, img)
    nb = L.nbits[1][at:at + pl.GROUP]
    assert at % pl.GROUP == 0 and nb.max() == 2 + 509 + 1 and int((nb >= 497).sum()) >= 15, nb
    tot = np.concatenate([L.group_totals(p) for p in range(3)])
    assert tot.max() == L.group_totals(1)[at // pl.GROUP] and pl.U16_GROUP_MIN <= tot.max() < 65536, tot.max()


@pytest.mark.parametrize("name,frames,cap,reach", pl.cut_cases(), ids=[c[0] for c in pl.cut_cases()])
def test_slot_cut_cases(oracle, name, frames, cap, reach):
    """The last stream outgrows its fixed slot, the cut falls where the case says, and the streams fit the capacity back to back."""
    n, frame_bytes = len(frames), frames[0].nbytes
    slot = pl.device_slot(cap, n, frame_bytes)
    sizes = [len(oracle.compress(f)) for f in frames]
    assert slot > 0 and slot * n == cap and sizes[-1] > slot and all(s <= slot for s in sizes[:-1]), (slot, sizes)
    assert sum((s + 15) // 16 * 16 for s in sizes) <= cap
    assert pl.cut_reach(pl.layout(oracle, frames[-1]), slot) == reach


def test_mixed_sets_share_a_bucket():
    for name, imgs in pl.mixed_sets().items():
        t = [pl.tiles_of(im) for im in imgs]
        assert pl.one_bucket(imgs) and len({im.shape for im in imgs}) == len(imgs), (name, t)
        assert set(t) == ({1, 2} if name.endswith("1-2") else {2, 3}), (name, t)
        tiny = [im for im in imgs if im.shape[0] * im.shape[1] % pl.TILE == 5]
        assert tiny and min(t) < max(t), name  # a last real tile of five pixels; planes with padding tiles
        if name.endswith("2-3"):
            assert any(pl.tiles_of(im) < max(t) for im in tiny), name  # ... and a padding tile behind that tile
        assert all(im.nbytes + im.nbytes // 4 + 64 >= pl.Layout(im).total_bytes() for im in imgs), name  # (no stream outgrows its slot)
