"""The corpus of tests/front_out_cases.py reaches what it is for: every claim of every frame, and every edge of the list at least once
in a gray8 frame and -- where a plane of RGB8 can hold it -- in an RGB8 frame, proved from the CPU oracle's trace alone."""
from tests import front_out_cases as fo


def test_every_frame_reaches_its_claims(oracle):
    seen_gray, seen_rgb = set(), set()
    for name, (frame, claims) in fo.frames().items():
        got = fo.reached(frame)
        missing = [c for c in claims if c not in got]
        assert not missing, (name, missing, sorted(got))
        (seen_gray if frame.ndim == 2 else seen_rgb).update(c for c in claims)
    assert seen_gray >= set(fo.EDGES), sorted(set(fo.EDGES) - seen_gray)
    assert seen_rgb >= set(fo.EDGES) - {"no-event", "one-event"}, sorted(set(fo.EDGES) - seen_rgb)


def test_the_overflowing_frames_are_the_ones_listed(oracle):
    """A tile with more slots than the default cap in exactly the frames the GPU test expects an overflow redo for."""
    from tests import chain_cases as cc

    for name, (frame, _) in fo.frames().items():
        cap = cc.CAP[256 if frame.ndim == 2 else 512]
        over = any(int(cc.tile_slots(tab).max()) > cap for tab in fo.run_tables(frame))
        assert over == (name in fo.OVERFLOWING), (name, over)


def test_the_fullest_tile_is_short_of_the_worst_case_cap():
    """The arithmetic behind the `worst-case` edge: the caps the encoder falls back to count every context, 4096 + 15 * 256 and
    4096 + 15 * 512; a context can hold an event only if a sample fits beyond both neighbours -- H - L <= 254 of 0 .. 255, <= 509 of
    -255 .. 255 --, and the fullest tiles over those contexts are 16 and 32 slots short of the caps."""
    assert fo.largest_tile(256) == 7936 and fo.largest_tile(512) == 11776       # the caps: every context, were that possible
    assert fo.largest_tile(255) == 7920 and fo.largest_tile(510) == 11744       # what a tile can reach
    for contexts in (255, 510):
        n = fo.worst_counts(contexts)
        assert n.sum() == 4096 and (n % 16 != 0).all() and int((-(-n // 16) * 16).sum()) == fo.largest_tile(contexts)
