"""What the tests of k_front's out stage share (test_front_out_cases_cpu.py, test_front_out_gpu.py): small frames whose tiles reach the
edges the stage branches on, and the proof of each from the CPU oracle's trace alone -- the GPU test uses nothing that the CPU test
has not proved.

k_front sorts a tile's events by context into SLOTS: contexts ascending, every context's run rounded up to whole records of 16, the
slots behind a run's last event padding (pix = 0xFFFF).  A tile of at most 4096 slots lies in LDS in slot order and goes out four
slots a store, 1024 a pass of the workgroup; a larger one (noise, the made-to-order tiles below) keeps the events' order in LDS and
the narrow stores.  The edges:
  no-event          a tile without an event (no slot in use)
  one-event         a tile with one event: 15 padding slots behind it
  run-16, run-32    a run of exactly 16 / 32 events with the next context's run directly behind it (no padding between them)
  slots-4080, slots-4096, slots-4112
                    slots in use one record short of the LDS image, exactly it, one record more (the first tile that is `large`)
  boundary-in-run   slot 4096 inside a run         boundary-between-runs   slot 4096 the first slot of a run
  pass-in-run       a pass boundary (slot 1024, 2048 or 3072) inside a run, its neighbours events of one context
  noise             a tile of noise: more than 4096 slots
  default-cap       slots in use exactly the default cap (6144 gray, 8192 for a plane of RGB), and one record more (cap_* of
                    chain_cases)
  worst-case        the fullest tile a plane can hold: every pixel an event, every context that can have an event one past whole
                    records.  That is 7920 slots of the worst-case cap 7936 for gray8 and 11744 of 11776 for a plane of RGB8, not the
                    caps themselves (largest_tile below): the caps count 256 / 512 contexts, but a sample outside [L, H] needs
                    H - L <= 254 (the samples span 0 .. 255) or <= 509 (Co spans -255 .. 255), so 255 / 510 contexts can hold events;
                    and 4096 events over them, each run 1 mod 16, leave a remainder -- 4096 - 255 = 16 * 240 + 1, 4096 - 510 =
                    16 * 224 + 2 -- that costs one / two padding slots, and slots come in sixteens.  The frames overflow the default
                    cap, so the encoder runs them again at the worst-case cap, which they fill but for 16 / 32 slots.
  short-last-tile   a plane's last tile is not full"""
import numpy as np

from tests import chain_cases as cc
from tests.chain_cases import REC, TILE, Row, co_row, gray_frame, rgb_frame
from tests.wide_cases import planes_of

WINDOW = 4096
SHAPES = ((64, 64), (64, 65), (80, 60), (61, 67))   # (W, H): one tile; a tile and a row; two tiles, the last short; a short tile


def _content(kind, rng, w, h):
    y, x = np.mgrid[0:h, 0:w]
    if kind == "constant":
        return np.full((h, w), 90, np.uint8)
    if kind == "one":       # one sample above a flat plane, in the plane's last tile: the only event of the frame
        f = np.full((h, w), 90, np.uint8)
        f[h - 1, w // 2] = 140
        return f
    if kind == "noise":
        return rng.integers(0, 256, size=(h, w)).astype(np.uint8)
    if kind == "ramp":      # a ramp with a little noise: few events among pixels in range
        return (((x + y) // 2 + rng.integers(0, 2, size=(h, w))) % 256).astype(np.uint8)
    raise ValueError(kind)


def _runs(counts, rgb=False):
    """A two-row frame (4096 x 2) whose second row -- tile 1 of the plane (gray) or of the Co plane (RGB) -- holds runs of counts[c]
    events of context c and nothing else."""
    row = cc._one_past_row(co_row(TILE) if rgb else Row(TILE, start=100), counts)
    return rgb_frame(row) if rgb else gray_frame(row)


# name -> (counts of tile 1, the claims about (plane, tile 1))
_BASE = [48] * 84 + [33]   # 4080 slots from 4065 events (a row holds 4094 made-to-order pixels)
_RUNS = {
    "runs_16_32": ([16, 32, 5, 16, 3], ("run-16", "run-32")),
    "slots_4080": (_BASE, ("slots-4080", "pass-in-run")),
    "slots_4096": (_BASE + [1], ("slots-4096", "pass-in-run")),
    "slots_4112_between": (_BASE + [16, 5], ("slots-4112", "boundary-between-runs")),
    "slots_4112_in_run": (_BASE + [20], ("slots-4112", "boundary-in-run")),
}

def largest_tile(contexts, pixels=TILE):
    """The most slots a tile of `pixels` events can use when `contexts` contexts can hold events: the padding, at most 15 a context,
    is what makes pixels + padding a multiple of 16."""
    return (pixels + 15 * contexts) // REC * REC


def worst_counts(contexts, pixels=TILE):
    """Events per context 0 .. contexts - 1 of a tile that reaches largest_tile: one event each, whole pairs of records more for the
    low contexts (any neighbourhood can produce those), the remainder on context 0."""
    n = np.ones(contexts, np.int64)
    extra, rest = divmod(pixels - contexts, REC)
    n[:extra // 2] += 2 * REC
    n[0] += (extra % 2) * REC + rest
    assert n.sum() == pixels and int((-(-n // REC) * REC).sum()) == largest_tile(contexts, pixels)
    return n


def _worst(rgb=False):
    """A two-row frame 8192 wide whose second row's second half -- tile 3 of the plane (gray) or of the Co plane (RGB) -- is 4096
    events with worst_counts per context.  The events come in no order of contexts: at every pixel the highest context that still
    lacks events and that the sample to the left allows (a context c needs a neighbour c away inside the samples' range, and a
    sample beyond both)."""
    row = co_row(2 * TILE) if rgb else Row(2 * TILE, start=254)
    counts = worst_counts(510 if rgb else 255)
    row.to_tile(3)

    def allows(left, c):
        for above in (left + c, left - c):
            if row.lo <= above <= row.hi and (max(left, above) + 1 <= row.hi or min(left, above) - 1 >= row.lo):
                return True
        return False

    left_over = counts.copy()
    for _ in range(TILE):
        left = int(row.row[row.x - 1])
        c = next(c for c in range(len(left_over) - 1, -1, -1) if left_over[c] and allows(left, c))
        row.event(c, 0)
        left_over[c] -= 1
    assert row.x == row.w and not left_over.any()
    return rgb_frame(row) if rgb else gray_frame(row)


_FRAMES = None


def frames():
    """{name: (frame, claims)}: every frame of the corpus, gray8 and RGB8, built once."""
    global _FRAMES
    if _FRAMES is None:
        out = {}
        for w, h in SHAPES:
            rng = np.random.default_rng(w * 1000 + h)
            for kind, claims in (("constant", ("no-event",)), ("one", ("one-event",)), ("noise", ("noise",)), ("ramp", ())):
                f = _content(kind, rng, w, h)
                short = ("short-last-tile",) if (w * h) % TILE else ()
                out["%s_%dx%d" % (kind, w, h)] = (f, claims + short)
                if kind in ("one", "noise"):
                    g = np.stack([f, _content(kind, rng, w, h), np.roll(f, 1, axis=1)], axis=-1).copy()
                    out["%s_rgb_%dx%d" % (kind, w, h)] = (g, (claims if kind == "noise" else ()) + short)
        for name, (counts, claims) in _RUNS.items():
            out[name] = (_runs(counts), claims)
            out[name + "_co"] = (_runs(counts, rgb=True), claims)
        for name in ("cap_fits", "cap_over", "cap_co_fits", "cap_co_over", "word_path"):
            for i, f in enumerate(cc.case(name).frames):
                out["%s_%d" % (name, i)] = (f, ("default-cap",) if name.startswith("cap_") else ())
        out["worst_case"] = (_worst(), ("worst-case",))
        out["worst_case_co"] = (_worst(rgb=True), ("worst-case",))
        _FRAMES = out
    return _FRAMES


OVERFLOWING = ("cap_over_0", "cap_co_over_0", "worst_case", "worst_case_co")   # a tile outgrows the default cap: one redo of the batch, counted in tile_overflows


def run_tables(frame):
    """[plane] -> [context, tile] events of every run, from the oracle's trace."""
    h, w = frame.shape[:2]
    nctx = 256 if frame.ndim == 2 else 512
    return [cc.run_table(cc.events(p, w, h), nctx) for p in planes_of(frame)]


def tile_claims(tab, t, cap, contexts):
    """What tile t of a plane with run table `tab` reaches, as the set of edge names above."""
    n = tab[:, t]
    slots = int((-(-n // REC) * REC).sum())
    got = set()
    if slots == 0:
        got.add("no-event")
    if n.sum() == 1:
        got.add("one-event")
    got.add("slots-%d" % slots)
    if slots > WINDOW and (n > 0).sum() > 128:   # (most of the contexts in use, hundreds of part-filled records)
        got.add("noise")
    if slots in (cap, cap + REC):
        got.add("default-cap")
    if slots == largest_tile(contexts) and n.sum() == TILE and (n > 0).sum() == contexts and (n[:contexts] % REC != 0).all():
        got.add("worst-case")
    # the runs in slot order: (first slot, events) of every context with events
    first = np.cumsum(-(-n // REC) * REC) - (-(-n // REC) * REC)
    used = np.flatnonzero(n)
    for a, b in zip(used[:-1], used[1:]):
        if n[a] in (16, 32) and first[b] == first[a] + n[a]:
            got.add("run-%d" % n[a])
    for c in used:
        lo, hi = int(first[c]), int(first[c] + n[c])   # the run's events lie in slots [lo, hi)
        if slots > WINDOW and lo < WINDOW < hi:
            got.add("boundary-in-run")
        if slots > WINDOW and lo == WINDOW:
            got.add("boundary-between-runs")
        if slots <= WINDOW and any(lo < m < hi for m in (1024, 2048, 3072)):
            got.add("pass-in-run")
    return got


def reached(frame):
    """Every edge some tile of some plane of the frame reaches."""
    h, w = frame.shape[:2]
    tabs = run_tables(frame)
    cap = cc.CAP[256 if frame.ndim == 2 else 512]
    got = set()
    for tab in tabs:
        for t in range(tab.shape[1]):
            got |= tile_claims(tab, t, cap, 255 if frame.ndim == 2 else 510)
    if (w * h) % TILE:
        got.add("short-last-tile")
    return got


EDGES = ("no-event", "one-event", "run-16", "run-32", "slots-4080", "slots-4096", "slots-4112", "boundary-in-run", "boundary-between-runs",
         "pass-in-run", "noise", "default-cap", "worst-case", "short-last-tile")
