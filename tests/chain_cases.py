"""What the tests of the 8-bit chain stage share (test_chain_cases_cpu.py, test_chain_replay_gpu.py): frames built to reach the
boundaries felics_chain.hip branches on -- k_enum's records, k_spine3's windows, halvings and hand-overs, k_assign3's records in
tile order -- and the proof, from the CPU oracle alone, that each frame reaches what it is for and that a replay with a slightly
different rule would give other Rice parameters there.

A CHAIN is the events (samples outside [L, H], behind a plane's first two) of one context of one plane, in raster order.  The
kernels hold it in TILE-LOCAL layout, modelled here from the oracle's trace alone: a tile is 4096 consecutive pixels of a plane; a
tile's events of one context are a RUN, cut into RECORDS of 16 (the last one of a run may be short); a tile's slots are the sum
over its contexts of ceil(n / 16) * 16; a chain's records in chain order are its runs tile by tile; a WINDOW is 64 consecutive
records of a chain within one slice; slice q of ns covers the tiles [T q / ns, T (q + 1) / ns).  Indices count from 0.
A HALVING AT i: the counters are halved after event i of the chain (it lifted their minimum above 1024).

The frames come from seeded searches (aim, the seeds marked "searched"), so they depend on numpy's Generator streams; should those
change, a builder's own assertion or test_chain_cases_cpu.py fails -- on the CPU, with the claim that no longer holds -- and never
a kernel test with a wrong frame: the GPU tests use nothing that the CPU tests have not proved."""
import numpy as np

from tests import oracle_lib
from tests.wide_cases import planes_of, replay_records

NK, HALVE = 6, 1024
REC, TILE, WIN = 16, 4096, 64
CAP = {256: 6144, 512: 8192}     # a tile's slots by default, per number of contexts (gray8 / the planes of RGB8)
WORD_PATH_MAX_SLOTS = 2048       # k_pack_t: up to this many slots in use the codes are built per event
SP3_MULTI_MIN = 3                # k_spine3: from this many windows in a launch a chain gets a walker and a helper wave
RULES = ("ge", "late", "small", "none", "swap", "pad", "reset")


# ------------------------------------------------------------------------------------------------------------------------
# events and replay
# ------------------------------------------------------------------------------------------------------------------------

def events(plane, w, h):
    """The events of an 8-bit plane, from the oracle's trace: pixel index, context, coded value and k of each in raster order, the
    stable sort by context (`order`: a chain is a run of it) and every pixel's code length (`nbits`)."""
    tr = oracle_lib.load().trace_channel(plane, w, h, depth=0)
    pix = np.flatnonzero(tr["cls"] != 0)
    pix = pix[pix >= 2]
    ev = {"pix": pix, "ctx": tr["ctx"][pix].astype(np.int64), "val": tr["val"][pix].astype(np.int64), "k": tr["k"][pix].astype(np.int64),
          "nbits": tr["nbits"], "npix": w * h}
    ev["order"] = np.argsort(ev["ctx"], kind="stable")
    return ev


def replay(es, rule="true", at=None, halvings=None, recs=None, state=None):
    """k of every event of one chain with coded values es, replayed in plain Python: k is the argmin of the six counters with ties to
    the largest k; the event adds (e >> k) + 1 + k to counter k; all counters are halved after an event that lifts their minimum
    above 1024.  `halvings` receives the indices of the events that halved (-1 - r: a padding slot of record r did).  `state`: the
    counters to start from, left as they are behind the last event.
    The mutated rules: "ge" halves at a minimum >= 1024; "late" halves one event after the one that asked for it (at = i: only the
    halving at event i is late); "small" breaks ties towards the smallest k; "none" never halves; "swap" replays the chain with
    events at and at + 1 exchanged and gives k in the exchanged order; and, with recs = the events of every record of the chain:
    "pad" replays every short record's padding slots as events of value 0 (a record total taken over the padding); "reset" zeroes
    the counters in front of record `at` (a lost carry, a lost chain_state)."""
    es = [int(e) for e in es]
    if rule == "swap":
        es[at], es[at + 1] = es[at + 1], es[at]
    if recs is None:
        stream = [(e, i, False) for i, e in enumerate(es)]
    else:
        assert sum(recs) == len(es)
        stream, i = [], 0
        for r, n in enumerate(recs):
            for j in range(n):
                stream.append((es[i], i, rule == "reset" and r == at and j == 0))
                i += 1
            if rule == "pad":
                stream += [(0, -1 - r, False)] * (REC - n)
    S = [0] * NK if state is None else state
    out, owed = [], False
    for e, i, zero in stream:
        if zero:
            S[:] = [0] * NK
        if i >= 0:
            m = min(S)
            out.append(S.index(m) if rule == "small" else NK - 1 - S[::-1].index(m))
        S[:] = [s + (e >> k) + 1 + k for k, s in enumerate(S)]
        m = min(S)
        asks = (m >= HALVE if rule == "ge" else m > HALVE) and rule != "none"
        if owed:  # (the late halving: instead of this event's own question)
            asks, owed = True, False
        elif asks and rule == "late" and (at is None or at == i):
            asks, owed = False, True
        if asks:
            S[:] = [s >> 1 for s in S]
            if halvings is not None:
                halvings.append(i)
    return out


def halvings_of(es, **kw):
    hv = []
    replay(es, halvings=hv, **kw)
    return hv


def shows_at(es, h, horizon=150, start=0, state=None):
    """Does the halving at event h, an event late, change a k of the `horizon` events behind it, and does the exchange of events h and
    h + 1?  (start, state: the counters in front of event `start`, to replay from there.)"""
    e = [int(v) for v in es[start:h + horizon]]
    h -= start
    S = [0] * NK if state is None else state
    true = replay(e, state=list(S))
    late = replay(e, "late", at=h, state=list(S))
    swap = replay(e, "swap", at=h, state=list(S))
    swap[h], swap[h + 1] = swap[h + 1], swap[h]
    return e[h] != e[h + 1] and late != true and swap != true


def aim(es, at, rng, top=120, span=150, accept=None, quiet_end=False):
    """es with the events [at - span, at] drawn again -- values of one magnitude, then for the last thirty of another, so that the best k
    is on the move at the end -- and some of them raised or lowered until event `at` halves, and the 60 events behind it drawn
    again until shows_at holds for it and accept(es) does (values stay below `top`;
    quiet_end: the last thirty below 4, those before from 16 up); the events in front of them stay, and so do their halvings."""
    es = np.array(es, np.int64)
    lo = at - span
    assert lo >= 0 and at + 61 < len(es)
    S0 = [0] * NK
    replay(es[:lo], state=S0)
    win = es[lo:at + 1]  # (a view)
    bits = [b for b in range(9) if (1 << b) <= top]
    for _ in range(200):
        b1, b2 = (rng.choice(bits[4:]), rng.choice(bits[:3])) if quiet_end else rng.choice(bits, size=2, replace=False)
        win[:span - 30] = rng.integers(0, 1 << b1, size=span - 30)
        win[span - 30:] = rng.integers(0, 1 << b2, size=31)
        for _ in range(400):
            hv = []
            replay(win, halvings=hv, state=list(S0))
            near = [h for h in hv if h >= span - 40]
            if near and near[0] == span:
                for _ in range(10):
                    if shows_at(es, at, start=lo, state=S0) and (accept is None or accept(es)):
                        return es
                    es[at + 1:at + 61] = rng.integers(0, 1 << rng.choice(bits), size=60)
                break
            # too early: lower an event in front of the halving; too late, or not at all: raise one
            if near and near[0] < span:
                j = int(rng.integers(0, near[0] + 1))
                win[j] = max(0, win[j] - int(rng.integers(1, 40)))
            else:
                j = int(rng.integers(0, span + 1))
                win[j] = min(top - 1, win[j] + int(rng.integers(1, 40)))
    raise AssertionError("no halving at %d that shows" % at)


# ------------------------------------------------------------------------------------------------------------------------
# the tile-local layout
# ------------------------------------------------------------------------------------------------------------------------

def run_table(ev, nctx):
    """[context, tile]: the events of every run of a plane."""
    tiles = -(-ev["npix"] // TILE)
    tab = np.zeros((nctx, tiles), np.int64)
    np.add.at(tab, (ev["ctx"], ev["pix"] // TILE), 1)
    return tab


def tile_slots(tab):
    """The slots in use of every tile of a plane."""
    return (-(-tab // REC) * REC).sum(axis=0)


def chain_records(row):
    """(tile, events) of every record of the chain whose runs are `row`, in chain order."""
    out = []
    for t, n in enumerate(row):
        out += [(t, min(REC, int(n) - j)) for j in range(0, int(n), REC)]
    return out


def slice_bounds(tiles, ns):
    return [tiles * q // ns for q in range(ns + 1)]


def launch_records(row, ns):
    """The chain's records in every slice of ns (0: k_spine3 has nothing to walk for it there)."""
    b = slice_bounds(len(row), ns)
    per_tile = -(-np.asarray(row) // REC)
    return [int(per_tile[b[q]:b[q + 1]].sum()) for q in range(ns)]


def locate(row, i, ns):
    """Where event i of the chain whose runs are `row` lies under ns slices: (slice, window of the slice's launch, record of the
    window, event of the record, events of that record)."""
    recs = chain_records(row)
    b = slice_bounds(len(row), ns)
    r, left = 0, i
    while left >= recs[r][1]:
        left -= recs[r][1]
        r += 1
    tile = recs[r][0]
    q = next(q for q in range(ns) if b[q] <= tile < b[q + 1])
    first = next(j for j, (t, _) in enumerate(recs) if t >= b[q])  # the slice's first record of the chain
    return q, (r - first) // WIN, (r - first) % WIN, left, recs[r][1]


def first_record_of_slices(row, ns):
    """The chain records at which a slice of ns starts that holds some of the chain's (the chain's very first one left out)."""
    recs = chain_records(row)
    b = slice_bounds(len(row), ns)
    out = []
    for q in range(ns):
        inside = [j for j, (t, _) in enumerate(recs) if b[q] <= t < b[q + 1]]
        if inside and inside[0] > 0:
            out.append(inside[0])
    return out


# ------------------------------------------------------------------------------------------------------------------------
# constructions
# ------------------------------------------------------------------------------------------------------------------------

class Row:
    """The second row of a two-row plane of `width`, made to order from left to right: an event of any wanted context c and coded
    value e (the left neighbour is the pixel before, the one above is left +- c, the sample hi + 1 + e or lo - 1 - e, whichever
    stays in range), or pixels equal to both neighbours, which are no events.  The first row's own events are by-products in other
    contexts.  Pixel x of the row is pixel width + x of the plane: tile boundaries fall where `width` and the gaps put them."""

    def __init__(self, width, lo=0, hi=255, start=None):
        self.w, self.lo, self.hi = width, lo, hi
        self.above = np.zeros(width, np.int64)
        self.row = np.zeros(width, np.int64)
        self.row[0] = (lo + hi) // 2 if start is None else start
        self.above[0] = self.row[0]
        self.x = 1
        self.skip(1)  # (the first row begins L, L + 50: its third sample and the second row's first lie in range)

    def event(self, ctx, e):
        left, ctx, e = int(self.row[self.x - 1]), int(ctx), int(e)
        best = None
        for above in (left + ctx, left - ctx):
            if self.lo <= above <= self.hi:
                for p in (max(left, above) + 1 + e, min(left, above) - 1 - e):
                    if self.lo <= p <= self.hi and (best is None or abs(2 * p - self.lo - self.hi) < abs(2 * best[1] - self.lo - self.hi)):
                        best = (above, p)
        assert best is not None, "no sample for context %d, value %d beside %d" % (ctx, e, left)
        self.above[self.x], self.row[self.x] = best
        self.x += 1

    def events(self, ctx, es):
        for e in es:
            self.event(ctx, e)
        return self

    def skip_to(self, x):
        """pixels that are no events up to x (exclusive): equal to their left neighbours L; the ones above them L and L +- 50 in turn, so
        that the first row is not flat there (a flat stretch would make the first event behind it a by-product of context 0) and
        holds no events either (every sample equals the one two before it)"""
        assert self.x <= x <= self.w, (self.x, x)
        left = self.row[self.x - 1]
        self.row[self.x:x] = left
        self.above[self.x:x] = left + 50 * (np.arange(self.x, x) & 1) * (1 if 2 * left <= self.lo + self.hi else -1)
        self.x = x
        return self

    def skip(self, n):
        return self.skip_to(self.x + n)

    def to_tile(self, t):
        """... up to the first pixel of the plane's tile t"""
        return self.skip_to(t * TILE - self.w)

    def plane(self):
        self.skip_to(self.w)
        return np.stack([self.above, self.row])


def gray_frame(row):
    return row.plane().astype(np.uint8)


def co_row(width):
    return Row(width, -255, 255, 0)


def rgb_frame(row, g=128):
    """An RGB8 frame whose Co plane (r - b) is the made-to-order plane: r = max(co, 0), b = max(-co, 0), g constant; Y and Cg
    are by-products."""
    co = row.plane()
    return np.stack([np.maximum(co, 0), np.full_like(co, g), np.maximum(-co, 0)], axis=-1).astype(np.uint8)


def chain_frame8(segments, width):
    """A two-row gray8 frame whose second row is the event list segments = [(context, coded values), ...], padded to `width` with
    pixels that are no events."""
    r = Row(width)
    for ctx, es in segments:
        r.events(ctx, es)
    return gray_frame(r)


# ------------------------------------------------------------------------------------------------------------------------
# cases
# ------------------------------------------------------------------------------------------------------------------------

class Chain:
    """One chain of a case, from the oracle's trace: its coded values and k, its runs (events per tile) and records."""

    def __init__(self, ev, tab, ctx):
        sel = ev["ctx"] == ctx
        self.es, self.k, self.row = ev["val"][sel], ev["k"][sel].tolist(), tab[ctx]
        self.recs = chain_records(self.row)
        self.sizes = [n for _, n in self.recs]
        self._hv = None

    def halvings(self):
        if self._hv is None:
            self._hv = halvings_of(self.es)
        return self._hv

    def first_event(self, record):
        return sum(self.sizes[:record])

    def shows(self, rule, at=None, behind=0):
        """Does the mutated replay change a k of the chain at or behind event `behind`?"""
        got = replay(self.es, rule, at=at, recs=self.sizes if rule in ("pad", "reset") else None)
        if rule == "swap":
            got[at], got[at + 1] = got[at + 1], got[at]  # k by event, not by place
        return got[behind:] != self.k[behind:]


class Case:
    """frames: same-shaped 8-bit frames, one sub-batch in this order.  slices: the slice counts the blocking call runs it with.
    target: (frame, plane, context) of the chain the replay rules are checked on.  marks: the chain events the case is aimed at.
    claims: what the case says it reaches, each a tuple premises() proves from the oracle.  overflows: does a tile outgrow the
    default slots (predicted by the builder from the trace model, proved by premises()).  "reset" is claimed record by record, in
    every case: at the window starts and the slice starts inside the chain where it has some, and in the cap_* cases -- whose target
    is 41 records in one tile: no window start, no slice start behind its first record -- at a record boundary in the middle."""

    def __init__(self, name, frames, slices=(3,), target=None, marks=None, claims=(), overflows=False, pad=False):
        self.name, self.frames, self.slices, self.target = name, [np.ascontiguousarray(f) for f in frames], tuple(slices), target
        self.marks, self.claims, self.overflows = dict(marks or {}), list(claims), overflows
        self.rules = RULES[:5] + (("pad",) if pad else ())  # on the target ("pad": it holds a short record in front of further events)
        assert len({f.shape for f in self.frames}) == 1 and self.frames[0].dtype == np.uint8, name
        self.rgb = self.frames[0].ndim == 3
        self.nctx = 512 if self.rgb else 256
        self._trace, self._chains = None, {}

    def trace(self):
        """Per plane of the batch (frame-major): the events and the run table."""
        if self._trace is None:
            self._trace = []
            for f in self.frames:
                h, w = f.shape[:2]
                for p in planes_of(f):
                    ev = events(p, w, h)
                    ev["tab"] = run_table(ev, self.nctx)
                    self._trace.append(ev)
        return self._trace

    def tiles(self):
        return -(-self.frames[0].shape[0] * self.frames[0].shape[1] // TILE)

    def chain(self, key=None):
        frame, plane, ctx = key or self.target
        if (frame, plane, ctx) not in self._chains:
            ev = self.trace()[frame * (3 if self.rgb else 1) + plane]
            self._chains[(frame, plane, ctx)] = Chain(ev, ev["tab"], ctx)
        return self._chains[(frame, plane, ctx)]

    def slots(self):
        """[plane][tile]: the slots in use"""
        return [tile_slots(ev["tab"]) for ev in self.trace()]


def _mixed(rng, n, lo=0, hi=120):
    """n coded values in [lo, hi) in runs of 20 to 150 whose magnitude (bits of the run) changes from run to run: the best k moves and
    the counters come close to each other, so that a halving an event early or late shows in a k behind it."""
    bits = [b for b in (1, 6, 2, 0, 5, 7, 3, 1, 4, 0, 2, 6, 8, 3) if (1 << b) <= hi - lo]
    out, i = [], int(rng.integers(0, len(bits)))
    while len(out) < n:
        out += (lo + rng.integers(0, 1 << bits[i % len(bits)], size=int(rng.integers(20, 150)))).tolist()
        i += 1
    return np.array(out[:n], np.int64)


GRAY5 = 10240  # two rows of it are five tiles: the second row is the second half of tile 2 (x < 2048), tile 3 and tile 4
GRAY6 = 12288  # ... six tiles: the second row is tiles 3, 4 and 5


def _three_runs(row, seed, top=120, spikes=()):
    """A context-0 chain of mixed values in three runs, one a tile, in three consecutive tiles from the one the row stands in: run A ends
    right IN FRONT OF an event that halves, in a short record whose padding -- if it counted -- would halve before that (the
    threshold crossed inside the padding only); run B begins with that event and ends WITH an event that halves, in a short record
    (the halving on the last real event of a short record); run C holds a halving on event 0 of a record (`first`) and one on
    event 15 (`last`).
    spikes: (event, value) put into run C behind the aimed events.  Returns the marks."""
    rng = np.random.default_rng(seed)
    a, n = 19 * REC + 3, 20 * REC + 5  # run A: 19 records and one of 3 events; run B: 20 and one of 5
    sizes = [REC] * 19 + [3]
    es = aim(_mixed(rng, 2600, 0, top), a, rng, top, accept=lambda e: -20 in halvings_of(e[:a], rule="pad", recs=sizes), quiet_end=True)
    b = a + n
    es = aim(es, b - 1, rng, top)
    first, last = b + REC * 20, b + REC * 40 + 15
    es = aim(aim(es, first, rng, top), last, rng, top)
    for i, v in spikes:
        es[b + i] = v
    t0 = (row.w + row.x) // TILE + 1  # the tile behind the one the row stands in
    assert row.x + a <= t0 * TILE - row.w and b - a < TILE and len(es) - b < TILE
    row.events(0, es[:a]).to_tile(t0).events(0, es[a:b]).to_tile(t0 + 1).events(0, es[b:])
    return {"behind-padding": a, "short-last": b - 1, "first": first, "last": last}  # (the callers of _record_claims add "plane")


def _record_claims(marks):
    return [("slice-resets", (0, marks["plane"], 0)), ("halving", "short-last", None, {"last_real": True, "short": True}), ("halving", "behind-padding", None, {"event": 0}),
            ("pad-halves-in-front-of", "behind-padding"), ("halving", "first", None, {"event": 0, "n": REC}),
            ("halving", "last", None, {"event": REC - 1, "n": REC})]


def _case_in_record():
    """Gray8, five tiles: the three runs of _three_runs."""
    row = Row(GRAY5)
    marks = _three_runs(row, 31)
    return Case("in_record", [gray_frame(row)], slices=(1, 3), target=(0, 0, 0), marks=marks, claims=_record_claims(dict(marks, plane=0)), pad=True)


def _window_row(row, seed, top=120):
    """A context-0 chain of 4096 events that fills one tile (the row's first whole one): 256 full records, four windows in any launch;
    a halving on event 1024 (window 1, record 0, event 0) and on event 3071 (window 2, record 63, event 15: the window's last
    event, its carry the halved state alone)."""
    rng = np.random.default_rng(seed)
    es = aim(aim(_mixed(rng, TILE, 0, top), 1024, rng, top), 3071, rng, top)
    t0 = -(-row.w // TILE)
    row.to_tile(t0).events(0, es)
    return {"window-first": 1024, "window-last": 3071}


def _zero_windows_row(row, seed):
    """A context-0 chain of 640, 384 and 301 events in three tiles, the first 1025 of them of value 0: no halving in the first two
    runs (40 and 24 records: two windows under one slice a tile, exactly one under one slice) and the first halving on the first event
    of the third, event 1024; mixed values behind it."""
    rng = np.random.default_rng(seed)
    tail = _mixed(rng, 300)
    t0 = -(-row.w // TILE)
    row.skip_to(16).events(0, [0] * 640).to_tile(t0).events(0, [0] * 384).to_tile(t0 + 1).events(0, [0]).events(0, tail)


def _case_in_window():
    """Gray8, five tiles.  Frame 0: _window_row.  Frame 1: _zero_windows_row."""
    a, b = Row(GRAY5), Row(GRAY5)
    marks = _window_row(a, 37)
    _zero_windows_row(b, 41)
    claims = [("halving", "window-first", 1, {"window": 1, "record": 0, "event": 0}), ("halving", "window-last", 1, {"window": 2, "record": 63, "event": 15}),
              ("launch", 1, (0, 0, 0), [256]), ("zero-windows", (1, 0, 0)),
              ("reset-shows", (0, 0, 0), [64, 128, 192]), ("reset-shows", (1, 0, 0), [40, 64])]
    return Case("in_window", [gray_frame(a), gray_frame(b)], slices=(1, 5), target=(0, 0, 0), marks=marks, claims=claims)


LENGTHS = ((256, 193, 257, 192, 63), (191, 129, 128, 127, 65, 64, 1))   # records in one launch, per frame and chain
LENGTH_CTX = ((1, 2, 0, 3, 4), (0, 1, 2, 3, 4, 5, 6))


def _lengths_frame(f, less=None):
    """Chains of LENGTHS[f][i] full records of context LENGTH_CTX[f][i], one behind the other from pixel 16 of the row (less: records
    fewer).  The chain of 257 is the target: values from 0 up; from pixel 7207, so that tile 5 ends with its record 61, a short
    one of 9 events, and tile 6 holds its other 195 (fewer by the records its own context's by-products add)."""
    rng = np.random.default_rng(43 + f)
    row = Row(16384).skip_to(16)
    for c, n in zip(LENGTH_CTX[f], LENGTHS[f]):
        if n == 257:
            row.skip_to(7207).events(c, _mixed(rng, 61 * REC + 9 + (195 - (less[c] if less else 0)) * REC))
            assert row.x % REC == 0
        else:
            row.events(c, _mixed(rng, (n - (less[c] if less else 0)) * REC, 16))
    return gray_frame(row)


def _case_lengths():
    """Gray8, eight tiles (the second row is tiles 4 .. 7), two frames: chains of 1 .. 257 records in one launch, each in a context of
    its own, every chain but the target from a multiple of 16 pixels of the row so that the tile boundaries cut no record.  The
    target (frame 0, context 0) holds values from 0 up; the others values from 16 up, so that their by-products in the first row
    have larger contexts, and are shortened by the records the target's by-products (contexts 1 + e) add to them."""
    less = [0] * 5
    for _ in range(6):  # (the by-products move a little with the chains' lengths)
        tab = run_table(events(_lengths_frame(0, less).astype(np.int32), 16384, 2), 256)
        off = {c: int((-(-tab[c] // REC)).sum()) - n for c, n in zip(LENGTH_CTX[0], LENGTHS[0])}
        if not any(off.values()):
            break
        less = [less[c] + off[c] for c in range(5)]
    frames = [_lengths_frame(0, less), _lengths_frame(1)]
    return Case("lengths", frames, slices=(1,), target=(0, 0, 0),
                claims=[("launch", 1, (f, 0, c), [n]) for f in range(2) for c, n in zip(LENGTH_CTX[f], LENGTHS[f])]
                + [("both-forms", 1), ("reset-shows", (0, 0, 0), [64, 128, 192, 256])], pad=True)


def _tiles_row(extra=None):
    """Gray8, five tiles; the second row's events lie in tiles 2, 3 and 4 and, in tile 4, in front of pixel 8192 of the row, so that
    the first row's by-products stay in tiles 0 and 1.  Context 0, the target (values from 0 up): tiles 2 and 4; contexts 1 .. 4
    (values from 16 up).  extra = (context, values): events of that context in tile 4."""
    rng = np.random.default_rng(47)
    row = Row(GRAY5)
    v = lambda n: _mixed(rng, n, 16)
    row.events(1, v(32)).events(2, v(33)).events(0, _mixed(rng, 165)).events(4, v(17))
    row.to_tile(3).events(1, v(48)).events(2, v(49)).events(3, v(161)).events(4, v(161))
    row.to_tile(4).events(0, _mixed(rng, 900)).events(1, v(1)).events(2, v(16)).events(3, v(40))
    if extra:
        row.events(extra[0], extra[1])
    assert row.x <= 8192
    return row


def _case_tiles():
    """Runs of 16 k and 16 k + 1 events (contexts 1 and 2); under two slices (tiles 0 - 1 and 2 - 4) a chain without events in the
    slice's first tile (context 3), in its middle tile (context 0, the target) and in its last tile (context 4); and a chain of
    by-products in tile 0 that goes on in the last tile and nowhere between."""
    tab = run_table(events(gray_frame(_tiles_row()).astype(np.int32), GRAY5, 2), 256)
    vals = _mixed(np.random.default_rng(53), 40, 16)
    for x in range(21, 122):
        if tab[x, 0] > 0 and tab[x, 1:].sum() == 0:
            f = gray_frame(_tiles_row((x, vals)))
            if run_table(events(f.astype(np.int32), GRAY5, 2), 256)[x].tolist() == [tab[x, 0], 0, 0, 0, 40]:
                break
    else:
        raise AssertionError("no context of by-products in tile 0 alone")
    claims = [("runs-from", 2, (0, 0, 1), [32, 48, 1]), ("runs-from", 2, (0, 0, 2), [33, 49, 16]), ("runs-from", 2, (0, 0, 3), [0, 161, 40]),
              ("runs-from", 2, (0, 0, 0), [165, 0, 900]), ("runs-from", 2, (0, 0, 4), [17, 161, 0]), ("runs", (0, 0, x), [int(tab[x, 0]), 0, 0, 0, 40]),
              ("slice-resets", (0, 0, 0)), ("reset-shows", (0, 0, x), [-(-int(tab[x, 0]) // REC)])]
    return Case("tiles", [f], slices=(1, 2, 5), target=(0, 0, 0), claims=claims, pad=True)


SLICE_COUNTS = (1, 2, 3, 5, 12)


def _case_slices():
    """Gray8, six tiles (the second row is tiles 3, 4, 5).  The target: the three runs of _three_runs -- a halving on the first event
    behind the boundary between tiles 3 and 4 (a slice boundary under 3, 5 and 12 slices) and one on the last event in front of
    the boundary between tiles 4 and 5 (one under 12).  Context 1: a chain in tiles 3 and 5 alone, resumed from chain_state across the slice of
    tile 4 (12 slices: one tile a slice, every other slice none at all)."""
    rng = np.random.default_rng(59)
    row = Row(GRAY6)
    row.events(1, _mixed(rng, 150, 40))
    marks = _three_runs(row, 61)
    row.events(1, _mixed(rng, 150, 40))
    first_of = {"window": 0, "record": 0, "event": 0}
    claims = [("halving", "behind-padding", 12, dict(first_of, slice=9)), ("halving", "behind-padding", 5, dict(first_of, slice=4)),
              ("halving", "behind-padding", 3, dict(first_of, slice=2)), ("halving", "short-last", 12, {"slice": 9, "last_real": True, "short": True}),
              ("runs-from", 3, (0, 0, 1), [150, 0, 150]), ("slice-resets", (0, 0, 0)), ("slice-resets", (0, 0, 1)),
              ("empty-slices", 12)]
    return Case("slices", [gray_frame(row)], slices=SLICE_COUNTS, target=(0, 0, 0), marks=marks, claims=claims, pad=True)


def _three_tile_frame(kind, rng, where, values=(0, 120)):
    """Two rows of 6144 (three tiles): 1500 events of context 0 in the second row at x in `where` = 0 (tiles 0 and 1 hold events, 2
    none), 2048 (tiles 0 and 2, 1 none) or 4096 (tiles 1 and 2, 0 none); None: no events at all."""
    row = Row(6144) if kind == "gray" else co_row(6144)
    if where is not None:
        row.skip_to(max(where, 2)).events(0, _mixed(rng, 1500, *values))
    return gray_frame(row) if kind == "gray" else rgb_frame(row)


def _case_planes_gray():
    """Eleven gray8 frames of three tiles (33 items for k_assign3 under one slice, groups of eight): the first group begins with an
    empty tile, holds one in the middle and ends with one, and spans three planes."""
    rng = np.random.default_rng(67)
    where = [4096, 2048, 2048, 0, None, 4096, 0, 2048, None, 0, 4096]
    return Case("planes_gray", [_three_tile_frame("gray", rng, x) for x in where], slices=(1, 3), target=(3, 0, 0),
                claims=[("assign-group", 1), ("planes-not-8",), ("reset-shows", (3, 0, 0), [64])])


def _case_planes_rgb():
    """Three RGB8 frames of three tiles, nine planes (under three slices nine items a launch: a group of eight and one of one); in
    tile 0 the first and the last frame hold no events, so the first group of that launch begins with empty tiles, holds some in the middle
    and ends with one (Co of the last frame)."""
    rng = np.random.default_rng(71)
    return Case("planes_rgb", [_three_tile_frame("rgb", rng, x, (0, 255)) for x in (4096, 0, 4096)], slices=(1, 3), target=(1, 1, 0),
                claims=[("assign-group", 3), ("planes-not-8",), ("reset-shows", (1, 1, 0), [64])])


def _case_chroma():
    """RGB8, five tiles a plane; the Co plane holds the three runs of _three_runs in context 0 with values up to 254 (the u16 event type)
    and, in the last run, the values 255, 256 and 509 (the largest there is: both neighbours -255, the sample 255) and an event of
    context 509, the largest that can hold one (neighbours 255 and -254: at 510 every sample lies in range), of value 0."""
    row = co_row(GRAY5)
    marks = _three_runs(row, 73, top=255, spikes=((700, 200), (701, 255), (702, 200), (703, 256)))
    row.events(0, [254 - int(row.row[row.x - 1])] if row.row[row.x - 1] < 0 else [int(row.row[row.x - 1]) + 254])  # to an end of the range
    left = int(row.row[row.x - 1])
    assert abs(left) == 255
    row.events(0, [509]).events(509, [0])
    return Case("chroma", [rgb_frame(row)], slices=(1, 3), target=(0, 1, 0), marks=marks,
                claims=_record_claims(dict(marks, plane=1)) + [("values", (0, 1, 0), [255, 256, 509]), ("runs", (0, 1, 509), [0, 0, 0, 0, 1])], pad=True)


def _case_chroma_window():
    """RGB8, five tiles a plane: _window_row on the Co plane, values up to 254."""
    row = co_row(GRAY5)
    marks = _window_row(row, 79, top=255)
    return Case("chroma_window", [rgb_frame(row)], slices=(1,), target=(0, 1, 0), marks=marks,
                claims=[("halving", "window-first", 1, {"window": 1, "record": 0, "event": 0}), ("halving", "window-last", 1, {"window": 2, "record": 63, "event": 15}),
                        ("launch", 1, (0, 1, 0), [256]), ("reset-shows", (0, 1, 0), [64, 128, 192])])


def _one_past_row(row, counts, seed=107):  # (the seed: searched on the CPU, so that every mutated rule shows in the 641 events)
    """Runs of counts[c] events of context c in the row's first whole tile (the second row begins with it): context 0 of mixed
    values, the others of value 0."""
    assert row.w % TILE == 0
    rng = np.random.default_rng(seed)
    for c, n in enumerate(counts):
        row.events(c, _mixed(rng, n) if c == 0 else [0] * n)
    return row


def _cap_counts(nctx, cap, over):
    """Events per context for a tile of exactly `cap` slots (over: one record more) with every run one past a whole record: 641
    events (41 records) of context 0, the target; runs of 17 events (two records) as long as the tile's pixels allow; runs of one."""
    recs = cap // REC + (1 if over else 0) - 41
    two = min((TILE - 700 - recs) // 15, recs // 2)
    one = recs - 2 * two
    assert 1 + two + one <= nctx - 2 and 641 + 17 * two + one < TILE - 1
    return [641] + [17] * two + [1] * one


def _case_cap(over):
    """Gray8, two tiles, the second row is tile 1: every context's run there one past a whole record -- 17 events or one -- and the
    tile's slots exactly 6144 (fits: tile_overflows stays 0) or 6160 (one overflow, the batch again with the worst-case cap)."""
    row = _one_past_row(Row(TILE, start=100), _cap_counts(256, CAP[256], over))
    slots = CAP[256] + (REC if over else 0)
    return Case("cap_over" if over else "cap_fits", [gray_frame(row)], slices=(1, 3), target=(0, 0, 0), overflows=over,
                claims=[("slots", 0, 1, slots), ("one-past",  0, 1), ("overflow", over), ("reset-shows", (0, 0, 0), [20])])


def _case_cap_co(over):
    """The same for a Co tile: 8192 / 8208 slots."""
    row = _one_past_row(co_row(TILE), _cap_counts(512, CAP[512], over))
    slots = CAP[512] + (REC if over else 0)
    return Case("cap_co_over" if over else "cap_co_fits", [rgb_frame(row)], slices=(1, 3), target=(0, 1, 0), overflows=over,
                claims=[("slots", 1, 1, slots), ("one-past", 1, 1), ("overflow", over), ("reset-shows", (0, 1, 0), [20])])


def _case_word_path():
    """Gray8, two tiles, two frames: tile 1 of the first holds exactly 2048 slots in use (the most k_pack_t's per-event path takes), of
    the second 2064; in both a chain of zeros learns k = 0 and then meets values of 100 and more: Rice codes of more than 23 bits."""
    frames = []
    for n in (WORD_PATH_MAX_SLOTS, WORD_PATH_MAX_SLOTS + 1):
        rng = np.random.default_rng(83)
        row = Row(TILE)
        row.events(0, [0] * 60 + [100, 0, 0, 119, 0, 0, 0, 30]).events(0, _mixed(rng, n - 68))
        frames.append(gray_frame(row))
    return Case("word_path", frames, slices=(1,), target=(0, 0, 0),
                claims=[("slots", 0, 1, WORD_PATH_MAX_SLOTS), ("slots", 1, 1, WORD_PATH_MAX_SLOTS + REC), ("long-code", 0, 1), ("long-code", 1, 1), ("reset-shows", (0, 0, 0), [64])])


def _case_enum_chunk():
    """One gray8 frame of 4096 x 4100: a row is a tile, 4100 tiles in one slice -- k_enum scans a chain's tiles 4096 at a time (64
    rounds of 64), so the second chunk holds tiles 4096 .. 4099.  Constant 128 except for a band, rows 4094 .. 4097: there every
    other pixel (x + y even, x >= 2) is an event of context 0 and a made-to-order value -- its left neighbour and the one above
    are 128, the sample 128 +- (1 + e), the sign by (x - y) / 2 so that the 128s between lie in range -- and single such samples
    in rows 0, 63, 64 and 4099.  The chain of context 0 is the only one: 2047 events in each of the tiles 4094 .. 4097, across the
    chunk boundary, and a few in tiles 0, 63 and 64 (both sides of a round boundary) and 4099."""
    w, h = TILE, 4100
    f = np.full((h, w), 128, np.uint8)
    rng = np.random.default_rng(101)
    yy, xx = np.meshgrid(np.arange(4094, 4098), np.arange(2, w), indexing="ij")
    at = (xx + yy) % 2 == 0
    es = _mixed(rng, int(at.sum()), 0, 120)
    sign = np.where(((xx - yy) // 2) % 2 == 0, 1, -1)[at]
    f[yy[at], xx[at]] = 128 + sign * (1 + es)
    for (y, x), e in zip(((0, 10), (0, 500), (63, 7), (63, 9), (64, 4000), (4099, 50), (4099, 4095)), (3, 40, 0, 17, 5, 90, 2)):
        f[y, x] = 128 + 1 + e
    return Case("enum_chunk", [f], slices=(1,), target=(0, 0, 0),
                claims=[("runs-from", 4094, (0, 0, 0), [2047, 2047, 2047, 2047, 0, 2]), ("tiles-hold", (0, 0, 0), {0: 2, 63: 2, 64: 1}),
                        ("only-chain", (0, 0, 0)), ("reset-shows", (0, 0, 0), [1, 2, 3, 3 + 128, 3 + 256, 3 + 384, 3 + 512])])


_BUILDERS = {"in_record": _case_in_record, "in_window": _case_in_window, "lengths": _case_lengths, "tiles": _case_tiles, "slices": _case_slices,
             "planes_gray": _case_planes_gray, "planes_rgb": _case_planes_rgb, "chroma": _case_chroma, "chroma_window": _case_chroma_window,
             "cap_fits": lambda: _case_cap(False), "cap_over": lambda: _case_cap(True), "cap_co_fits": lambda: _case_cap_co(False),
             "cap_co_over": lambda: _case_cap_co(True), "word_path": _case_word_path}
NAMES = tuple(_BUILDERS)                  # the small cases: every frame below 40 000 pixels
_BUILDERS["enum_chunk"] = _case_enum_chunk
LARGE = ("enum_chunk",)                   # 16.8 MPix: encoded once
OVERFLOWING = ("cap_over", "cap_co_over")  # the cases with Case.overflows (the GPU tests give each a context of its own)
_CASES = {}


def case(name):
    if name not in _CASES:
        _CASES[name] = _BUILDERS[name]()
    return _CASES[name]


# ------------------------------------------------------------------------------------------------------------------------
# premises and sensitivity
# ------------------------------------------------------------------------------------------------------------------------

def _assign_groups(slots, tiles, ns):
    """Per launch of k_assign3 (a slice of ns that holds tiles), its groups of eight (plane, tile) items as lists of slot totals."""
    b = slice_bounds(tiles, ns)
    out = []
    for q in range(ns):
        items = [(p, int(slots[p][t])) for p in range(len(slots)) for t in range(b[q], b[q + 1])]
        if items:
            out.append([items[i:i + 8] for i in range(0, len(items), 8)])
    return out


def premises(c):
    """Asserts, from the oracle's trace alone, everything case c claims: where its chains' records, windows and halvings lie for every
    slice count it runs with, what its tiles hold, and that every mutated replay the claim names changes a k behind the place."""
    tr = c.trace()
    T = c.tiles()
    slots = c.slots()
    assert any((s > CAP[c.nctx]).any() for s in slots) == c.overflows, (c.name, [s.max() for s in slots])
    for claim in c.claims:
        kind = claim[0]
        if kind == "halving":
            _, mark, ns, want = claim
            ch, i = c.chain(), c.marks[mark]
            assert i in ch.halvings(), (c.name, mark, i)
            for n in (c.slices if ns is None else (ns,)):
                assert n in c.slices, (c.name, claim)
                q, win, rec, evt, size = locate(ch.row, i, n)
                got = {"slice": q, "window": win, "record": rec, "event": evt, "n": size, "last_real": evt == size - 1, "short": size < REC}
                assert all(got[k] == v for k, v in want.items()), (c.name, mark, n, got, want)
            assert ch.shows("late", at=i, behind=i + 1), (c.name, mark, "late")
            assert ch.shows("swap", at=i, behind=i), (c.name, mark, "swap")
        elif kind == "pad-halves-in-front-of":
            ch, i = c.chain(), c.marks[claim[1]]
            r = next(r for r in range(len(ch.sizes)) if ch.first_event(r + 1) == i)  # the record that ends in front of event i
            assert ch.sizes[r] < REC and -1 - r in halvings_of(ch.es, rule="pad", recs=ch.sizes), (c.name, claim, ch.sizes[r])
            assert ch.shows("pad", behind=i), (c.name, claim)
        elif kind == "launch":
            _, ns, key, counts = claim
            assert ns in c.slices and [n for n in launch_records(c.chain(key).row, ns) if n] == counts, (c.name, claim, launch_records(c.chain(key).row, ns))
        elif kind == "both-forms":
            wins = [-(-n // WIN) for ev in tr for row in ev["tab"] for n in launch_records(row, claim[1]) if n]
            assert min(wins) < SP3_MULTI_MIN <= max(wins) and {1, 2, 3, 4, 5} <= set(wins), (c.name, sorted(set(wins)))
        elif kind == "zero-windows":
            ch = c.chain(claim[1])
            assert (ch.es[:1025] == 0).all() and ch.halvings()[0] == 1024
            assert [n for n in launch_records(ch.row, 5) if n] == [40, 24, 19] and 5 in c.slices and 1 in c.slices
            assert locate(ch.row, 1023, 5)[1:4] == (0, 23, 15) and locate(ch.row, 1024, 5)[1:4] == (0, 0, 0)  # two windows without, the third begins with it
            assert locate(ch.row, 1024, 1)[1:4] == (1, 0, 0)
            assert ch.shows("none", behind=1025), c.name
        elif kind == "reset-shows":
            ch = c.chain(claim[1])
            for r in claim[2]:
                assert 0 < r < len(ch.sizes) and ch.shows("reset", at=r, behind=ch.first_event(r)), (c.name, claim, r)
        elif kind == "runs":
            assert c.chain(claim[1]).row.tolist() == list(claim[2]), (c.name, claim, c.chain(claim[1]).row.tolist())
        elif kind == "runs-from":
            assert c.chain(claim[2]).row[claim[1]:].tolist() == list(claim[3]), (c.name, claim, c.chain(claim[2]).row.tolist())
        elif kind == "tiles-hold":
            row = c.chain(claim[1]).row
            assert all(row[t] == n for t, n in claim[2].items()) and len(row) > TILE, (c.name, claim)
        elif kind == "only-chain":
            assert all((ev["ctx"] == claim[1][2]).all() for ev in tr) and 1 in c.slices, c.name
        elif kind == "slice-resets":
            ch = c.chain(claim[1])
            starts = {ns: first_record_of_slices(ch.row, ns) for ns in c.slices}
            assert any(starts.values()), (c.name, claim)
            for ns, rs in starts.items():
                for r in rs:
                    assert ch.shows("reset", at=r, behind=ch.first_event(r)), (c.name, claim, ns, r)
        elif kind == "empty-slices":
            b = slice_bounds(T, claim[1])
            width = [y - x for x, y in zip(b, b[1:])]
            assert claim[1] in c.slices and 0 in width and 1 in width, (c.name, b)
        elif kind == "assign-group":
            ns = claim[1]
            assert ns in c.slices
            launches = _assign_groups(slots, T, ns)
            assert any(sum(len(g) for g in groups) % 8 != 0 for groups in launches), c.name
            assert any(len(g) == 8 and len({p for p, _ in g}) > 1 and g[0][1] == 0 and g[-1][1] == 0 and any(n == 0 for _, n in g[1:-1])
                       and any(n > 0 for _, n in g) for groups in launches for g in groups), (c.name, launches[0][0])
        elif kind == "planes-not-8":
            assert len(tr) % 8 != 0 and len(tr) > 8, (c.name, len(tr))
        elif kind == "values":
            assert set(claim[2]) <= set(c.chain(claim[1]).es.tolist()), (c.name, claim)
        elif kind == "slots":
            _, plane, tile, n = claim
            assert slots[plane][tile] == n, (c.name, claim, slots[plane].tolist())
        elif kind == "one-past":
            runs = tr[claim[1]]["tab"][:, claim[2]]
            assert (runs[runs > 0] % REC == 1).all() and (runs > 0).sum() > 100, (c.name, claim)
        elif kind == "overflow":
            assert c.overflows == claim[1]
        elif kind == "long-code":
            ev = tr[claim[1]]
            sel = ev["pix"] // TILE == claim[2]
            assert ((ev["val"][sel] >> ev["k"][sel]) + 1 + ev["k"][sel]).max() > 23, (c.name, claim)
        else:
            raise AssertionError("unknown claim %r" % (claim,))


def sensitivity(c):
    """Every rule of the case, mutated, changes a k of the target chain (behind its first event); cases without marked events: every
    halving late, and the exchange of the first halving event with the one behind it that shows."""
    ch = c.chain()
    assert replay(ch.es) == ch.k, c.name
    for rule in c.rules:
        if rule in ("late", "swap") and c.marks:
            continue  # (claimed mark by mark: premises)
        if rule == "swap":
            assert any(ch.es[h] != ch.es[h + 1] and ch.shows("swap", at=h, behind=h) for h in ch.halvings() if h + 1 < len(ch.es)), (c.name, rule)
        else:
            assert ch.shows(rule, behind=1), (c.name, rule)


def replay_matches_oracle(c):
    """The replay (true rule) gives the oracle's k for every record of every plane of the case."""
    for i, ev in enumerate(c.trace()):
        want = ev["k"][ev["order"]]
        got = replay_records(ev, NK)
        assert (got == want).all(), "%s plane %d: record %d" % (c.name, i, int(np.flatnonzero(got != want)[0]))
