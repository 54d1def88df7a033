"""What the tests of the 16-bit front end share (test_wide_cases_cpu.py, test_wide_replay_gpu.py): frames built to reach the
boundaries felics_wide.hip branches on -- the event sort, the chain heads, the wave-per-chain and the four-lanes-per-chain
replay of the estimator with its hand-over -- and the proof, from the CPU oracle alone, that each frame reaches what it is for
and that a replay with a slightly different rule would give other Rice parameters there.

A CHAIN is the events (samples outside [L, H], behind a plane's first two) of one context of one plane, in raster order; the
kernels hold a plane's events as records sorted stably by context, so a chain is a run of records.  Chain indices count from 0.
A HALVING AT i: the counters are halved after event i (it lifted their minimum above 1024).  A forced LIMIT L: the four-lane kernel
replays events 0 .. L - 1 of every chain and hands the rest to the wave-wide kernel, whose blocks of 64 then start at event L."""
import numpy as np

from tests import oracle_lib

NK, HALVE = 15, 1024
NEVER = 1 << 30            # a limit no chain reaches: the four-lane kernel alone
SORT_TILE = 4096           # records of a sort tile; four consecutive tiles share a histogram workgroup
POISON_CTX = 0x1A5A5       # the low 18 bits of the 0xA5 bytes FELICS_POISON fills the record buffer with
RULES = ("ge", "late", "small", "none")


# ------------------------------------------------------------------------------------------------------------------------
# events, chains, replay
# ------------------------------------------------------------------------------------------------------------------------

def planes_of(img):
    """The planes the encoder codes: the frame itself, or Y / Co / Cg of an RGB frame (the division truncates towards zero)."""
    if img.ndim == 2:
        return [img.astype(np.int32)]
    r, g, b = (img[..., i].astype(np.int32) for i in range(3))
    co = r - b
    t = b + np.trunc(co / 2).astype(np.int32)
    cg = g - t
    return [t + np.trunc(cg / 2).astype(np.int32), co, cg]


def events(plane, w, h):
    """The events of a plane, from the oracle's trace: pixel index, context, coded value and k of each in raster order (pix, ctx,
    val, k), and `order`, the stable sort by context that gives the records as the kernels hold them."""
    tr = oracle_lib.load().trace_channel(plane, w, h, depth=1)
    pix = np.flatnonzero(tr["cls"] != 0)
    pix = pix[pix >= 2]
    ev = {"pix": pix, "ctx": tr["ctx"][pix].astype(np.int64), "val": tr["val"][pix].astype(np.int64), "k": tr["k"][pix].astype(np.int64)}
    ev["order"] = np.argsort(ev["ctx"], kind="stable")
    return ev


def chains_of(ev):
    """(context, first record, length) of every chain of a plane, in record order, as three arrays."""
    ctx = ev["ctx"][ev["order"]]
    if len(ctx) == 0:
        z = np.zeros(0, np.int64)
        return z, z, z
    first = np.flatnonzero(np.r_[True, ctx[1:] != ctx[:-1]])
    return ctx[first], first, np.diff(np.r_[first, len(ctx)])


def replay(es, rule="true", at=None, halvings=None):
    """k of every event of one chain with coded values es, replayed in plain Python: k is the argmin of the fifteen counters with ties
    to the largest k; the event adds (e >> k) + 1 + k to counter k; all counters are halved after an event that lifts their minimum
    above 1024.  `halvings`: a list that receives the indices of the events that halved.
    The mutated rules: "ge" halves at a minimum >= 1024; "late" halves one event after the one that asked for it (at = i: only the
    halving at event i is late); "small" breaks ties towards the smallest k; "none" never halves; "swap" replays the chain with
    events at and at + 1 exchanged and gives k in the exchanged order."""
    es = np.array(es, np.int64)
    if rule == "swap":
        es[[at, at + 1]] = es[[at + 1, at]]
    ks = np.arange(NK)
    adds = (es[:, None] >> ks) + 1 + ks  # what every event adds to every counter
    S = np.zeros(NK, np.int64)
    out, owed = [], False
    for i in range(len(es)):
        out.append(int(S.argmin()) if rule == "small" else NK - 1 - int(S[::-1].argmin()))
        S += adds[i]
        m = int(S.min())
        asks = m >= HALVE if rule == "ge" else m > HALVE
        if rule == "none":
            asks = False
        if owed:  # (the late halving: instead of this event's own question)
            asks, owed = True, False
        elif asks and rule == "late" and (at is None or at == i):
            asks, owed = False, True
        if asks:
            S >>= 1
            if halvings is not None:
                halvings.append(i)
    return out


def replay_records(ev, nk=NK):
    """k of every record of a plane by the true rule, all chains side by side (numpy over the chains, one step per chain index);
    nk counters (the 8-bit estimator has six: tests/chain_cases.py)."""
    val = ev["val"][ev["order"]]
    _, first, length = chains_of(ev)
    out = np.zeros(len(val), np.int64)
    if len(val) == 0:
        return out
    by_len = np.argsort(-length, kind="stable")
    first, length = first[by_len], length[by_len]
    S = np.zeros((len(first), nk), np.int64)
    ks = np.arange(nk)
    for t in range(int(length[0])):
        n = int(np.searchsorted(-length, -t, side="left"))  # chains longer than t: a prefix
        A = S[:n]
        at = first[:n] + t
        out[at] = nk - 1 - np.argmin(A[:, ::-1], axis=1)
        A += (val[at][:, None] >> ks) + 1 + ks
        A[A.min(axis=1) > HALVE] >>= 1
    return out


# ------------------------------------------------------------------------------------------------------------------------
# constructions
# ------------------------------------------------------------------------------------------------------------------------

def chain_frame(segments, width=None, start=30000):
    """A two-row gray16 frame whose second row is a made-to-order event list: segments = [(context, coded values), ...].  A pixel
    of the second row has its left neighbour and the one above; the row above is the second row shifted and offset by the context,
    so every pixel (1, x >= 1) is an event of the wanted context and the wanted value whatever went before.  The first row's own
    events are by-products in other contexts (near 1 + e and context + 1 + e).  Padded to `width` with samples that are no events."""
    n = sum(len(e) for _, e in segments)
    w = max(width or 0, n + 1)
    row = np.zeros((2, w), np.int64)
    row[1, 0] = start
    x = 1
    for ctx, es in segments:
        for e in es:
            left = int(row[1, x - 1])
            above = left + ctx if left + ctx <= 65535 else left - ctx
            lo, hi = min(left, above), max(left, above)
            e = int(e)
            p = hi + 1 + e if (left < 32768 or lo - 1 - e < 0) else lo - 1 - e
            assert 0 <= p <= 65535 and 0 <= above <= 65535, (ctx, e, left)
            row[0, x], row[1, x] = above, p
            x += 1
    row[0, 0] = row[0, 1] + 7777 if row[0, 1] < 50000 else row[0, 1] - 7777
    row[0, x:] = row[1, x - 1]  # the padding: equal to both neighbours, so in range
    row[1, x:] = row[1, x - 1]
    return row.astype(np.uint16)


def single_chain_frame(w, s):
    """W x 3, first row s * x, all rows the same: W - 2 events, all of context s and value s - 1."""
    return np.tile((s * np.arange(w)).astype(np.uint16), (3, 1))


def checkerboard(w, h):
    yy, xx = np.indices((h, w))
    return (((xx + yy) & 1) * 65535).astype(np.uint16)


def level_noise(rng, w, h, levels=(0, 513, 1026, 1539)):
    """Samples drawn from a few levels.  The default gives contexts 0, 513 and 1026, which differ in both 9-bit sort digits, and chains
    of thousands of events -- but values so alike that k never moves.  LEVELS adds close pairs and a far level: fourteen contexts
    in both digits, values from 1 to 8999 in one chain, so that the order of a chain's events shows in its k."""
    return np.array(levels, np.uint16)[rng.integers(0, len(levels), size=(h, w))]


LEVELS = (0, 2, 513, 1026, 1031, 9000)


def noise_with_records(rng, w, h, nrec):
    """Full-range noise from the start of the frame and a constant behind it (no events there), cut some 30 events short of nrec;
    the rest are single samples in the constant's last row, each an event and nothing else (its neighbours to the right and
    below still equal one of theirs)."""
    f = rng.integers(0, 65536, size=w * h, dtype=np.uint16)
    m = int(1.5 * (nrec - 30))
    assert m + 3 * w < w * h, "the frame is too small for %d events" % nrec

    def count(g):
        return len(events(g.reshape(h, w).astype(np.int32), w, h)["pix"])

    for _ in range(40):
        g = f.copy()
        g[m:] = g[m - 1]
        short = nrec - count(g)
        if 0 <= short <= (w - 2) // 2:
            break
        m += int(1.4 * short) - 5 if short > 0 else -20
    assert 0 <= short <= (w - 2) // 2 and m + 3 * w < w * h, (nrec, m, short)
    last = g.reshape(h, w)[h - 1]
    last[2:2 + 2 * short:2] ^= 0x5555
    assert count(g) == nrec
    return g.reshape(h, w)


def mixed_values(rng, n, bits):
    """n coded values in runs of 40 to 400 whose magnitude (bits of the run) changes from run to run: the best k moves, counters
    come close to each other, and where the values are large the counters are halved several times in 64 events."""
    out = []
    i = 0
    while len(out) < n:
        b = bits[i % len(bits)]
        out += rng.integers(0, 1 << b, size=int(rng.integers(40, 400))).tolist()
        i += 1
    return np.array(out[:n], np.int64)


def rgb_from_chroma(co, cg, y0=0):
    """An RGB16 frame with the given Co and Cg planes (int arrays of one shape); every sample must fit 16 bits."""
    co, cg = np.asarray(co, np.int64), np.asarray(cg, np.int64)
    b = np.where(co < 0, -co, 0) + y0
    r = b + co
    t = b + np.trunc(co / 2).astype(np.int64)
    g = cg + t
    lift = np.maximum(0, -g)  # (cg below -t: raise r, g and b together, which leaves Co and Cg alone)
    r, g, b = r + lift, g + lift, b + lift
    img = np.stack([r, g, b], axis=-1)
    assert img.min() >= 0 and img.max() <= 65535, (img.min(), img.max())
    return img.astype(np.uint16)


# ------------------------------------------------------------------------------------------------------------------------
# cases
# ------------------------------------------------------------------------------------------------------------------------

CHAIN_LENGTHS = (1, 2, 3, 4, 5, 31, 32, 33, 63, 64, 65, 127, 128, 129)
LIMIT_EDGES = (1, 6, 32, 33, 128)  # one, not a multiple of 4, 32, 33, a multiple of 64
STARTS = (64, 1024, 4096, 16384)

EDGES = tuple(
    ["len:%d" % n for n in CHAIN_LENGTHS] + ["limit:%d" % n for n in LIMIT_EDGES]
    + ["halve:mod64=0", "halve:mod64=63", "halve:last-partial", "halve:two-in-block", "halve:mod32=31", "halve:mod32=0", "halve:handover"]
    + ["halve:mod4=%d" % r for r in range(4)] + ["start:%d" % o for o in STARTS]
    + ["records:4095", "records:4096", "records:4097", "records:>16384", "tiles:straddle", "tiles:unaligned"]
    + ["empty:first", "empty:middle", "empty:last", "planes:shared-context", "chains:>150000", "long:>8192"]
    + ["chroma:largest-fields", "poison:last-context", "sort:stability"] + ["rule:%s" % r for r in RULES])


class Case:
    """frames: same-shaped frames, one sub-batch in this order.  limits: the forced limits the case is aimed at (0 and NEVER
    are run for every case).  target: (frame, plane, context) of the chain the replay rules are checked on.  edges: what the case
    claims to reach; premises() proves every claim from the oracle."""

    def __init__(self, name, frames, limits=(), target=None, edges=()):
        self.name, self.frames, self.limits, self.target, self.edges = name, [np.ascontiguousarray(f) for f in frames], tuple(limits), target, tuple(edges)
        assert len({f.shape for f in self.frames}) == 1, name
        self._trace, self._late = None, {}

    def trace(self):
        """Per plane of the batch (frame-major): the events, the chains, and the records' k by the Python replay."""
        if self._trace is None:
            self._trace = []
            for f in self.frames:
                h, w = f.shape[:2]
                for p in planes_of(f):
                    ev = events(p, w, h)
                    ev["chain_ctx"], ev["chain_first"], ev["chain_len"] = chains_of(ev)
                    self._trace.append(ev)
        return self._trace

    def plane_index(self, frame, plane):
        return frame * (3 if self.frames[0].ndim == 3 else 1) + plane

    def target_values(self):
        frame, plane, ctx = self.target
        ev = self.trace()[self.plane_index(frame, plane)]
        sel = ev["ctx"] == ctx
        return ev["val"][sel], ev["k"][sel]

    def target_halvings(self):
        hv = []
        replay(self.target_values()[0], halvings=hv)
        return hv

    def late_shows(self, h):
        """Does halving one event late at event h alone change a k of the target chain?"""
        if h not in self._late:
            self._late[h] = late_shows(self.target_values()[0], h)
        return self._late[h]


def late_shows(es, h):
    """Does halving one event late at event h alone change a k of the chain?"""
    return replay(es, "late", at=h) != replay(es)


def _case_dense():
    """One context-0 chain of mixed magnitudes with halvings at every residue, on its own and cut right behind a halving; the limits
    put a halving on the last four-lane event, on the first wave-wide event (lane 0 of its block) and on lane 63 of that block."""
    es = mixed_values(np.random.default_rng(1), 3000, (1, 14, 2, 0, 9, 15, 3, 1, 12, 0, 2, 6, 15, 1))  # (the seed: searched on the CPU)
    hv = []
    replay(es, halvings=hv)
    cut = next(h for h in hv if h > 700 and (h + 1) % 64 not in (0, 1))  # a chain that ends with the event that halves, mid-block
    hand = next(h for h in hv if h > 300 and h % 4 != 0 and late_shows(es, h))
    w = len(es) + 1
    frames = [chain_frame([(0, es)], w), chain_frame([(0, es[:cut + 1]), (5000, es[:200] % 300)], w), chain_frame([(0, es)], w, start=20000)]
    return Case("dense", frames, limits=(hand, hand + 1, hand - 63, 64 * (hand // 64) - 3), target=(0, 0, 0),
                edges=["halve:mod64=0", "halve:mod64=63", "halve:last-partial", "halve:two-in-block", "halve:mod32=31", "halve:mod32=0",
                       "halve:handover"] + ["halve:mod4=%d" % r for r in range(4)] + ["rule:%s" % r for r in RULES])


def _case_lengths():
    """Chains of every length on the list, and of L - 1, L and L + 1 events for every limit on the list, each in a context of its
    own (multiples of 1000; the by-products of values below 400 never are)."""
    rng = np.random.default_rng(11)
    want = sorted(set(CHAIN_LENGTHS) | {n + d for n in LIMIT_EDGES for d in (-1, 0, 1) if n + d > 0})
    order = [want[i] for i in rng.permutation(len(want))]
    segs = [(1000 * (i + 1), rng.integers(0, 400, size=n)) for i, n in enumerate(order)]
    return Case("lengths", [chain_frame(segs), chain_frame(segs[::-1])], limits=LIMIT_EDGES,
                edges=["len:%d" % n for n in CHAIN_LENGTHS] + ["limit:%d" % n for n in LIMIT_EDGES])


def _case_single():
    """The single-chain frames: every event of a plane in one context, so neighbouring planes of one slope end and begin with the
    same context; halvings at 1024 and 1537 (slope 1), 341, 512 and 683 (slope 3)."""
    w = 1602
    return Case("single", [single_chain_frame(w, 1), single_chain_frame(w, 1), single_chain_frame(w, 3), single_chain_frame(w, 3)],
                limits=(1024, 1025, 341), edges=["planes:shared-context"])


def _case_checker():
    """The 0 / 65 535 checkerboard, 64 x 40: one context-0 chain of 2457 events of one value, halvings at 56, 85 and 114."""
    return Case("checker", [checkerboard(64, 40)] * 2, limits=(85, 86), edges=["planes:shared-context"])


def _case_starts():
    """Contexts 0 .. 4 with 64, 960, 3072, 12288 and 100 events (values from 16 up, so that the first row's by-products have larger
    contexts): chains that start at records 64, 1024, 4096 and 16384 of their plane, which holds more than 16384."""
    rng = np.random.default_rng(13)
    segs = [(c, 16 + mixed_values(rng, n, (3, 8, 5, 11, 2))) for c, n in enumerate((64, 960, 3072, 12288, 100))]
    return Case("starts", [chain_frame(segs), chain_frame(segs, start=28000)], limits=(2048,),
                edges=["start:%d" % o for o in STARTS] + ["records:>16384"])


def _case_levels():
    """Level noise, 128 x 100: contexts that differ in both sort digits, chains of hundreds and thousands of events over two sort
    tiles, and neighbours in a chain whose exchange changes a k -- what a sort that is not stable would do."""
    rng = np.random.default_rng(17)
    frames = [level_noise(rng, 128, 100, LEVELS), level_noise(rng, 128, 100), level_noise(rng, 128, 100, LEVELS)]
    return Case("levels", frames, limits=(96, 1000), target=(0, 0, 513), edges=["sort:stability"] + ["rule:%s" % r for r in RULES])


def _case_tiles():
    """Planes of 4095, 4096 and 4097 records (one, one and two sort tiles) between planes without events: the first group of four
    sort tiles takes in three planes."""
    rng = np.random.default_rng(19)
    w, h = 100, 66
    flat = np.full((h, w), 1234, np.uint16)
    return Case("tiles", [flat] + [noise_with_records(rng, w, h, n) for n in (4095, 4096, 4097)] + [flat, noise_with_records(rng, w, h, 4097), flat],
                limits=(2,), edges=["records:4095", "records:4096", "records:4097", "tiles:straddle", "empty:first", "empty:middle", "empty:last"])


def _case_many():
    """Full-range noise, 256 x 256: eight frames of ~26 000 chains each behind a plane of one sort tile, so that more chains than
    the four-lane kernel's grid takes in one stride come in, more than 8192 of them longer than a limit of 1, and groups of four
    sort tiles begin at a tile of their plane that is no multiple of four."""
    rng = np.random.default_rng(23)
    w = h = 256
    frames = [noise_with_records(rng, w, h, 4000)] + [rng.integers(0, 65536, size=(h, w), dtype=np.uint16) for _ in range(8)]
    return Case("many", frames, limits=(1,), edges=["chains:>150000", "long:>8192", "tiles:unaligned", "tiles:straddle"])


def _case_chroma():
    """RGB16, 8 x 4.  Frame 0: Co holds an event of the largest value there is, 131 069 (both neighbours -65 535, the sample 65 535),
    in context 0 behind an event of value 0, so with k = 0: a code of 2^17 bits; and one of the largest context an event can have,
    131 069 (neighbours -65 535 and 65 534: at 131 070 every sample lies in range).  Frame 1, the batch's last: its Cg plane's largest
    context is that of the poison pattern, and its chain ends at the last record of the buffer."""
    lo, hi = -65535, 65535
    co = np.full((4, 8), lo)
    co[1, 2] = lo + 1          # context 0, value 0: k = 0 from here on
    co[2, 5] = hi              # context 0, value 131 069
    co[3, 1], co[3, 2] = hi - 1, hi  # (3, 2): neighbours 65 534 and -65 535, the sample above both
    a = rgb_from_chroma(co, np.zeros((4, 8), np.int64))
    cg = np.zeros((4, 8), np.int64)
    top = 65535 - POISON_CTX
    cg[1, 3], cg[0, 4] = 65535, top        # (1, 4): left 65 535, above `top`
    cg[1, 4] = top - 500
    cg[2, 5], cg[1, 6] = 65535, top        # a second event of the context, and a third
    cg[2, 6] = top - 3
    cg[3, 2], cg[2, 3] = top, 65535
    cg[3, 3] = top - 70
    b = rgb_from_chroma(np.zeros((4, 8), np.int64), cg)
    return Case("chroma", [a, b], limits=(1, 2), edges=["chroma:largest-fields", "poison:last-context"])


_BUILDERS = {"dense": _case_dense, "lengths": _case_lengths, "single": _case_single, "checker": _case_checker, "starts": _case_starts,
             "levels": _case_levels, "tiles": _case_tiles, "many": _case_many, "chroma": _case_chroma}
NAMES = tuple(_BUILDERS)
_CASES = {}


def case(name):
    if name not in _CASES:
        _CASES[name] = _BUILDERS[name]()
    return _CASES[name]


# ------------------------------------------------------------------------------------------------------------------------
# premises and sensitivity
# ------------------------------------------------------------------------------------------------------------------------

def sort_tile_groups(counts):
    """Per group of four consecutive sort tiles of a batch whose planes hold `counts` records: [(plane, tile within the plane), ...]"""
    tiles = [(p, t) for p, n in enumerate(counts) for t in range(-(-int(n) // SORT_TILE))]
    return [tiles[i:i + 4] for i in range(0, len(tiles), 4)]


def _halving_edge(c, edge):
    es, _ = c.target_values()
    hv = c.target_halvings()
    shows = c.late_shows
    kind = edge.split(":")[1]
    if kind.startswith("mod"):
        m, r = kind[3:].split("=")
        hit = [h for h in hv if h >= int(m) and h % int(m) == int(r)]
        assert hit, (edge, hv)
        assert any(shows(h) for h in hit[:3]), "%s: a late halving at %s changes no k" % (edge, hit[:3])
    elif kind == "two-in-block":
        pairs = [(a, b) for a, b in zip(hv, hv[1:]) if a // 64 == b // 64]
        assert pairs, (edge, hv)
        assert any(shows(b) for _, b in pairs[:3]), edge
        triple = [a for a, b in zip(hv, hv[2:]) if a // 64 == b // 64]
        assert triple, "three halvings in one block: %s" % hv
    elif kind == "handover":
        ok = [h for h in hv if h in c.limits and h + 1 in c.limits and h - 63 in c.limits]
        assert ok and all(shows(h) for h in ok), (edge, c.limits, hv[:20])
        assert any(h % 4 != 0 for h in ok) and any(lim % 32 not in (0, 1) and lim % 4 != 0 for lim in c.limits), c.limits
    elif kind == "last-partial":
        found = False
        for ev in c.trace():
            for ctx, n in zip(ev["chain_ctx"], ev["chain_len"]):
                if n > 64 and n % 64 != 0:
                    h2 = []
                    replay(ev["val"][ev["ctx"] == ctx], halvings=h2)
                    found = found or (bool(h2) and h2[-1] == n - 1)
        assert found, edge


def premises(c):
    """Asserts, from the oracle's trace alone, that case c reaches every edge it claims."""
    tr = c.trace()
    counts = [len(ev["pix"]) for ev in tr]
    lens = np.concatenate([ev["chain_len"] for ev in tr]) if tr else np.zeros(0, np.int64)
    for edge in c.edges:
        kind, _, arg = edge.partition(":")
        if kind == "len":
            assert (lens == int(arg)).any(), edge
        elif kind == "limit":
            lim = int(arg)
            assert lim in c.limits and all((lens == n).any() for n in (lim - 1, lim, lim + 1) if n > 0), edge
        elif kind == "halve":
            _halving_edge(c, edge)
        elif kind == "start":
            assert any(((ev["chain_first"] > 0) & (ev["chain_first"] % int(arg) == 0)).any() for ev in tr), edge
        elif kind == "records":
            assert any(n > 16384 for n in counts) if arg == ">16384" else int(arg) in counts, (edge, counts)
        elif edge == "tiles:straddle":
            assert any(len({p for p, _ in g}) > 1 for g in sort_tile_groups(counts)), (edge, counts)
        elif edge == "tiles:unaligned":
            assert any(len(g) == 4 and len({p for p, _ in g}) == 1 and g[0][1] % 4 != 0 for g in sort_tile_groups(counts)), (edge, counts)
        elif kind == "empty":
            assert max(counts) > 0
            where = {"first": counts[0] == 0, "last": counts[-1] == 0,
                     "middle": any(n == 0 and max(counts[:i]) > 0 and max(counts[i + 1:]) > 0 for i, n in enumerate(counts) if 0 < i < len(counts) - 1)}
            assert where[arg], (edge, counts)
        elif edge == "planes:shared-context":
            assert any(len(a["pix"]) and len(b["pix"]) and a["chain_ctx"][-1] == b["chain_ctx"][0] for a, b in zip(tr, tr[1:])), edge
        elif edge == "chains:>150000":
            assert len(lens) > 150000, (edge, len(lens))
        elif edge == "long:>8192":
            assert any(lim > 0 and int((lens > lim).sum()) > 8192 for lim in c.limits), edge
        elif edge == "chroma:largest-fields":
            assert c.frames[0].ndim == 3
            chroma = [ev for i, ev in enumerate(tr) if i % 3 != 0]
            assert any(((ev["val"] == 131069) & (ev["k"] == 0)).any() for ev in chroma), edge
            assert any((ev["ctx"] == 131069).any() for ev in chroma), edge
        elif edge == "poison:last-context":
            assert c.frames[0].ndim == 3 and tr[-1]["chain_ctx"][-1] == POISON_CTX and tr[-1]["chain_len"][-1] >= 3, (edge, tr[-1]["chain_ctx"])
        elif edge == "sort:stability":
            assert stability_pair(c) is not None, edge
            ctxs = {int(x) for ev in tr for x in ev["chain_ctx"]}
            assert len({x & 511 for x in ctxs}) > 2 and len({x >> 9 for x in ctxs}) > 2, ctxs  # both digits tell the chains apart
            assert all(n > SORT_TILE for n in counts), counts
        elif kind == "rule":
            es, k = c.target_values()
            true = replay(es)
            assert true == k.tolist()
            got = replay(es, arg)
            assert any(a != b for a, b in list(zip(got, true))[1:]), "%s: the %s rule gives the same k behind the chain's first event" % (c.name, arg)
        else:
            raise AssertionError("unknown edge " + edge)


def stability_pair(c):
    """The first neighbours in the target chain with different values whose exchange changes a k."""
    es, _ = c.target_values()
    true = replay(es)
    for i in range(1, min(len(es) - 1, 400)):
        if es[i] != es[i + 1]:
            got = replay(es, "swap", at=i)
            got[i], got[i + 1] = got[i + 1], got[i]  # k by event, not by place
            if got != true:
                return i
    return None


def replay_matches_oracle(c):
    """The Python replay (true rule) gives the oracle's k for every record of every plane of the case."""
    for i, ev in enumerate(c.trace()):
        want = ev["k"][ev["order"]]
        got = replay_records(ev)
        assert (got == want).all(), "%s plane %d: record %d" % (c.name, i, int(np.flatnonzero(got != want)[0]))
