"""What the tests of the GPU decoders' edges share (test_decode_cases_cpu.py, test_decode_edges_gpu.py): the corpus -- every frame of
pack_layout, wide_cases and chain_cases plus frames built here --, a model of the estimator, the placement of a stream in the device
blob, the grids of the decoders' bit readers, the edges a frame reaches under a placement, what must be reached (REQUIRED), and
the corrupt variants of a stream.  Everything comes from the CPU oracle's trace through pack_layout.Layout (first, nbits, val, k,
cls, ctx); nothing here imports the library under test.

THE READERS (felics_gpudecode.hip, felics_lanewalk.h).  ScalarBits, the wave forms' reader, holds the stream in CHUNKS of 64 dwords,
2048 bits, counted from the 4-byte-aligned address at or below the pointer it is given: the payload, s + 14, for k_decode8 and
k_decode16 (grid "p14"), the stream itself, s, for the indexed walks (init_at: grid "s").  With the stream at an address that is a
(mod 4), bit b of the stream lies at b - 112 + 8 ((a + 14) & 3) of grid p14 and at b + 8 a of grid s.  LaneReader has dwords only.

A CODE is what the trace gives per pixel: the two raw samples of a plane (32 bits each), an in-range code (a flag bit, m bits, and
one EXTRA bit for the larger remainders), or a Rice code: two flag bits, a RUN of val >> k ones, a zero and k REMAINDER bits."""
import zlib

import numpy as np

from tests import chain_cases, pack_layout as pl, wide_cases
from tests.pack_layout import CLS_ABOVE, CLS_BELOW, CLS_IN, CLS_RAW, Layout

CHUNK_BITS = 64 * 32
HEADER_BITS = 112
DEC16_SLOTS = 512           # felics_gpudecode.hip: constexpr uint32_t DEC16_SLOTS = 512 (cached rows of k_decode16, direct-mapped)
HALVE = 1024
KINDS = ("gray8", "rgb8", "gray16", "rgb16")
GRIDS = ("p14", "s")
NK = {"gray8": 6, "rgb8": 6, "gray16": 15, "rgb16": 15}
MAX_K0 = {"gray8": 254, "rgb8": 509, "gray16": 65534, "rgb16": 131069}   # the largest coded value of each kind
IN_MAX = {"gray8": 9, "rgb8": 10, "gray16": 17, "rgb16": 18}             # the longest in-range code
LIMIT = {"gray8": 1024, "rgb8": 1024, "gray16": 262144, "rgb16": 262144}  # the decoders' bound on a Rice operand
RUNS = (31, 32, 33, 63, 64, 65)
LANE_MIN_W = 8              # the lane forms take rows of eight samples and more
WAVE16_MAX_W = 16128        # k_decode16's LDS (160 KB: 512 rows of 64 bytes, their tags, two rows of int32 in blocks of 64 samples)
WAVE8_MAX_W = 39424         # k_decode8's: the table of 256 rows (512 would be 36 352) and two rows of int16


def kind_of(img):
    return ("gray", "rgb")[img.ndim == 3] + ("8", "16")[img.dtype == np.uint16]


def depth_of(kind):
    return 16 if kind.endswith("16") else 8


# ------------------------------------------------------------------------------------------------------------------------
# the estimator model
# ------------------------------------------------------------------------------------------------------------------------

def model_plane(ctx, val, nk):
    """The Rice events of one plane in raster order (contexts, coded values) replayed: one row of nk counters per context, k the
    smallest counter with ties to the largest k, S[k] += (e >> k) + 1 + k, all counters halved when the minimum passes 1024.
    Per event: k, `mn` (the minimum behind the update, in front of the halving) and `small` (the smallest k among the minima where
    the tie is between counters that are not zero, else k).  `final`: {context: the k its next event would get}."""
    n = len(ctx)
    out = {"k": np.zeros(n, np.int64), "mn": np.zeros(n, np.int64), "small": np.zeros(n, np.int64), "final": {}}
    if n == 0:
        return out
    order = np.argsort(ctx, kind="stable")
    c, v = ctx[order], val[order]
    first = np.flatnonzero(np.r_[True, c[1:] != c[:-1]])
    length = np.diff(np.r_[first, n])
    by_len = np.argsort(-length, kind="stable")
    first, length = first[by_len], length[by_len]
    S = np.zeros((len(first), nk), np.int64)
    ks = np.arange(nk)
    k, mn, small = (np.zeros(n, np.int64) for _ in range(3))
    for t in range(int(length[0])):
        m = int(np.searchsorted(-length, -t, side="left"))  # chains longer than t: a prefix
        A, at = S[:m], first[:m] + t
        big = nk - 1 - np.argmin(A[:, ::-1], axis=1)
        k[at] = big
        small[at] = np.where(A.min(axis=1) > 0, np.argmin(A, axis=1), big)
        A += (v[at][:, None] >> ks) + 1 + ks
        lo = A.min(axis=1)
        mn[at] = lo
        A[lo > HALVE] >>= 1
    for name, a in (("k", k), ("mn", mn), ("small", small)):
        out[name][order] = a
    out["final"] = dict(zip(c[first].tolist(), (nk - 1 - np.argmin(S[:, ::-1], axis=1)).tolist()))
    return out


def replay_chain(es, nk, at=None, threshold=HALVE, minima=None):
    """k of every event of one context's chain; the halving asks `minimum > threshold` at event `at` alone and > 1024 elsewhere.
    minima: a list that receives the minimum behind every update, in front of the halving."""
    S, out = [0] * nk, []
    for i, e in enumerate(es):
        m = min(S)
        out.append(nk - 1 - S[::-1].index(m))
        S = [s + (int(e) >> k) + 1 + k for k, s in enumerate(S)]
        if minima is not None:
            minima.append(min(S))
        if min(S) > (threshold if i == at else HALVE):
            S = [s >> 1 for s in S]
    return out


THRESHOLD_EDGES = (("est:1024", 1024, 1023), ("est:1025", 1025, 1025))


def threshold_edges(es, nk, true=None):
    """Of one context's chain: "est:1024" -- an update leaves the minimum at exactly 1024, which is not halved, and halving there
    (the threshold moved to 1023 at that event) gives a later event another k; "est:1025" -- it leaves exactly 1025, which is
    halved, and not halving there (the threshold 1025) gives a later event another k."""
    mn = []
    ks = replay_chain(es, nk, minima=mn)
    assert true is None or ks == list(true)
    out = set()
    for name, want, thr in THRESHOLD_EDGES:
        for j in [j for j, m in enumerate(mn) if m == want][:8]:
            if replay_chain(es, nk, at=j, threshold=thr)[j + 1:] != ks[j + 1:]:
                out.add(name)
                break
    return out


# ------------------------------------------------------------------------------------------------------------------------
# frames
# ------------------------------------------------------------------------------------------------------------------------

class Frame:
    """One frame of the corpus: case and index name it (and place it: placement()); the layout and the model are worked out once."""

    def __init__(self, case, index, img):
        self.case, self.index, self.img = case, index, np.ascontiguousarray(img)
        self.kind = kind_of(self.img)
        self.shape = self.img.shape
        self.h, self.w = self.shape[:2]
        self._L = self._codes = self._model = self._fixed = None
        self._reach = {}

    @property
    def key(self):
        return "%s[%d]" % (self.case, self.index)

    @property
    def on_gpu(self):
        """do the device calls decode it in a GPU form?  (rows wider than the wave forms' LDS holds are the host decoder's)"""
        return self.w <= (WAVE16_MAX_W if depth_of(self.kind) == 16 else WAVE8_MAX_W)

    @property
    def lanes(self):
        return self.on_gpu and self.w >= LANE_MIN_W

    def layout(self):
        if self._L is None:
            self._L = Layout(self.img)
        return self._L

    def codes(self):
        """the codes of all planes one behind the other: first, nbits, val, k, cls, ctx, plane, index in the plane"""
        if self._codes is None:
            L = self.layout()
            c = {name: np.concatenate(getattr(L, name)) for name in ("first", "nbits", "val", "k", "cls", "ctx")}
            c["plane"] = np.repeat(np.arange(L.nplanes), L.npix)
            c["pix"] = np.tile(np.arange(L.npix), L.nplanes)
            c["rice"] = ((c["cls"] == CLS_BELOW) | (c["cls"] == CLS_ABOVE)) & (c["pix"] >= 2)
            c["q"] = np.where(c["rice"], c["val"] >> c["k"], 0)
            self._codes = c
        return self._codes

    def events(self, p):
        """plane p's Rice events in raster order: pixel, context, value, traced k"""
        L = self.layout()
        pix = np.flatnonzero(((L.cls[p] == CLS_BELOW) | (L.cls[p] == CLS_ABOVE)) & (np.arange(L.npix) >= 2))
        return pix, L.ctx[p][pix], L.val[p][pix], L.k[p][pix]

    def model(self):
        if self._model is None:
            self._model = [model_plane(ev[1], ev[2], NK[self.kind]) for ev in (self.events(p) for p in range(self.layout().nplanes))]
        return self._model


def model_matches_trace(frame):
    """The model gives the oracle's k for every Rice event of the frame."""
    for p, m in enumerate(frame.model()):
        want = frame.events(p)[3]
        bad = np.flatnonzero(m["k"] != want)
        assert bad.size == 0, "%s plane %d: event %d, model k %d, trace k %d" % (frame.key, p, bad[0], m["k"][bad[0]], want[bad[0]])


# ------------------------------------------------------------------------------------------------------------------------
# the placement
# ------------------------------------------------------------------------------------------------------------------------

ROTATIONS = (0, 1, 2, 3)


def placement(case, index, rot):
    """The address (mod 4) of the stream of frame `index` of `case` in the device blob under rotation rot: a pure function of the
    three, and over the four rotations every stream gets all four."""
    return (zlib.crc32(case.encode()) + index + rot) & 3


def place(frames, streams, rot, tail=16):
    """The device blob of `streams` (the streams of `frames`, in that order) under rotation rot -> (bytes, offsets, lens).  Stream i
    begins at the first offset behind its predecessor that is placement(...) above a multiple of 16; device allocations are
    aligned far beyond that, so the offset modulo 4 is the address modulo 4.  `tail` zero bytes behind the last stream."""
    blob, offs = bytearray(), []
    for f, s in zip(frames, streams):
        blob += bytes((-len(blob)) % 16 + placement(f.case, f.index, rot))
        offs.append(len(blob))
        blob += s
    return bytes(blob) + bytes(tail), offs, [len(s) for s in streams]


def shift_of(grid, a):
    """what to add to a stream bit to get its position in the grid, for a stream at address a (mod 4)"""
    return 8 * ((a + 14) & 3) - HEADER_BITS if grid == "p14" else 8 * a


def total_dw(grid, a, nbytes):
    """ScalarBits::total_dw for a stream of nbytes at address a: the dwords from the aligned address that hold stream bytes"""
    skew, n = (((a + 14) & 3), nbytes - 14) if grid == "p14" else (a, nbytes)
    return (skew + n + 3) >> 2


# ------------------------------------------------------------------------------------------------------------------------
# the edges
# ------------------------------------------------------------------------------------------------------------------------

WHERE = ("in-range", "flags", "run64", "rem", "between")


def _chunk_edges(frame, a, out):
    """Where the chunk boundaries of both grids fall in the stream at address a.  in-range: strictly inside an in-range code; flags:
    between the two flag bits of a Rice code or right behind them; run64: strictly inside a run of 64 ones or more; rem: strictly
    inside the k remainder bits (a remainder bit on either side); between: exactly between two codes; raw: strictly inside
    the 64 bits of a plane's two raw samples."""
    c, L = frame.codes(), frame.layout()
    first = c["first"]
    for grid in GRIDS:
        sh = shift_of(grid, a)
        dw = total_dw(grid, a, L.total_bytes())
        if dw % 64 in (0, 1):
            out.add("end:%s:dw%d" % (grid, dw % 64))
        B = np.arange(-sh % CHUNK_BITS, L.total_bits, CHUNK_BITS)
        B = B[(B > HEADER_BITS) & (B < L.total_bits)]
        if B.size == 0:
            continue
        i = np.searchsorted(first, B, side="right") - 1
        o = B - first[i]
        cls, q, k, rice = c["cls"][i], c["q"][i], c["k"][i], c["rice"][i]
        raw = c["pix"][i] < 2
        hit = {"between": (o == 0) & ~(raw & (c["pix"][i] == 1)),
               "raw": (raw & (o > 0)) | (raw & (c["pix"][i] == 1) & (o == 0)),
               "in-range": (cls == CLS_IN) & ~raw & (o > 0),
               "flags": rice & ((o == 1) | (o == 2)),
               "run64": rice & (q >= 64) & (o > 2) & (o < 2 + q),
               "rem": rice & (o > 3 + q) & (o < 3 + q + k)}
        for name, m in hit.items():
            if m.any():
                out.add("chunk:%s:%s" % (grid, name))


def _fixed_edges(frame):
    """the edges that do not depend on the placement"""
    if frame._fixed is not None:
        return frame._fixed
    out = set()
    c, L, kind = frame.codes(), frame.layout(), frame.kind
    rice, q, k, val = c["rice"], c["q"], c["k"], c["val"]
    if L.total_bits % 8 == 0:
        out.add("end:last-bit")
    if L.total_bits % 8 == 1:
        out.add("end:pad7")
    runs = set(q[rice & (q >= 31) & (q <= 65)].tolist())
    out |= {"run:%d" % r for r in RUNS if r in runs}
    if (rice & (val == MAX_K0[kind]) & (k == 0)).any():
        out.add("max-k0")
    if frame.lanes:  # what the lane step branches on counts where a lane form decodes the frame
        span = q + 1 + k
        if (rice & (span == 30)).any():
            out.add("lane:short30")
        if (rice & (span == 31)).any():
            out.add("lane:long31")
        if (rice & (span > 31)).any():
            out.add("lane:long")
    # in-range codes: m bits for a context of n = ctx + 1 values, one more for the larger remainders
    inr = (c["cls"] == CLS_IN) & (c["pix"] >= 2)
    m = np.floor(np.log2(c["ctx"] + 1.0)).astype(np.int64)
    extra = c["nbits"] - 1 - m
    assert ((extra[inr] == 0) | (extra[inr] == 1)).all()
    if (inr & (c["nbits"] == IN_MAX[kind]) & (extra == 1)).any():
        out.add("in:max-extra")
    if (inr & (m == IN_MAX[kind] - 2) & (extra == 0)).any():
        out.add("in:max-plain")
    # the estimator
    nk = NK[kind]
    reload_, epoch = False, False
    trained = {}
    for p, mdl in enumerate(frame.model()):
        pix, ctx, ev, tk = frame.events(p)
        for x in np.unique(ctx[(mdl["mn"] == 1024) | (mdl["mn"] == 1025)])[:8]:
            if not {"est:1024", "est:1025"} <= out:
                out |= threshold_edges(ev[ctx == x], nk, tk[ctx == x].tolist())
        tie = mdl["small"] != mdl["k"]
        if (tie & ((ev >> mdl["small"]) + mdl["small"] != (ev >> mdl["k"]) + mdl["k"])).any():
            out.add("est:tie")
        if depth_of(kind) == 16 and len(ctx):
            # k_decode16's LDS cache: the event finds another context in its slot, has had an event in this plane, and gets a k other than 14
            slot = ctx & (DEC16_SLOTS - 1)
            order = np.argsort(slot, kind="stable")
            evicted = np.zeros(len(ctx), bool)
            evicted[order[1:]] = (slot[order][1:] == slot[order][:-1]) & (ctx[order][1:] != ctx[order][:-1])
            _, first_at = np.unique(ctx, return_index=True)
            seen = np.ones(len(ctx), bool)
            seen[first_at] = False
            reload_ = reload_ or bool((evicted & seen & (tk != 14)).any())
            # plane epochs: a context trained in the plane in front (its row would give a k other than 14) has its first event here
            epoch = epoch or any(trained.get(int(x), 14) != 14 for x in ctx[first_at])
        trained = mdl["final"]
    if reload_:
        out.add("lds:reload")
    if epoch:
        out.add("lds:epoch")
    frame._fixed = out
    return out


def reached(frame, a):
    """The edges the frame reaches with its stream at address a (mod 4)."""
    if a not in frame._reach:
        out = set(_fixed_edges(frame))
        _chunk_edges(frame, a, out)
        frame._reach[a] = out
    return frame._reach[a]


def _required():
    """{(kind, reader, a): names}.  reader "wave": k_decode8 / k_decode16 (grid p14); "lane": the lane forms; "index": the indexed
    walks (grid s).  a: an address (every name must be reached at that address) or None (at some address)."""
    req = {}
    for kind in KINDS:
        rgb = kind.startswith("rgb")
        for reader, grid in (("wave", "p14"), ("index", "s")):
            for a in range(4):
                req[(kind, reader, a)] = {"chunk:%s:%s" % (grid, w) for w in WHERE + (("raw",) if rgb else ())}
            req[(kind, reader, None)] = set()
        req[(kind, "wave", None)] |= {"run:%d" % r for r in RUNS} | {"max-k0", "in:max-extra", "in:max-plain", "est:1024", "est:1025", "est:tie"}
        req[(kind, "lane", None)] = {"lane:short30", "lane:long31", "lane:long"}
    for depth, kinds in ((8, KINDS[:2]), (16, KINDS[2:])):
        # the stream's end: once per depth and grid, whatever the colour -- carried by the gray kind's entry, checked over both
        for reader, grid in (("wave", "p14"), ("index", "s")):
            req[("depth%d" % depth, reader, None)] = {"end:%s:dw0" % grid, "end:%s:dw1" % grid, "end:last-bit", "end:pad7"}
    req[("gray16", "wave", None)] |= {"lds:reload"}
    req[("rgb16", "wave", None)] |= {"lds:reload", "lds:epoch"}
    return req


REQUIRED = _required()


def missing(frames):
    """What of REQUIRED the frames (those a GPU form decodes) do not reach under the committed placement: [(kind, reader, a, name)]."""
    got = {}
    for f in frames:
        if not f.on_gpu:
            continue
        for rot in ROTATIONS:
            a = placement(f.case, f.index, rot)
            r = reached(f, a)
            for who in (f.kind, "depth%d" % depth_of(f.kind)):
                for reader in ("wave", "lane", "index"):
                    got.setdefault((who, reader, a), set()).update(r)
                    got.setdefault((who, reader, None), set()).update(r)
    return sorted((kind, reader, -1 if a is None else a, name) for (kind, reader, a), names in REQUIRED.items()
                  for name in names - got.get((kind, reader, a), set()))


# ------------------------------------------------------------------------------------------------------------------------
# new frames
# ------------------------------------------------------------------------------------------------------------------------

def zeros_spike(w, at, dtype=np.uint8):
    """One row of zeros with a sample of 1 (context 0 learns k = 0) and a full-scale sample at pixel `at`: the largest value a gray
    sample can code, at k = 0 -- a run of 254 (65 534) ones"""
    f = np.zeros((1, w), dtype)
    f[0, 4] = 1
    f[0, at] = 65535 if dtype == np.uint16 else 255
    return f


def primed_spikes(shape, dtype, base, n, seed):
    """A flat frame of `base` with one sample of base + 1 in front (context 0 learns k = 0) and n full-scale samples behind it."""
    rng = np.random.default_rng(seed)
    f = np.full(shape, base, dtype)
    h, w = shape[:2]
    f[0, 3] = base + 1
    top = 65535 if dtype == np.uint16 else 255
    f[rng.integers(1, h, n), rng.integers(0, w, n)] = top
    return f


def run_frame(kind, runs, width=None):
    """A two-row frame whose second row holds, in context 0 behind an event of value 0 (k = 0), events of the values in `runs` each
    followed by enough events of value 0 to bring k back to 0: runs of exactly those lengths.  Gray: the frame; RGB: its Co plane."""
    es = [0]
    for r in runs:
        es += [r] + [0] * (r + 4)
    n = len(es) + 2
    if kind == "gray16":
        return wide_cases.chain_frame([(0, es)], width or n)
    if kind == "gray8":
        return chain_cases.chain_frame8([(0, es)], width or n + 2)
    row = chain_cases.co_row(width or n + 2) if kind == "rgb8" else chain_cases.Row(width or n + 2, -65535, 65535, 0)
    row.events(0, es)
    co = row.plane()
    if kind == "rgb8":
        return chain_cases.rgb_frame(row)
    return wide_cases.rgb_from_chroma(co, np.zeros_like(co))


def _halving_values(seed, n=600):
    return wide_cases.mixed_values(np.random.default_rng(seed), n, (1, 9, 2, 0, 7, 11, 3, 1, 6))


def halving_rgb16(seed):
    """RGB16 whose Co plane holds one context-0 chain of events of mixed magnitudes: the counters pass 1024 again and again."""
    es = _halving_values(seed)
    row = chain_cases.Row(len(es) + 4, -65535, 65535, 0)
    row.events(0, es)
    co = row.plane()
    return wide_cases.rgb_from_chroma(co, np.zeros_like(co))


def _halving_seeds(seeds=range(400)):
    """One seed per edge of THRESHOLD_EDGES: the first whose chain reaches it (searched, not hoped for)."""
    found = {}
    for seed in seeds:
        for name in threshold_edges(_halving_values(seed), 15):
            found.setdefault(name, seed)
        if len(found) == len(THRESHOLD_EDGES):
            return sorted(set(found.values()))
    raise AssertionError("no seed reaches %s" % sorted({n for n, _, _ in THRESHOLD_EDGES} - set(found)))


def _new_frames():
    out = []

    def add(case, frames):
        out.extend(Frame("new:" + case, i, f) for i, f in enumerate(frames))

    # gray8: a run of 254 ones (the largest value at k = 0) across the chunk boundaries of both grids at every address -- they lie
    # between bits 2024 and 2160 of the stream; a zero costs one bit, so the spike's pixel moves its run by a bit
    at = pl.search(lambda s: zeros_spike(4096, s), lambda L: L.run(0, int(np.argmax(L.nbits[0][2:])) + 2)[0], 1930, 2000, 1800)
    add("zeros8", [zeros_spike(4096, at)])
    add("zeros16", [zeros_spike(300, 200, np.uint16)])
    # the runs the 8-bit corpora lack, and the lane step's last short and first long code, from made-to-order chains
    for kind in KINDS:
        add("runs-" + kind, [run_frame(kind, RUNS), run_frame(kind, (27, 28, 29, 30))])
    # rgb16: halvings, with the minimum on exactly 1024 and on exactly 1025
    add("halving-rgb16", [halving_rgb16(seed) for seed in _halving_seeds()])
    # RGB: a chunk boundary inside the two raw samples of plane 1.  A flat row of w pixels puts them at bits w + 174 .. w + 238; the
    # first boundaries lie at bits 2024 .. 2048 (grid s) and 2136 .. 2160 (grid p14) of the stream
    for dtype, tag in ((np.uint8, "8"), (np.uint16, "16")):
        add("raw" + tag, [pl.flat(2000 - 174, 1, dtype, True), pl.flat(2110 - 174, 1, dtype, True)])
    # the frames the older tests call spikes, primed so that they hold the runs their comments name
    add("spikes8", [primed_spikes((96, 257), np.uint8, 7, 200, 7)])
    add("spikes16", [primed_spikes((40, 300), np.uint16, 9, 60, 12)])
    return out


def _flat_ends():
    """Flat frames (a bit a pixel) of every length around 256 and 512 stream bytes: the streams whose last dword is lane 63 of a
    chunk, or lane 0 of the next, under some placement; and every count of padding bits."""
    out = []
    for dtype, tag in ((np.uint8, "8"), (np.uint16, "16")):
        frames = [pl.flat(w, 1, dtype) for nbytes in (252, 256, 268, 272) for w in (8 * nbytes - 174, 8 * nbytes - 173)]
        out.extend(Frame("new:ends" + tag, i, f) for i, f in enumerate(frames))
    return out


# ------------------------------------------------------------------------------------------------------------------------
# the corpus
# ------------------------------------------------------------------------------------------------------------------------

_CORPUS = None


def corpus():
    """Every frame of pack_layout.NAMES, wide_cases.NAMES and chain_cases.NAMES, and the new ones."""
    global _CORPUS
    if _CORPUS is None:
        out = []
        for mod, tag in ((pl, "pack"), (wide_cases, "wide"), (chain_cases, "chain")):
            for name in mod.NAMES:
                out.extend(Frame("%s:%s" % (tag, name), i, f) for i, f in enumerate(mod.case(name).frames))
        _CORPUS = out + _new_frames() + _flat_ends()
    return _CORPUS


def of_kind(kind):
    return [f for f in corpus() if f.kind == kind]


def groups(frames):
    """the frames by shape: [[frames of one shape and type], ...], in the order of each shape's first frame"""
    by = {}
    for f in frames:
        by.setdefault((f.kind, f.shape), []).append(f)
    return list(by.values())


def shared_trained_contexts(first, second):
    """Contexts of plane 0 that `first` leaves trained (the row would give a k other than 14) and `second` -- decoded by the next call
    on the same tables -- uses: a row of the earlier epoch read as this one's would show in k."""
    trained = {c for c, k in first.model()[0]["final"].items() if k != 14}
    return sorted(trained & set(second.events(0)[1].tolist()))


# ------------------------------------------------------------------------------------------------------------------------
# corrupt variants
# ------------------------------------------------------------------------------------------------------------------------

def longest_run_at_k0(img):
    """the ones of the longest run among the frame's Rice codes with k = 0 (0: there is none), from the oracle's trace"""
    c = Frame("", 0, img).codes()
    sel = c["rice"] & (c["k"] == 0)
    return int(c["q"][sel].max()) if sel.any() else 0


def _bits_to_bytes(bits):
    return np.packbits(np.asarray(bits, np.uint8)).tobytes()


def longest_run(frame):
    """(first bit of the run, ones) of the frame's longest run"""
    c = frame.codes()
    i = int(np.argmax(c["q"]))
    return int(c["first"][i]) + 2, int(c["q"][i])


def variant_frames(kind):
    """The frames whose corrupt variants run: of each kind the smallest one that a lane form takes too, holds a run of 200 ones or
    more, and whose stream is longer than a chunk."""
    ok = [f for f in of_kind(kind) if f.lanes and longest_run(f)[1] >= 200 and f.layout().total_bytes() > 600]
    return sorted(ok, key=lambda f: (f.w * f.h, f.key))[:1]


def tail(frame, stream, operand_above, k_want=None):
    """A hand-assembled tail: the stream up to its first Rice code whose traced k is k_want (any k: None), then that code's two flag
    bits, a run of (operand_above >> k) + 1 ones, the zero, k zero bits -- an operand just above operand_above -- and zero bytes,
    64 at least, so that no length check can fire: the operand's bound is the one check left."""
    c = frame.codes()
    sel = np.flatnonzero(c["rice"] & ((c["k"] == k_want) if k_want is not None else True))
    i = int(sel[0])
    at, k = int(c["first"][i]), int(c["k"][i])
    head = np.unpackbits(np.frombuffer(stream, np.uint8))[:at + 2]
    run = (operand_above >> k) + 1
    assert (run << k) > operand_above
    out = _bits_to_bytes(np.concatenate([head, np.ones(run, np.uint8), np.zeros(1 + k, np.uint8)]))
    # (zeros: 64 bytes, and as many as give the stream a bit for every sample -- the host decoder refuses a shorter one unread)
    return out + bytes(max(64, frame.img.size // 8 + 64 - len(out)))


def variants(frame, stream, a):
    """[(name, bytes)]: the corrupt variants of the frame's stream, placed at address a (mod 4): cut by one byte; cut in the middle
    of the longest run; cut so that it ends exactly on a chunk boundary of each grid (the last one inside the stream); the tails."""
    out = [("cut-1", stream[:-1])]
    rs, q = longest_run(frame)
    if q >= 8:
        out.append(("cut-run", stream[:(rs + q // 2) // 8]))
    for grid in GRIDS:
        sh = shift_of(grid, a)
        n = ((len(stream) * 8 + sh) // CHUNK_BITS * CHUNK_BITS - sh) // 8
        if 14 < n < len(stream):
            out.append(("cut-chunk-" + grid, stream[:n]))
    out.append(("tail-limit", tail(frame, stream, LIMIT[frame.kind])))
    if depth_of(frame.kind) == 16:
        out.append(("tail-2^32", tail(frame, stream, (1 << 32) - 1, k_want=14)))
    return out
