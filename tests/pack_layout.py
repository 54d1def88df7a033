"""What the tests of the two-pass pack share (test_pack_layout_cpu.py, test_two_pass_pack.py): a model of where every code of a stream
lies, from the CPU oracle's per-pixel code lengths alone, the edges of the pack kernels worked out from that model, and frames built
to reach them.  Nothing here imports the library under test.

THE MODEL.  Per plane (the frame itself, or Y / Co / Cg), trace_channel gives every pixel's code length; a TILE is 4096 consecutive
pixels of a plane; the 112 header bits belong to tile 0 of plane 0; tiles and planes lie back to back with no alignment, and the
stream is the total rounded up to bytes.  The pack kernel works on 32-bit WORDS of the stream: a tile's workgroup packs the words
first_word = lo >> 5 .. last_word = (hi - 1) >> 5 in WINDOWS of 2048 words counted from first_word, every thread the codes of a
GROUP of sixteen pixels, and only a tile's first and last word can be shared with a neighbour.  A Rice code longer than 32 bits is
written as two flag bits, a RUN of val >> k ones and k + 1 bits behind it; a LONG code here is one of 60 000 bits or more."""
import numpy as np

from tests import oracle_lib
from tests.wide_cases import planes_of

TILE = 4096
GROUP = 16
WIN_WORDS = 2048
WIN_BITS = WIN_WORDS * 32
HEADER_BITS = 8 * 14
LONG = 60000
CLS_IN, CLS_BELOW, CLS_ABOVE, CLS_RAW = 0, 1, 2, 3


# ------------------------------------------------------------------------------------------------------------------------
# the layout
# ------------------------------------------------------------------------------------------------------------------------

class Layout:
    """first[p][i], nbits[p][i]: the first bit in the image stream and the length of the code of pixel i of plane p; val, k, cls, ctx:
    the trace; tiles[p][t] = (lo, hi): the tile's bits [lo, hi) in the stream; plane_lo[p]; total_bits."""

    def __init__(self, img):
        o = oracle_lib.load()
        h, w = img.shape[:2]
        assert w * h >= 2, "a frame of one pixel has a literal second sample: not modelled"
        depth = 1 if img.dtype == np.uint16 else 0
        self.shape, self.npix, self.depth = img.shape, w * h, depth
        self.first, self.nbits, self.val, self.k, self.cls, self.ctx, self.tiles, self.plane_lo = [], [], [], [], [], [], [], []
        at = 0
        for p, plane in enumerate(planes_of(img)):
            tr = o.trace_channel(plane, w, h, depth)
            nb = tr["nbits"].astype(np.int64)
            self.plane_lo.append(at)
            start = at + (HEADER_BITS if p == 0 else 0)
            first = start + np.concatenate([[0], np.cumsum(nb)[:-1]])
            end = start + int(nb.sum())
            edges = [at] + [int(first[a]) for a in range(TILE, self.npix, TILE)] + [end]
            self.tiles.append(list(zip(edges[:-1], edges[1:])))
            self.first.append(first)
            self.nbits.append(nb)
            for name in ("val", "k", "cls", "ctx"):
                getattr(self, name).append(tr[name].astype(np.int64))
            at = end
        self.total_bits = at
        self.nplanes, self.ntiles = len(self.tiles), len(self.tiles[0])

    def total_bytes(self):
        return (self.total_bits + 7) // 8

    def all_tiles(self):
        return [(p, t) for p in range(self.nplanes) for t in range(self.ntiles)]

    def has_successor(self, p, t):
        return t < self.ntiles - 1 or p < self.nplanes - 1

    # ---- words and windows of a tile
    def words(self, p, t):
        lo, hi = self.tiles[p][t]
        return lo >> 5, (hi - 1) >> 5

    def start_bit(self, p, t):
        """the position (0 .. 31) of the tile's first bit in its first word"""
        return self.tiles[p][t][0] & 31

    def in_one_word(self, p, t):
        fw, lw = self.words(p, t)
        return fw == lw

    def windows(self, p, t):
        fw, lw = self.words(p, t)
        return (lw - fw) // WIN_WORDS + 1

    def window_of(self, p, t, bit):
        return ((bit >> 5) - self.words(p, t)[0]) // WIN_WORDS

    def word_in_window(self, p, t, bit):
        return ((bit >> 5) - self.words(p, t)[0]) % WIN_WORDS

    def boundaries(self, p, t):
        """the first bit of every window of the tile behind its first"""
        fw = self.words(p, t)[0]
        return [(fw + WIN_WORDS * j) * 32 for j in range(1, self.windows(p, t))]

    def pixels(self, p, t):
        return t * TILE, min((t + 1) * TILE, self.npix)

    # ---- codes
    def run(self, p, i):
        """[start, end) of the run of ones of pixel i's code (a Rice code), in stream bits"""
        assert self.cls[p][i] in (CLS_BELOW, CLS_ABOVE)
        s = int(self.first[p][i]) + 2
        return s, s + int(self.val[p][i] >> self.k[p][i])

    def long_codes(self, p, t=None):
        a, b = (0, self.npix) if t is None else self.pixels(p, t)
        return [int(i) + a for i in np.flatnonzero(self.nbits[p][a:b] >= LONG)]

    def group_totals(self, p):
        """bits of every thread's group of sixteen pixels of plane p (the header in the first group of plane 0)"""
        nb = self.nbits[p]
        pad = (-len(nb)) % GROUP
        tot = np.concatenate([nb, np.zeros(pad, np.int64)]).reshape(-1, GROUP).sum(1)
        if p == 0:
            tot[0] += HEADER_BITS
        return tot


def layout(oracle, img):
    """The layout of img's stream (oracle: the loaded CPU oracle; the trace comes from it and from nothing else)."""
    assert oracle is oracle_lib.load()
    return Layout(np.ascontiguousarray(img))


# ------------------------------------------------------------------------------------------------------------------------
# the edges a frame reaches
# ------------------------------------------------------------------------------------------------------------------------

EDGES = (
    # windows: a tile of two, of three or more; what lies on a window boundary: the boundary between two codes, a code of at most 32
    # bits, a run; a group with whole codes on both sides; the boundary between two groups
    "win:2", "win:3+", "bound:code", "bound:short", "bound:run", "bound:group", "bound:group-edge",
    # long codes: the run from window 0 into window 1, beginning in the last word of a window, ending in the first word of one, the
    # code inside one window, the run covering a whole window, a long code with k >= 1 and a remainder that is not 0, two in one
    # group, as the last pixel of a tile, the first of the next, the last of a plane whose successor starts in the code's last word
    "run:w0-w1", "run:starts-last-word", "run:ends-first-word", "run:inside", "run:covers", "run:rem", "run:two-in-group",
    "run:tile-last", "run:tile-first", "run:plane-last",
    # shared words: a tile inside one word that it shares with its predecessor (-first), with its successor too (-both), one that
    # fills its predecessor's word to the last bit, one that starts on bit 0 and is shorter than a word, one shorter than a word
    # that lies in two, one whose successor starts on bit 0, a word that three tiles write
    "tile:inside-shared-first", "tile:inside-shared-both", "tile:fills-word", "tile:bit0-short", "tile:short-two-words", "tile:ends-aligned",
    "word:three-tiles",
    # over the frames of a case: every position 0 .. 31 of the first bit of tile 1 of plane 0; of plane 1 and of plane 2
    "align:tile1-all32", "align:planes-all32",
    # 8-bit: sixteen of the longest chroma codes in one group, against the 16-bit group totals of the 8-bit instantiations
    "u16:group-max",
)
U16_GROUP_MIN = 16 * 480  # "sixteen of the longest codes": every code of the group within 30 bits of the longest there is (2 + 509 + 1)


def frame_edges(L):
    """The edges (of EDGES, those of one frame) that the frame with layout L reaches."""
    out = set()
    touched = {}
    for p, t in L.all_tiles():
        lo, hi = L.tiles[p][t]
        fw, lw = L.words(p, t)
        a, b = L.pixels(p, t)
        first, nb = L.first[p][a:b], L.nbits[p][a:b]
        nwin = L.windows(p, t)
        if nwin == 2:
            out.add("win:2")
        if nwin >= 3:
            out.add("win:3+")
        for B in L.boundaries(p, t):
            i = int(np.searchsorted(first, B, side="right")) - 1  # the code that holds bit B, or starts there
            if i < 0:
                continue
            g0 = i // GROUP * GROUP
            if first[i] == B:
                out.add("bound:code")
                if i == g0:
                    out.add("bound:group-edge")
            elif nb[i] <= 32:
                out.add("bound:short")
            elif L.cls[p][a + i] != CLS_RAW:
                rs, re = L.run(p, a + i)
                if rs < B < re:
                    out.add("bound:run")
            g1 = min(g0 + GROUP, b - a)
            ends = first[g0:g1] + nb[g0:g1]
            if (ends <= B).any() and (first[g0:g1] >= B).any():
                out.add("bound:group")
        longs = L.long_codes(p, t)
        for i in longs:
            rs, re = L.run(p, i)
            ws, we = L.window_of(p, t, rs), L.window_of(p, t, re - 1)
            c0, c1 = int(L.first[p][i]), int(L.first[p][i] + L.nbits[p][i])
            if ws == 0 and we == 1:
                out.add("run:w0-w1")
            if we > ws and L.word_in_window(p, t, rs) == WIN_WORDS - 1:
                out.add("run:starts-last-word")
            if we > ws and L.word_in_window(p, t, re - 1) == 0:
                out.add("run:ends-first-word")
            if L.window_of(p, t, c0) == L.window_of(p, t, c1 - 1):
                out.add("run:inside")
            if any(rs <= (fw + WIN_WORDS * j) * 32 and re >= (fw + WIN_WORDS * (j + 1)) * 32 for j in range(nwin)):
                out.add("run:covers")
            k = int(L.k[p][i])
            if k >= 1 and int(L.val[p][i]) & ((1 << k) - 1):
                out.add("run:rem")
            if i == b - 1 and t < L.ntiles - 1:
                out.add("run:tile-last")
            if i == a and t >= 1:
                out.add("run:tile-first")
            if i == L.npix - 1 and p < L.nplanes - 1 and c1 & 31:
                out.add("run:plane-last")
        if len({i // GROUP for i in longs}) < len(longs):
            out.add("run:two-in-group")
        one = fw == lw
        if one and lo & 31 and hi & 31:
            out.add("tile:inside-shared-first")
            if L.has_successor(p, t):
                out.add("tile:inside-shared-both")
        if one and lo & 31 and not hi & 31:
            out.add("tile:fills-word")
        if not lo & 31 and hi - lo < 32:
            out.add("tile:bit0-short")
        if hi - lo < 32 and not one:
            out.add("tile:short-two-words")
        if not hi & 31 and L.has_successor(p, t):
            out.add("tile:ends-aligned")
        for w in {fw, lw}:
            touched[w] = touched.get(w, 0) + 1
    if max(touched.values()) >= 3:
        out.add("word:three-tiles")
    if L.nplanes == 3 and L.depth == 0:  # (8-bit chroma: no code is longer than 512 bits)
        tot = np.concatenate([L.group_totals(p) for p in range(3)])
        assert tot.max() < 65536
        if tot.max() >= U16_GROUP_MIN:
            out.add("u16:group-max")
    return out


def tile1_alignments(layouts):
    return {L.start_bit(0, 1) for L in layouts if L.ntiles > 1}


def plane_alignments(layouts, p):
    return {L.plane_lo[p] & 31 for L in layouts if L.nplanes == 3}


# ------------------------------------------------------------------------------------------------------------------------
# constructions
# ------------------------------------------------------------------------------------------------------------------------

BASE16, BASE8 = 1000, 9


def flat(w, h, dtype=np.uint16, rgb=False):
    """A constant frame: every code behind the first two samples is one bit."""
    v = BASE16 if dtype == np.uint16 else BASE8
    return np.full((h, w, 3) if rgb else (h, w), v, dtype)


def bump(img, i, by=1):
    """Pixel i (raster index) `by` above its flat surroundings: an event of context 0 and value by - 1, and longer codes for the
    neighbours that see it (an RGB frame: all three samples, so only the Y plane changes)."""
    w = img.shape[1]
    img[i // w, i % w] += by


def prime(img, i=None):
    """Two pixels v + 1, v + 2 side by side in a flat row: an event of value 0 in context 0 and one in context 1, each the first of its
    context, so that both contexts code their next event with k = 0."""
    w = img.shape[1]
    i = w + 2 if i is None else i
    bump(img, i, 1)
    bump(img, i + 1, 2)


def spike(img, i, ctx=0):
    """A full-scale sample at pixel i of a flat region, in context 0 (both neighbours flat) or 1 (the pixel in front of it one above
    the flat value); behind prime() and in front of any other spike of that context it costs a code of ~64 500 bits."""
    w = img.shape[1]
    if ctx == 1:
        bump(img, i - 1, 1)
    img[i // w, i % w] = 65535


def quiet16(w, h, spikes=(), bumps=(), rgb=False):
    """A flat gray16 (or gray RGB16: r = g = b) frame, primed, with bumps (pixel indices) and spikes ((pixel index, context))."""
    img = flat(w, h, np.uint16, rgb)
    prime(img)
    for i in bumps:
        bump(img, i)
    for i, ctx in spikes:
        spike(img, i, ctx)
    return img


def rgb_of_chroma(co, cg, dtype):
    """An RGB frame with the given Co and Cg planes (int arrays of one shape); every sample must fit the type."""
    top = 65535 if dtype == np.uint16 else 255
    co, cg = np.asarray(co, np.int64), np.asarray(cg, np.int64)
    b = np.where(co < 0, -co, 0)
    r = b + co
    g = cg + b + np.trunc(co / 2).astype(np.int64)
    lift = np.maximum(0, -g)
    img = np.stack([r + lift, g + lift, b + lift], axis=-1)
    assert img.min() >= 0 and img.max() <= top, (img.min(), img.max())
    return img.astype(dtype)


def chroma16(w, h, at, first_value):
    """RGB16 whose Co plane is flat at -65 535 with one event of `first_value` in context 0 (value 0: k = 0 behind it; value 1: k = 1)
    and the sample 65 535 at pixel `at`: the largest coded value there is, 131 069, in context 0."""
    co = np.full((h, w), -65535, np.int64)
    co[1, 2] += 1 + first_value
    co[at // w, at % w] = 65535
    return rgb_of_chroma(co, np.zeros((h, w), np.int64), np.uint16)


def chroma8_longest(w=176):
    """RGB8, w x 5, one tile a plane; the Co plane.  Row 0: flat at -255.  Row 1: a staircase -255, -255, -254, -253 ... up to -128:
    the left neighbour of a step is x - 2 above the flat row and the step one above that, so every step is the one event, of value
    0, of context x - 2 -- every context from 0 up codes its next event with k = 0.  Row 2 repeats row 1 (a sample that equals the
    one above it is no event).  Rows 3 and 4, from a pixel of row 4 whose index is a multiple of sixteen: an event in each of the
    contexts 0 .. 15 that swings from one end of the samples' range to the other (the samples above them, in row 3, see -128 above
    themselves: contexts of 100 and more; the swing starts a pixel early, in context 100).  Sixteen of the longest codes 8-bit
    samples have, ~510 bits each, in one thread's group.  Returns the frame and the index of the group's first pixel."""
    co = np.full((5, w), -255, np.int64)
    steps = 128
    co[1, 1:steps + 1] = -255 + np.arange(steps)
    co[1, steps + 1:] = v = -255 + steps - 1
    co[2:5] = co[1]
    x0 = w - 2 * GROUP
    assert (4 * w + x0) % GROUP == 0 and x0 > steps + 1
    lead = GROUP + 2  # rows 3 and 4 leave v by the same kind of staircase, so that the swing's first sample has left the contexts 0 .. 15
    co[3:5, x0 - 1 - lead:x0 - 1] = v + 1 + np.arange(lead)
    left = v + lead
    for x, c in enumerate([100] + list(range(GROUP)), x0 - 1):  # (context 100 first: the sample above the next event then sees v and v + 100)
        above = left + c if left + c <= 255 else left - c
        p = 255 if 255 - max(left, above) > min(left, above) + 255 else -255
        co[3, x], co[4, x] = above, p
        left = p
    co[3:5, x0 + GROUP:] = left
    return rgb_of_chroma(co, np.zeros((5, w), np.int64), np.uint8), 4 * w + x0


def search(build, measure, want_lo, want_hi, start, tries=12):
    """The parameter s (a pixel index: one flat pixel more in front is one bit more) at which want_lo <= measure(layout of build(s))
    <= want_hi, found by stepping s by what is missing."""
    s = start
    for _ in range(tries):
        L = Layout(build(s))
        m = measure(L)
        if want_lo <= m <= want_hi:
            return s
        s += want_lo - m if m < want_lo else want_hi - m
    raise AssertionError("no parameter found: %s last gave %d, wanted %d .. %d" % (s, m, want_lo, want_hi))


def bump_sites(w, h, last_column=False):
    """Pixels of a flat frame, in raster order, whose bumps do not see each other (nor the pixels of prime()): every third column of
    the odd rows from row 3, or the last column of the even rows from row 4 (no right neighbour: a bump there lengthens one code
    fewer)."""
    if last_column:
        return [y * w + w - 1 for y in range(4, h - 1, 2)]
    return [y * w + x for y in range(3, h - 1, 2) for x in range(3, w - 3, 3)]


def first_long(L, p=0, n=0):
    """(first bit, one past the last bit) of the n-th long code of plane p"""
    i = L.long_codes(p)[n]
    return int(L.first[p][i]), int(L.first[p][i] + L.nbits[p][i])


# ------------------------------------------------------------------------------------------------------------------------
# cases
# ------------------------------------------------------------------------------------------------------------------------

QW, QH = 70, 64  # the quiet gray16 frames: 4480 pixels, two tiles, the tile boundary in the middle of a row


class Case:
    """frames: what the case encodes, in this order (batches(): the runs of one shape and type, one call each).  edges: what the case
    reaches -- reached() works it out from the oracle, and test_pack_layout_cpu.py asserts that the two are equal."""

    def __init__(self, name, frames, edges):
        self.name, self.frames, self.edges = name, [np.ascontiguousarray(f) for f in frames], frozenset(edges)
        self._layouts = None

    def layouts(self):
        if self._layouts is None:
            self._layouts = [Layout(f) for f in self.frames]
        return self._layouts

    def reached(self):
        Ls = self.layouts()
        out = set().union(*(frame_edges(L) for L in Ls))
        if tile1_alignments(Ls) == set(range(32)):
            out.add("align:tile1-all32")
        if plane_alignments(Ls, 1) == set(range(32)) and plane_alignments(Ls, 2) == set(range(32)):
            out.add("align:planes-all32")
        return out

    def batches(self):
        out = []
        for f in self.frames:
            if out and out[-1][0].shape == f.shape and out[-1][0].dtype == f.dtype:
                out[-1].append(f)
            else:
                out.append([f])
        return out


def _noise_frames(want, shape, seeds=range(400)):
    """One full-range noise frame per edge of `want`: the first seed whose frame reaches it (searched, not hoped for)."""
    out = []
    for edge in want:
        for seed in seeds:
            f = np.random.default_rng(seed).integers(0, 65536, size=shape, dtype=np.uint16)
            if edge in frame_edges(Layout(f)):
                out.append(f)
                break
        else:
            raise AssertionError("no seed reaches " + edge)
    return out


def _case_noise16():
    """Full-range noise, 64 x 65: tile 0 of every plane holds ~70 000 bits, two windows.  Gray: a frame whose window boundary is the
    boundary between two codes, and one where a short code lies across it.  RGB: the same through the i32 planes."""
    frames = _noise_frames(("bound:code", "bound:short"), (65, 64)) + _noise_frames(("bound:code",), (65, 64, 3))
    return Case("noise16", frames, ["win:2", "bound:code", "bound:short", "bound:group", "tile:ends-aligned"])


def _spike_ending_at(end):
    """The quiet frame whose spike's code ends at bit `end` of the stream"""
    s = search(lambda s: quiet16(QW, QH, spikes=[(s, 0)]), lambda L: first_long(L)[1], end, end, 790)
    return quiet16(QW, QH, spikes=[(s, 0)])


def _group_edge_frame():
    """A spike that is the last pixel of its group and whose code ends on the last bit of window 0: the pixel index is fixed by the
    group, so the bits in front of it are made up with bumps (four bits each, three in the last column)."""
    sites4, sites3 = bump_sites(QW, 10), bump_sites(QW, 10, last_column=True)
    for s in range(799, 700, -GROUP):
        need = WIN_BITS - first_long(Layout(quiet16(QW, QH, spikes=[(s, 0)])))[1]
        for b in range(4):
            a, r = divmod(need - 3 * b, 4)
            if need - 3 * b >= 0 and r == 0 and a <= len(sites4):
                f = quiet16(QW, QH, spikes=[(s, 0)], bumps=sites4[:a] + sites3[:b])
                if first_long(Layout(f))[1] == WIN_BITS:
                    return f
    raise AssertionError("no spike ends its group and its window at once")


def _case_windows16():
    """Quiet gray16 frames, 70 x 64, one ~64 537-bit code each in tile 0 (two windows): the code ends on the last bit of window 0 and
    the next starts window 1; it ends five bits earlier and the short code behind it lies across the boundary; it is the last
    of its group as well, so that a thread ends with the window; it lies across the boundary itself.  Two such codes: three windows."""
    frames = [_spike_ending_at(WIN_BITS), _spike_ending_at(WIN_BITS - 5), _group_edge_frame(), quiet16(QW, QH, spikes=[(2000, 0)]),
              quiet16(QW, QH, spikes=[(1500, 0), (1530, 1)])]
    return Case("windows16", frames, ["win:2", "win:3+", "bound:code", "bound:short", "bound:run", "bound:group", "bound:group-edge",
                                      "run:w0-w1", "run:inside", "tile:ends-aligned"])


def _case_runs16():
    """The long code in every position: from window 0 into window 1; a second one whose run begins in the last word of window 0; one
    whose run ends in the first word of window 1; one inside window 0; two in one group; the last pixel of tile 0; the first of
    tile 1; and, RGB, the last pixel of the Y plane with Co starting in the code's last word."""
    def second_run_start(L):
        return L.run(0, L.long_codes(0)[1])[0]

    def two(s):
        return quiet16(QW, QH, spikes=[(s, 0), (s + 40, 1)])

    def run_last_bit(L):
        return L.run(0, L.long_codes(0)[0])[1] - 1

    s2 = search(two, second_run_start, WIN_BITS - 32, WIN_BITS - 1, 700)
    s3 = search(lambda s: quiet16(QW, QH, spikes=[(s, 0)]), run_last_bit, WIN_BITS, WIN_BITS + 31, 800)
    last = quiet16(QW, QH, spikes=[(QW * QH - 1, 0)], rgb=True)
    if not first_long(Layout(last))[1] & 31:
        last = quiet16(QW, QH, spikes=[(QW * QH - 1, 0)], bumps=bump_sites(QW, QH)[:1], rgb=True)
    frames = [quiet16(QW, QH, spikes=[(2000, 0)]), two(s2), quiet16(QW, QH, spikes=[(s3, 0)]), quiet16(QW, QH, spikes=[(300, 0)]),
              quiet16(QW, QH, spikes=[(1602, 0), (1606, 1)]), quiet16(QW, QH, spikes=[(TILE - 1, 0)]), quiet16(QW, QH, spikes=[(TILE, 0)]), last]
    return Case("runs16", frames, ["win:2", "win:3+", "bound:code", "bound:run", "bound:group", "run:w0-w1", "run:starts-last-word",
                                   "run:ends-first-word", "run:inside", "run:two-in-group", "run:tile-last", "run:tile-first", "run:plane-last"])


def _case_chroma16():
    """RGB16, 128 x 40.  The sample 65 535 in a Co plane that is -65 535 everywhere else, in context 0: behind one event of value 0
    (k = 0) a code of 2^17 bits whose run covers a whole window; behind one of value 1 (k = 1) a code of 65 538 bits with the
    remainder 1 behind its run."""
    at = 128 * 10 + 7
    return Case("chroma16", [chroma16(128, 40, at, 0), chroma16(128, 40, at, 1)],
                ["win:2", "win:3+", "bound:run", "bound:group", "run:w0-w1", "run:covers", "run:rem"])


def _aligned_tile0(w, h, dtype, rgb=False):
    """A flat frame whose tile 0 is made up to whole words with bumps"""
    sites4, sites3 = bump_sites(w, TILE // w - 1), bump_sites(w, TILE // w - 1, last_column=True)
    for a in range(12):
        for b in range(4):
            f = flat(w, h, dtype, rgb)
            for i in sites4[:a] + sites3[:b]:
                bump(f, i)
            if Layout(f).start_bit(0, 1) == 0:
                return f
    raise AssertionError("no bumps align tile 0")


def _shared_frames(dtype):
    """Flat frames whose last tile holds 1 to 31 pixels: five (inside the word tile 0 ends in), eighteen (to the word's last bit), 31
    (into the next word), seven behind a tile 0 of whole words; RGB: five and eighteen, and five behind bumps."""
    near = flat(3, 1367, dtype, True)
    for i in (40, 400, 1000, 2000):
        bump(near, i)
    return [flat(3, 1367, dtype), flat(11, 374, dtype), flat(4127, 1, dtype), _aligned_tile0(11, 373, dtype), flat(3, 1367, dtype, True),
            flat(11, 374, dtype, True), near, _aligned_tile0(11, 373, dtype, True)]


SHARED_EDGES = ("tile:inside-shared-first", "tile:inside-shared-both", "tile:fills-word", "tile:bit0-short", "tile:short-two-words",
                "tile:ends-aligned", "word:three-tiles")


def _case_shared16():
    return Case("shared16", _shared_frames(np.uint16), SHARED_EDGES)


def _case_shared8():
    return Case("shared8", _shared_frames(np.uint8), SHARED_EDGES)


SWEEP_W, SWEEP_H = 52, 79  # 4108 pixels: tile 1 holds twelve


def _sweep(dtype, rgb):
    """Flat frames of one shape with 0, 1, 2 ... bumps in tile 0 (four bits each, three in the last column, more for a context's
    first): one frame for every position 0 .. 31 of the first bit of tile 1 (gray) or of plane 1 (RGB: plane 2 follows it at a
    constant distance)."""
    sites4, sites3 = bump_sites(SWEEP_W, 60), bump_sites(SWEEP_W, 60, last_column=True)
    got = {}
    for a in range(16):
        for b in range(5):
            f = flat(SWEEP_W, SWEEP_H, dtype, rgb)
            for i in sites4[:a] + sites3[:b]:
                bump(f, i)
            L = Layout(f)
            got.setdefault(L.plane_lo[1] & 31 if rgb else L.start_bit(0, 1), f)
            if len(got) == 32:
                return [got[i] for i in range(32)]
    raise AssertionError("positions reached: %s" % sorted(got))


SWEEP_EDGES = ("align:tile1-all32", "tile:inside-shared-first", "tile:fills-word", "tile:bit0-short", "tile:short-two-words", "tile:ends-aligned")
SWEEP_EDGES_RGB = SWEEP_EDGES + ("align:planes-all32", "tile:inside-shared-both", "word:three-tiles")


def _case_sweep16():
    return Case("sweep16", _sweep(np.uint16, False), SWEEP_EDGES)


def _case_sweep16rgb():
    return Case("sweep16rgb", _sweep(np.uint16, True), SWEEP_EDGES_RGB)


def _case_sweep8():
    return Case("sweep8", _sweep(np.uint8, False), SWEEP_EDGES)


def _case_sweep8rgb():
    return Case("sweep8rgb", _sweep(np.uint8, True), SWEEP_EDGES_RGB)


def _case_chroma8():
    return Case("chroma8", [chroma8_longest()[0]], ["u16:group-max"])


_BUILDERS = {"noise16": _case_noise16, "windows16": _case_windows16, "runs16": _case_runs16, "chroma16": _case_chroma16,
             "shared16": _case_shared16, "sweep16": _case_sweep16, "sweep16rgb": _case_sweep16rgb,
             "shared8": _case_shared8, "sweep8": _case_sweep8, "sweep8rgb": _case_sweep8rgb, "chroma8": _case_chroma8}
NAMES = tuple(_BUILDERS)
NAMES16 = tuple(n for n in NAMES if n.endswith("16") or n.endswith("16rgb"))
NAMES8 = tuple(n for n in NAMES if n not in NAMES16)
_CASES = {}


def case(name):
    if name not in _CASES:
        _CASES[name] = _BUILDERS[name]()
    return _CASES[name]


# ------------------------------------------------------------------------------------------------------------------------
# the slot cut
# ------------------------------------------------------------------------------------------------------------------------

def device_slot(cap, n, frame_bytes):
    """The fixed slot felics_compress_batch_device gives each of n streams in a buffer of cap bytes (encode_device): the n-th part
    rounded down to 16 bytes; 0 -- exact placement from the start -- below 64 bytes or a quarter of a frame."""
    slot = cap // n & ~15
    return 0 if slot < 64 or slot < frame_bytes // 4 else slot


def default_slot(frame_bytes):
    """The slot of a stream where the library sizes it itself: the frame and a quarter, 16-byte aligned"""
    return (frame_bytes + frame_bytes // 4 + 64 + 15) & ~15


def cut_reach(L, slot):
    """Where the first bit behind a slot of `slot` bytes falls in the stream with layout L: "cut:run" inside the run of a long code,
    "cut:window<j>" in window j of a tile of several windows, away from the window's first and last word."""
    bit, out = slot * 8, set()
    for p, t in L.all_tiles():
        lo, hi = L.tiles[p][t]
        if lo <= bit < hi:
            if L.windows(p, t) >= 2 and 0 < L.word_in_window(p, t, bit) < WIN_WORDS - 1:
                out.add("cut:window%d" % L.window_of(p, t, bit))
            if any(L.run(p, i)[0] + 32 < bit < L.run(p, i)[1] - 32 for i in L.long_codes(p, t)):
                out.add("cut:run")
    return out


def cut_cases():
    """[(name, frames, capacity, reach)]: batches for felics_compress_batch_device in which the last stream outgrows its fixed slot --
    the last, so that what a cut writes too far lands behind the capacity -- and all streams fit the capacity placed back to back."""
    noise = np.random.default_rng(3).integers(0, 65536, size=(65, 64), dtype=np.uint16)
    return [("run", [flat(QW, QH), flat(QW, QH), quiet16(QW, QH, spikes=[(2000, 0)])], 3 * 3296, {"cut:run", "cut:window0"}),
            ("window0", [flat(64, 65), flat(64, 65), noise], 3 * 5008, {"cut:window0"}),
            ("window1", [flat(64, 65), flat(64, 65), noise], 3 * 8400, {"cut:window1"})]


# ------------------------------------------------------------------------------------------------------------------------
# images of several shapes for one mixed sub-batch
# ------------------------------------------------------------------------------------------------------------------------

def tiles_of(img):
    return -(-(img.shape[0] * img.shape[1]) // TILE)


def one_bucket(imgs):
    """Do the images share a bucket of felics_compress_images (bucket_images: T_min .. ceil(1.25 T_min) tiles)?"""
    t = [tiles_of(im) for im in imgs]
    return max(t) <= (5 * min(t) + 3) // 4


def mixed_sets():
    """{name: 16-bit images of one colour type and several shapes that share a bucket}.  A bucket holds T_min .. ceil(1.25 T_min)
    tiles, so images of one and two tiles share one and images of two and three another, but no bucket holds all three: two sets
    per colour type.  In each, the planes with fewer tiles than the largest image get padding tiles, and one of those is a flat
    frame whose last real tile holds five pixels."""
    noise = np.random.default_rng(3).integers(0, 65536, size=(65, 64), dtype=np.uint16)
    tiny, tiny_rgb = flat(3, 1367), flat(3, 1367, rgb=True)
    return {
        "gray-1-2": [flat(64, 64), quiet16(64, 60, spikes=[(800, 0)]), tiny, quiet16(QW, QH, spikes=[(TILE - 1, 0)]), noise, case("sweep16").frames[7]],
        "gray-2-3": [tiny, quiet16(QW, QH, spikes=[(TILE, 0)]), flat(7, 1171), quiet16(QW, 120, spikes=[(2 * TILE, 0)]), noise,
                     quiet16(66, 68, spikes=[(300, 0)])],
        "rgb-1-2": [flat(64, 64, rgb=True), tiny_rgb, chroma16(128, 40, 128 * 10 + 7, 0), quiet16(QW, QH, spikes=[(QW * QH - 1, 0)], rgb=True)],
        "rgb-2-3": [tiny_rgb, flat(7, 1171, rgb=True), chroma16(128, 40, 128 * 10 + 7, 1), chroma16(128, 70, 128 * 40 + 9, 0)],
    }
