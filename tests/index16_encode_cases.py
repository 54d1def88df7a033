"""What the tests of the 16-bit encoder's restart index share (test_index16_encode_cpu.py, test_index16_encode_gpu.py) beside
index16_common.py: further cases, each a frame plus the edge of the row kernel it is meant to reach, and a model of the ROW RULE
written from the issue's words -- the events of a frame straight from its pixels, the chains, and the rows a rule gives.  That the
cases reach their edges, and that nearly right rules give other bytes, is shown in test_index16_encode_cpu.py."""
import struct

from tests import index16_common as ic

BIG = (0, 65535)           # a chain (context 0) whose every operand is 65 534: a halving every 29 events
FEW = (1000, 1040, 1100)   # contexts 0, 40, 60 and 100, small operands: chains of several hundred events, a halving every few hundred
# (find_seeds below: the first seeds whose 64 x 130 frames reach these edges at segment 4096)
SEED_LANE0, SEED_LANE63, SEED_HALVE_BEFORE, SEED_TWO_HALVINGS = 4, 18, 3, 0


def _straddle():
    """64 x 260: FEW content in rows 0-31 and from row 201 on, flat between.  The flat band's last event stands in row 33 at the latest
    and the next one in row 201 (pixel 12 864): every chain's gap straddles the checkpoints at 4096, 8192 and 12 288."""
    f = ic.chosen(64, 260, FEW, 61)
    f[32:201] = FEW[0]
    return f


def cases():
    """name -> (frame, what it is for).  The seeds are chosen (on the CPU) so that each edge holds; test_index16_encode_cpu.py proves it."""
    return {
        "straddle3": (_straddle(), "(a) one gap straddling three checkpoints: three identical non-empty sets of rows"),
        "few_a": (ic.chosen(64, 130, FEW, SEED_LANE0), "(d) a crossing event whose index in its chain is = 0 mod 64: lane 0 and its carried predecessor"),
        "few_b": (ic.chosen(64, 130, FEW, SEED_LANE63), "(d) a crossing event whose index in its chain is = 63 mod 64: lane 63"),
        "big_a": (ic.chosen(64, 130, BIG, SEED_HALVE_BEFORE), "(e) a halving on the event immediately before a crossing event"),
        "big_b": (ic.chosen(64, 130, BIG, SEED_TWO_HALVINGS), "(e) two halvings in the 64-event block that holds a crossing"),
    }


# ---- the model ------------------------------------------------------------------------------------------------------------------------

def events_of(img):
    """per plane the events in raster order: (pixel, context, operand), from the pixels alone (misc.rs:6-24, compression.rs:200-230)"""
    h, w = img.shape[:2]
    out = []
    for p in ic.planes_of(img):
        p = [int(v) for v in p]
        ev = []
        for i in range(2, len(p)):
            y, x = divmod(i, w)
            if x > 0 and y > 0:
                a, b = p[i - 1], p[i - w]
            elif y == 0:
                a, b = p[i - 1], p[i - 2]
            elif y >= 2:
                a, b = p[i - w], p[i - 2 * w]
            else:
                a, b = p[i - w], p[i - w + 1]
            lo, hi = min(a, b), max(a, b)
            if p[i] > hi:
                ev.append((i, hi - lo, p[i] - hi - 1))
            elif p[i] < lo:
                ev.append((i, hi - lo, lo - p[i] - 1))
        out.append(ev)
    return out


def chains_of(events):
    """context -> its events in raster order, each (pixel, operand, counters before, counters after, halved): the estimator replayed
    along the chain (parameter_selection.rs:49-85: all fifteen counters grow by the code length, and are halved once the smallest
    exceeds 1024)"""
    out = {}
    state = {}
    for i, ctx, e in events:
        row = state.setdefault(ctx, [0] * 15)
        before = row[:]
        for k in range(15):
            row[k] += (e >> k) + 1 + k
        halved = min(row) > 1024
        if halved:
            row[:] = [v >> 1 for v in row]
        out.setdefault(ctx, []).append((i, e, before, row[:], halved))
    return out


def crossings(chain, seg, rule="right"):
    """(index in the chain, checkpoints) of every event b of a chain that gives rows.  rule "right": the checkpoints j with
    pix_a < j seg <= pix_b for the event a before b.  "gt": pix_a < j seg < pix_b.  "first": only the first straddled checkpoint."""
    out = []
    for n in range(1, len(chain)):
        pa, pb = chain[n - 1][0], chain[n][0]
        js = [j for j in range(pa // seg + 1, pb // seg + 1) if rule != "gt" or j * seg < pb]
        if rule == "first":
            js = js[:1]
        if js:
            out.append((n, js))
    return out


def rows_model(img, seg, rule="right"):
    """(n_rows of every (plane, segment) entry, the rows' bytes in the index's order) under a rule: "right", "gt", "first" as in
    crossings, "after": the counters after the event instead of before it, "live": a row for every context with an event in front of
    p0, whether or not another follows."""
    h, w = img.shape[:2]
    k = (h * w + seg - 1) // seg
    counts, blob = [], bytearray()
    for ev in events_of(img):
        per = [dict() for _ in range(k)]
        for ctx, chain in chains_of(ev).items():
            if rule == "live":
                for j in range(1, k):
                    done = [c for c in chain if c[0] < j * seg]
                    if done:
                        per[j][ctx] = done[-1][3]
                continue
            for n, js in crossings(chain, seg, "right" if rule == "after" else rule):
                for j in js:
                    per[j][ctx] = chain[n][3 if rule == "after" else 2]
        for j in range(k):
            counts.append(len(per[j]))
            for ctx in sorted(per[j]):
                blob += struct.pack("<15I", *per[j][ctx]) + struct.pack("<I", ctx)
    return counts, bytes(blob)


def rows_of_index(index):
    """the same two from a built index"""
    lay = ic.Layout16(index)
    return lay.n_rows(), index[lay.rows_base:]


def find_seeds(limit=400):
    """the search the SEED_* values came from: for each edge the first seed whose frame reaches it at segment 4096"""
    want = {}
    for seed in range(limit):
        for values, keys in ((FEW, ("lane0", "lane63")), (BIG, ("halve_before", "two_halvings"))):
            got = edges(ic.chosen(64, 130, values, seed), 4096)
            for key in keys:
                if got[key] and key not in want:
                    want[key] = seed
        if len(want) == 4:
            break
    return want


def edges(img, seg):
    """which of the row kernel's edges a frame reaches at a segment size: name -> a witness (context, index in the chain), or None"""
    out = dict.fromkeys(("lane0", "lane63", "halve_before", "two_halvings", "straddle3", "at_p0", "ends_before_p0", "chains_over_300"))
    npix = img.shape[0] * img.shape[1]
    for ev in events_of(img):
        for ctx, chain in chains_of(ev).items():
            if len(chain) >= 300:
                out["chains_over_300"] = (ctx, len(chain))
            last = chain[-1][0]
            for p0 in range(seg, npix, seg):
                if last == p0 - 1 and len(chain) > 1:
                    out["ends_before_p0"] = (ctx, p0)
            for n, js in crossings(chain, seg):
                if n >= 64 and n % 64 == 0:
                    out["lane0"] = (ctx, n)
                if n % 64 == 63:
                    out["lane63"] = (ctx, n)
                if chain[n - 1][4]:
                    out["halve_before"] = (ctx, n)
                block = chain[n // 64 * 64:n // 64 * 64 + 64]
                if sum(1 for c in block if c[4]) >= 2:
                    out["two_halvings"] = (ctx, n)
                if len(js) >= 3:
                    out["straddle3"] = (ctx, n)
                if any(chain[n][0] == j * seg for j in js):
                    out["at_p0"] = (ctx, n)
    return out

