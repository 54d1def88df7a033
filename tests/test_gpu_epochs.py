"""Long-lived contexts: the three pieces of state a context keeps valid between calls by an epoch tag instead of a clear
(felics_amd/csrc/felics_epochs.h) taken across their wraps on the GPU, and the API families mixed on one context.

  look-back status words of k_pack_t   tag: 18 bits of a lane's epoch, one per sub-batch   FELICS_TEST_LOOKBACK_EPOCH
  dense tables of k_decode16           tag: 32 bits, three per pass                        FELICS_TEST_DECODE16_EPOCH
  hashed tables of k_decode16_lanes    tag: 15 bits, three per launch                      FELICS_TEST_DECODE16_LANES_EPOCH

The switches are read when a context is created and name the LAST epoch the counter pretends to have handed out on a fresh buffer,
so a few calls reach a wrap that is otherwise days (or 10 923 launches) away.  The rules themselves are walked exhaustively on the
host (tests/test_epochs.py); what only the GPU can show is that the clear is ordered ahead of the launch that reuses the first tags
and behind everything that still reads the old ones.  Every stream is compared byte for byte with the oracle's, every decoded frame
sample for sample with its source (whose stream the oracle's own decoder has taken back to it); there are no tolerances."""
import collections
import contextlib
import os
import re
import time

import numpy as np
import pytest

from tests import index_common as ic
from tests import region_common as rcm

pytestmark = pytest.mark.gpu

LOOKBACK_MASK = 0x3FFFF          # LOOKBACK_EPOCH_MASK
DEC16_EPOCH_LAST = 0xFFFFFFF0    # the wave form clears once its counter has passed this
DEC16L_EPOCH_MAX = 0x7FFF
SORT_TILE = 4096


@contextlib.contextmanager
def _env(**kv):
    """environment variables for the calls inside; None unsets"""
    old = {k: os.environ.get(k) for k in kv}
    try:
        for k, v in kv.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = str(v)
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


@contextlib.contextmanager
def _encoder(**kv):
    """a fresh context created under these variables (the library reads them in felics_ctx_create)"""
    import felics_amd

    with _env(**kv):
        e = felics_amd.Encoder(0)
    try:
        yield e
    finally:
        e.close()


def _rows(npix):
    """felics_lanetable.h, dec16l_rows: rows of one plane's table"""
    need = 2 * min(max(npix - 2, 0), 131071)
    if need > 65536:
        return 131071
    rows = 64
    while rows < need:
        rows *= 2
    return rows


def _traced(capfd, what):
    """The epochs the library says it handed out since the last look (FELICS_TRACE_EPOCHS=1: a line on stderr for each, felics_epochs.h's
    answer as the caller used it): [(lane, epoch, clear)] for "look-back", [(epoch0, clear)] for "decode16" and "decode16 lanes"."""
    out = []
    for line in capfd.readouterr().err.splitlines():
        m = re.fullmatch(r"\[felics\] %s(?: lane (\d+))? epoch 0x([0-9a-f]+) clear ([01])" % re.escape(what), line)
        if m:
            out.append(((int(m.group(1)),) if m.group(1) else ()) + (int(m.group(2), 16), m.group(3) == "1"))
    return out


class Source:
    """frames with the oracle's stream of each, made once per module"""

    def __init__(self, oracle):
        self.oracle = oracle
        self.cache = {}

    def stream(self, img):
        key = (img.shape, img.dtype.str, img.tobytes())
        if key not in self.cache:
            s = self.oracle.compress(img)
            assert (self.oracle.decompress(s) == img).all()
            self.cache[key] = s
        return self.cache[key]


@pytest.fixture(scope="module")
def src(oracle):
    return Source(oracle)


def _same(got, want, what):
    assert len(got) == len(want), what
    for i, (g, w) in enumerate(zip(got, want)):
        if g != w:
            raise AssertionError("%s, stream %d: differs from the oracle at byte %s (sizes %d vs %d)" % (what, i, ic.first_difference(g, w), len(g), len(w)))


# ---- look-back tags ---------------------------------------------------------------------------------------------------------------

def _frames8(w, h, rgb, count, turn):
    """`count` frames of w x h whose content goes round flat -> noise -> synth S1 with `turn`, so no two calls in a row code alike"""
    from felics_amd import synth

    rng = np.random.default_rng(1000 * turn + w + rgb)
    out = []
    for i in range(count):
        kind = (turn + i) % 3
        if kind == 0:
            out.append(np.full((h, w, 3) if rgb else (h, w), 40 + 7 * ((turn + i) % 23), np.uint8))
        elif kind == 1:
            out.append(rng.integers(0, 256, size=(h, w, 3) if rgb else (h, w), dtype=np.uint8))
        else:
            out.append(synth.rgb8(w, h, turn + i) if rgb else synth.gray8(w, h, turn + i, "S1"))
    return out


def _mixed_jobs(imgs):
    """felics_mixed.cpp, bucket_images, for 8-bit images: per colour, sorted by sort tiles T, a sub-batch holds T_min .. ceil(1.25 T_min)"""
    jobs = 0
    for rgb in (False, True):
        tiles = sorted(-(-im.shape[0] * im.shape[1] // SORT_TILE) for im in imgs if (im.ndim == 3) == rgb)
        a = 0
        while a < len(tiles):
            lim = (5 * tiles[a] + 3) // 4  # ceil(1.25 T_min)
            while a < len(tiles) and tiles[a] <= lim:
                a += 1
            jobs += 1
    return jobs


class Lanes:
    """What run_lane does with the lanes' epochs (felics_encode.cpp, felics_epochs.h): every 8-bit sub-batch takes the next lane in
    turn (next_lane), that lane's epoch goes up by one, and the status words are cleared in front of it when the 18 tag bits are 0."""

    def __init__(self, nlanes, last):
        self.epoch = [last] * nlanes
        self.clears = [0] * nlanes
        self.next = 0
        self.subs = 0

    def take(self, count):
        out = []
        for _ in range(count):
            lane = self.next
            self.epoch[lane] = (self.epoch[lane] + 1) & 0xFFFFFFFF
            clear = (self.epoch[lane] & LOOKBACK_MASK) == 0
            self.clears[lane] += clear
            self.next = (lane + 1) % len(self.epoch)
            self.subs += 1
            out.append((lane, self.epoch[lane], clear))
        return out


def _submit(enc, frames):
    """felics_submit_batch_device on frames of one shape: the ticket and the buffers it needs until it lands"""
    import torch

    n = len(frames)
    h, w = frames[0].shape[:2]
    slot = (frames[0].nbytes * 5 // 4 + 64 + 15) // 16 * 16
    d_in = torch.from_numpy(np.stack(frames)).cuda()
    d_out = torch.zeros(slot * n, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ticket = enc.submit_batch_device(d_in.data_ptr(), n, w, h, int(frames[0].ndim == 3), 0, d_out.data_ptr(), slot * n)
    return ticket, d_in, d_out


def _land(enc, flying):
    ticket, _, d_out = flying
    offs, lens = enc.wait_batch(ticket)
    host = d_out.cpu().numpy()
    return [host[int(o):int(o) + int(ln)].tobytes() for o, ln in zip(offs, lens)]


@pytest.mark.parametrize("own_tails", [False, True], ids=["shared-tail", "own-tails"])
@pytest.mark.parametrize("nlanes", [2, 4])
@pytest.mark.parametrize("wrap", [0x3FFFF, 0xFFFFFFFF], ids=["18-bit-wrap", "32-bit-wrap"])
def test_lookback_tags_across_the_wraps(src, capfd, wrap, nlanes, own_tails):
    """A context whose lanes start three epochs below a wrap of the look-back tags -- the first clear at 0x40000, and the counter
    running over to 0, which clears as well -- driven until every lane has crossed it.

    Epochs per call, from the code: run_lane takes ONE epoch of ONE lane per 8-bit sub-batch, and the lanes are handed out in turn
    (next_lane).  felics_compress is one sub-batch; felics_compress_batch of n frames is ceil(n / ceil(n / 8)) chunks, a sub-batch
    each; felics_submit_batch_device is one; felics_compress_images is one per bucket of its images (_mixed_jobs).  So after S
    sub-batches lane L has taken floor((S - L + lanes - 1) / lanes) epochs; the model (Lanes) is held against lane_count() and, call
    by call, against stats()["submissions"] and against the lane, epoch and clear the library reports for every sub-batch
    (FELICS_TRACE_EPOCHS), which also shows that the start value took effect.  The calls come in rounds of one sub-batch per lane: 1024 x 256 frames (64 tiles a plane:
    the status buffer gets its size), single frames of 333 x 77 (seven tiles a plane), tickets kept two in flight through the round
    below the wrap and the round that clears, 1024 x 256 frames again directly behind the clear, one mixed-shape call, and a batch
    of nine RGB frames.  Content goes round flat, noise and synth S1 from call to call."""
    last = wrap - 3
    with _encoder(FELICS_LANES=nlanes, FELICS_OWN_TAILS="1" if own_tails else None, FELICS_TEST_LOOKBACK_EPOCH=hex(last),
                  FELICS_TRACE_EPOCHS="1") as enc:
        assert enc.lane_count() == nlanes
        model = Lanes(nlanes, last)
        turn = [0]

        def frames(w, h, rgb, count):
            turn[0] += 1
            return _frames8(w, h, rgb, count, turn[0])

        def counted(subs):
            taken = model.take(subs)
            assert enc.stats()["submissions"] == model.subs, (enc.stats(), model.subs)
            assert _traced(capfd, "look-back") == taken
            return taken

        # round 1: every lane's status buffer sized for 64 tiles a plane, tags wrap - 2
        big = frames(1024, 256, False, nlanes)
        _same(enc.compress_batch(big), [src.stream(f) for f in big], "1024 x 256 below the wrap")
        assert [e for _, e, _ in counted(nlanes)] == [(wrap - 2) & 0xFFFFFFFF] * nlanes
        # round 2: single frames, gray and RGB in turn, tags wrap - 1
        for i in range(nlanes):
            f = frames(333, 77, bool(i % 2), 1)[0]
            _same([enc.compress(f)], [src.stream(f)], "single frame %d" % i)
            counted(1)
        # rounds 3 and 4: tickets, two in flight all the way through tags `wrap` and wrap + 1 (the clear)
        flying = collections.deque()
        cleared = 0
        for i in range(2 * nlanes):
            if len(flying) == 2:
                fr, fl = flying.popleft()
                _same(_land(enc, fl), [src.stream(f) for f in fr], "ticket")
            fr = frames(333, 77, bool(i % 3 == 1), 3)
            flying.append((fr, _submit(enc, fr)))
            cleared += counted(1)[0][2]
        while flying:
            fr, fl = flying.popleft()
            _same(_land(enc, fl), [src.stream(f) for f in fr], "ticket")
        assert cleared == nlanes and model.clears == [1] * nlanes  # every lane has crossed, in the round of the tickets
        # round 5: 64 tiles a plane directly behind the clear (look-backs over words the clear has just zeroed)
        big = frames(1024, 256, False, nlanes)
        _same(enc.compress_batch(big), [src.stream(f) for f in big], "1024 x 256 behind the clear")
        assert all(((e - 1) & LOOKBACK_MASK) == 0 for _, e, _ in counted(nlanes))
        # one mixed-shape call: four buckets (gray 1-2 tiles, gray 7, RGB 1, RGB 7)
        mixed = [frames(333, 77, False, 1)[0], frames(100, 50, False, 1)[0], frames(64, 64, False, 1)[0], frames(333, 77, True, 1)[0],
                 frames(40, 30, True, 1)[0]]
        assert _mixed_jobs(mixed) == 4
        _same(enc.compress_images(mixed), [src.stream(f) for f in mixed], "mixed-shape call")
        counted(4)
        # a batch of nine RGB frames: chunks of two, five sub-batches
        nine = frames(333, 77, True, 9)
        _same(enc.compress_batch(nine), [src.stream(f) for f in nine], "nine RGB frames")
        counted(5)
        st = enc.stats()
        assert model.clears == [1] * nlanes and all(((e - wrap) & 0xFFFFFFFF) >= 3 for e in model.epoch)
        assert (st["lookback_fallbacks"], st["scatter_fallbacks"], st["tile_overflows"], st["slot_overflows"]) == (0, 0, 0, 0), st
        assert st["two_pass"] == 0 and st["failed"] == 0 and st["ticket_retries"] == 0, st


# ---- the 16-bit decoders ----------------------------------------------------------------------------------------------------------

def _blob(streams):
    offs, blob = [], bytearray()
    for s in streams:
        offs.append(len(blob))
        blob += s + bytes((-len(s)) % 16)
    return offs, np.frombuffer(bytes(blob) + bytes(16), dtype=np.uint8).copy()


def _decode_same(enc, src, imgs):
    """felics_decompress_batch_device on the oracle's streams of same-shaped images: every frame against its source.  Returns the
    call's decode_stats delta."""
    import torch

    streams = [src.stream(im) for im in imgs]
    offs, blob = _blob(streams)
    d_in = torch.from_numpy(blob).cuda()
    per = imgs[0].nbytes
    d_px = torch.full((max(per * len(imgs), 16) + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    before = enc.decode_stats()
    _, status = enc.decompress_batch_device(d_in.data_ptr(), offs, [len(s) for s in streams], d_px.data_ptr(), per * len(imgs))
    after = enc.decode_stats()
    host = d_px.cpu().numpy()
    assert (status == 0).all(), status
    assert (host[per * len(imgs):] == 0xA5).all()
    for i, im in enumerate(imgs):
        assert (host[i * per:(i + 1) * per].view(im.dtype).reshape(im.shape) == im).all(), (i, im.shape, im.dtype)
    d = {k: after[k] - before[k] for k in after}
    d["lanes16_table_bytes"] = after["lanes16_table_bytes"]
    return d


def _decode_mixed(enc, src, imgs):
    """felics_decompress_images_device on the oracle's streams of any images: every frame against its source; the delta of decode_stats"""
    import torch

    streams = [src.stream(im) for im in imgs]
    offs, blob = _blob(streams)
    d_in = torch.from_numpy(blob).cuda()
    cap = sum((im.nbytes + 15) // 16 * 16 for im in imgs)
    d_px = torch.full((cap + 64,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    before = enc.decode_stats()
    po, _, status = enc.decompress_images_device(d_in.data_ptr(), offs, [len(s) for s in streams], d_px.data_ptr(), cap)
    after = enc.decode_stats()
    host = d_px.cpu().numpy()
    assert (status == 0).all(), status
    assert (host[cap:] == 0xA5).all()
    for i, im in enumerate(imgs):
        assert (host[int(po[i]):int(po[i]) + im.nbytes].view(im.dtype).reshape(im.shape) == im).all(), (i, im.shape, im.dtype)
    d = {k: after[k] - before[k] for k in after}
    d["lanes16_table_bytes"] = after["lanes16_table_bytes"]
    return d


def _content16(h, w, rgb, count, rng):
    """`count` frames: synth.gray16 crops and full-range noise, alternating"""
    from felics_amd import synth

    base = synth.gray16(max(w + 40, 128), max(h + 40, 128), int(rng.integers(0, 1000)))
    out = []
    for i in range(count):
        if i % 2:
            out.append(rng.integers(0, 65536, size=(h, w, 3) if rgb else (h, w), dtype=np.uint16))
        else:
            g = base[i % 37:i % 37 + h, (3 * i) % 31:(3 * i) % 31 + w]
            out.append(np.stack([g, np.roll(g, 3, axis=1), 65535 - g], -1).copy() if rgb else g.copy())
    return out


def test_decode16_wave_form_across_its_wrap(src, capfd):
    """k_decode16's dense tables, the counter started one pass below 0xFFFFFFF0.  Same-shape calls of three streams (one pass, three
    epochs each): the first takes 0xFFFFFFEE .. F0, the second F1 .. F3, the third finds the counter past 0xFFFFFFF0, clears and takes
    1 .. 3.  Then a mixed call with four 16-bit rows in the wave form: its pass wants a larger table, the buffer grows and the counter
    goes back to the start value, so the calls behind it cross the wrap a second time on the new buffer.  The epochs the library
    reports (FELICS_TRACE_EPOCHS) must be exactly these."""
    rng = np.random.default_rng(71)
    last = DEC16_EPOCH_LAST - 3
    with _encoder(FELICS_TEST_DECODE16_EPOCH=hex(last), FELICS_TRACE_EPOCHS="1") as enc, _env(FELICS_TEST_DECODE16_LANES="0"):
        for turn in range(2):
            for rgb in (False, True, False, True):
                d = _decode_same(enc, src, _content16(40, 56, rgb, 3, rng))
                assert (d["wave16"], d["lanes16"], d["host"], d["undecoded"]) == (3, 0, 0, 0), d
            if turn == 0:
                imgs = _content16(40, 56, False, 2, rng) + _content16(40, 56, True, 1, rng) + _content16(21, 30, False, 1, rng)
                imgs.append(rng.integers(0, 256, size=(30, 50), dtype=np.uint8))
                d = _decode_mixed(enc, src, imgs)
                assert (d["wave16"], d["lanes16"], d["host"], d["undecoded"]) == (4, 0, 0, 0), d
    assert _traced(capfd, "decode16") == [(last + 1, False), (last + 4, False), (1, True), (4, False), (last + 1, False),
                                          (last + 4, False), (1, True), (4, False), (7, False)]


def test_decode16_lane_form_across_its_wrap(src, capfd):
    """k_decode16_lanes' hashed tables, the counter started two launches below DEC16L_EPOCH_MAX (FELICS_TEST_DECODE16_LANES=1 puts
    every 16-bit stream with W >= 8 in the lane form).  Shapes on both sides of a table-size switch, (4, 17) with 256 rows a plane and
    (8, 8) with 128, the larger first so that the buffer keeps its size (a same-shape call sizes it for a whole wave: 64 x 3 x 256
    rows): launches one and two take 0x7FF9 .. 0x7FFE, the third clears and takes 1 .. 3.  The mixed call, two waves of rgb16 and
    one of gray16, wants 65 536 rows: the buffer grows, the counter goes back to the start value, and its two passes and the
    same-shape calls behind it cross the wrap again on the new buffer.  The epochs the library reports (FELICS_TRACE_EPOCHS) must be
    exactly these."""
    rng = np.random.default_rng(72)
    last = DEC16L_EPOCH_MAX - 1 - 6
    with _encoder(FELICS_TEST_DECODE16_LANES_EPOCH=last, FELICS_TRACE_EPOCHS="1") as enc, _env(FELICS_TEST_DECODE16_LANES="1"):
        for turn in range(2):
            for (h, w), rgb in (((4, 17), True), ((4, 17), False), ((8, 8), True), ((8, 8), False)):
                d = _decode_same(enc, src, _content16(h, w, rgb, 5, rng))
                assert (d["lanes16"], d["wave16"], d["host"], d["undecoded"]) == (5, 0, 0, 0), d
                assert d["lanes16_table_bytes"] == 5 * (3 if rgb else 1) * _rows(h * w) * 64
            if turn == 0:
                imgs = _content16(8, 8, True, 128, rng) + _content16(4, 17, False, 64, rng) + _content16(8, 8, False, 3, rng)
                d = _decode_mixed(enc, src, [imgs[i] for i in rng.permutation(len(imgs))])
                assert (d["lanes16"], d["wave16"], d["host"], d["undecoded"]) == (192, 3, 0, 0), d
                assert d["lanes16_table_bytes"] == max(128 * 3 * _rows(64), 64 * _rows(68)) * 64
    assert _traced(capfd, "decode16 lanes") == [(last + 1, False), (last + 4, False), (1, True), (4, False), (last + 1, False),
                                                (last + 4, False), (1, True), (4, False), (7, False), (10, False)]


CYCLE_EDGE_STEP, CYCLE_MIDDLE, CYCLE_EDGE, CYCLE_APART = 3001, 300, 72, 8  # lanewalk_check.cpp


def _cycle_frame(edge, index):
    """lanewalk_check.cpp's cycle_frame: an 8 x 8 gray16 frame of sixteen values, 4096 apart (middle) or CYCLE_EDGE_STEP apart (edge)"""
    state = ((index + 1) * 2654435761) & 0xFFFFFFFF
    if edge:
        state ^= 0x5BD1E995
    px = np.zeros(64, np.uint16)
    for p in range(64):
        state = (state * 1664525 + 1013904223) & 0xFFFFFFFF
        px[p] = ((state >> 8) & 15) * (CYCLE_EDGE_STEP if edge else 4096)
    return px.reshape(8, 8)


def test_decode16_lane_form_whole_cycle(src, capfd):
    """The one cycle short enough to run: 10 924 launches of k_decode16_lanes on one table buffer, with no start value -- one call of
    10 924 x 64 streams of 8 x 8 gray16 in passes of 64 (FELICS_TEST_DECODE16_LANES_PASS=64).  Launch 10 923 finds the epochs used up,
    clears and takes epochs 1 .. 3 again (the library's own report, FELICS_TRACE_EPOCHS, must say so: one clear, in front of that
    launch).  What a missing or late clear would leave it: a row of another epoch is an empty row and is reclaimed by whoever probes
    it, so launch 1's rows live on only where launches 2 .. 10 922 never probe.  Hence two kinds of frames, all of sixteen widely
    spaced values (every pixel out of range, few contexts, large errors): launches 1 and 10 923 decode "edge" frames, values 3001
    apart, slot j frame j and frame j + 8; every other launch "middle" frames, 4096 apart, stream i frame i % 300, whose sixteen
    contexts leave most of the edge contexts' rows alone.  lanewalk_check's "whole cycle" case runs this very schedule on the host on
    a table that is never cleared: all 64 slots of launch 10 923 then decode wrongly (nine or ten rows of launch 1 left in each), and
    with middle frames alone none would.  Measured on an MI355X: 1.06 s for the call, 1.6 s for the test."""
    import torch

    launches = 10924
    n = launches * 64
    imgs = [_cycle_frame(False, i) for i in range(CYCLE_MIDDLE)] + [_cycle_frame(True, i) for i in range(CYCLE_EDGE)]
    distinct = len(imgs)
    streams = [src.stream(im) for im in imgs]
    stride = (max(len(s) for s in streams) + 15) // 16 * 16
    table = np.zeros((distinct, stride), np.uint8)
    for i, s in enumerate(streams):
        table[i, :len(s)] = np.frombuffer(s, np.uint8)
    which = np.arange(n) % CYCLE_MIDDLE
    which[:64] = CYCLE_MIDDLE + np.arange(64)
    which[10922 * 64:10923 * 64] = CYCLE_MIDDLE + CYCLE_APART + np.arange(64)
    d_in = torch.from_numpy(table).cuda()[torch.from_numpy(which).cuda()].contiguous()  # stream i at i * stride
    offs = np.arange(n, dtype=np.uint64) * stride
    lens = np.array([len(s) for s in streams], np.uint64)[which]
    d_px = torch.zeros(n * 128, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    with _encoder(FELICS_TRACE_EPOCHS="1") as enc, _env(FELICS_TEST_DECODE16_LANES="1", FELICS_TEST_DECODE16_LANES_PASS="64"):
        t0 = time.perf_counter()
        _, status = enc.decompress_batch_device(d_in.data_ptr(), offs, lens, d_px.data_ptr(), n * 128)
        seconds = time.perf_counter() - t0
        st = enc.decode_stats()
    traced = _traced(capfd, "decode16 lanes")
    print("whole cycle: %d launches of 64 streams in %.2f s" % (launches, seconds))
    assert traced == [(1 + 3 * (k % 10922), k == 10922) for k in range(launches)]
    assert (status == 0).all(), np.flatnonzero(status)[:8]
    assert (st["lanes16"], st["wave16"], st["host"], st["undecoded"], st["streams"]) == (n, 0, 0, 0, n), st
    assert st["lanes16_table_bytes"] == 64 * _rows(64) * 64  # one pass's tables: the buffer of the first pass served them all
    want = torch.from_numpy(np.stack(imgs).view(np.uint8).reshape(distinct, 128)).cuda()[torch.from_numpy(which).cuda()]
    wrong = torch.nonzero((d_px.view(n, 128) != want).any(1)).flatten()
    assert wrong.numel() == 0, ("streams decoded wrongly, the first in launch %d" % (int(wrong[0]) // 64 + 1), wrong[:8].tolist())


# ---- interleaved traffic ----------------------------------------------------------------------------------------------------------

def _image(rng, h, w, rgb, wide):
    """one frame: flat, noise or a synth crop"""
    from felics_amd import synth

    kind = int(rng.integers(0, 3))
    shape = (h, w, 3) if rgb else (h, w)
    dt, top = (np.uint16, 65536) if wide else (np.uint8, 256)
    if kind == 0:
        return np.full(shape, int(rng.integers(0, top)), dt)
    if kind == 1:
        return rng.integers(0, top, size=shape, dtype=dt)
    f = int(rng.integers(0, 50))
    if wide:
        g = synth.gray16(w, h, f)
        return np.stack([g, np.roll(g, 2, axis=1), 65535 - g], -1).copy() if rgb else g
    return synth.rgb8(w, h, f) if rgb else synth.gray8(w, h, f, "S1")


def _shape(rng, step):
    """(h, w) between 1 x 8 and 700 x 300 (W x H), the extremes at fixed steps, sizes going up and down"""
    fixed = {3: (8, 1), 7: (300, 700), 11: (1, 8), 20: (300, 700), 21: (5, 9), 33: (299, 697)}
    if step in fixed:
        return fixed[step]
    if step % 2:
        return int(rng.integers(1, 40)), int(rng.integers(8, 60))
    return int(rng.integers(40, 301)), int(rng.integers(60, 701))


def _index_blob(indexes):
    stride = max((max(len(i) for i in indexes) + 15) // 16 * 16, 64)
    return stride, np.frombuffer(b"".join(i + bytes(stride - len(i)) for i in indexes), dtype=np.uint8).copy()


def test_interleaved_traffic_on_one_context(src):
    """48 calls on one context from a fixed seed, drawn from every family -- compress, compress_batch, compress_images,
    compress_batch_device_indexed, compress_arrays_device, decompress_batch_device (8- and 16-bit, wave and lane forms by the test
    switches), decompress_images_device, decompress_arrays_device, decompress_batch_device_indexed and
    decompress_regions_device_indexed -- with shapes between 1 x 8 and 700 x 300 going up and down, so the grow-only buffers are
    reallocated while the lanes' and the tables' epochs run on.  The first ten calls are one of each family.  The decode calls take the
    lane switches in turn (forced, forbidden, unset), and every mixed decode holds a whole wave of small gray8 and of small gray16
    streams, so decode_stats must end with streams in all four of wave8, lanes8, wave16 and lanes16."""
    import torch

    from felics_amd import api

    rng = np.random.default_rng(2026)
    families = ["compress", "compress_batch", "compress_images", "encode_indexed", "compress_arrays", "decode_same", "decode_images",
                "decode_arrays", "decode_indexed", "decode_regions"]
    order = [families[i] for i in rng.permutation(len(families))] + [families[int(i)] for i in rng.integers(0, len(families), 38)]
    seen = collections.Counter()
    forms = collections.Counter()
    switches = [("1", "1"), ("0", "0"), (None, None), ("1", "0"), ("0", "1")]  # FELICS_TEST_DECODE_LANES, FELICS_TEST_DECODE16_LANES
    decodes = 0
    with _encoder() as enc:
        for step, family in enumerate(order):
            h, w = _shape(rng, step)
            rgb, wide = bool(rng.integers(0, 2)), bool(rng.integers(0, 2))
            what = "call %d (%s, %d x %d)" % (step, family, w, h)
            seen[family] += 1
            if family == "compress":
                im = _image(rng, h, w, rgb, wide)
                _same([enc.compress(im)], [src.stream(im)], what)
            elif family == "compress_batch":
                ims = [_image(rng, h, w, rgb, wide) for _ in range(int(rng.integers(2, 11)))]
                _same(enc.compress_batch(ims), [src.stream(im) for im in ims], what)
            elif family == "compress_images":
                ims = [_image(rng, *_shape(rng, step + k), bool(rng.integers(0, 2)), bool(rng.integers(0, 2))) for k in range(int(rng.integers(3, 7)))]
                _same(enc.compress_images(ims), [src.stream(im) for im in ims], what)
            elif family == "encode_indexed":
                ims = [_image(rng, h, w, rgb, False) for _ in range(int(rng.integers(1, 5)))]
                streams, indexes = ic.encode_indexed(enc, ims, 4096)
                _same(streams, [src.stream(im) for im in ims], what)
                _same(indexes, [api.index_build(s, 4096) for s in streams], what + ", index")
            elif family == "compress_arrays":
                mosaic = _image(rng, h + 9, w + 14, False, False)  # (8-bit: the tensors of the array interface)
                rgba = np.concatenate([_image(rng, h, w, True, False), _image(rng, h, w, False, False)[..., None]], -1)
                t_mosaic, t_rgba = torch.from_numpy(mosaic).cuda(), torch.from_numpy(rgba).cuda()
                arrays = [t_mosaic[4:4 + h, 5:5 + w], t_rgba[..., :3], t_mosaic]
                dense = [np.ascontiguousarray(a) for a in (mosaic[4:4 + h, 5:5 + w], rgba[..., :3], mosaic)]
                cap = sum((d.nbytes * 5 // 4 + 64 + 15) // 16 * 16 + 64 for d in dense) * 2
                out = torch.zeros(cap, dtype=torch.uint8, device="cuda")
                torch.cuda.synchronize()
                offs, lens = enc.compress_arrays_device(arrays, out.data_ptr(), cap)
                host = out.cpu().numpy()
                _same([host[int(o):int(o) + int(ln)].tobytes() for o, ln in zip(offs, lens)], [src.stream(d) for d in dense], what)
            elif family == "decode_same":
                n = int(rng.integers(1, 9)) if h * w > 4000 else 67
                ims = [_image(rng, h, w, rgb, wide) for _ in range(min(n, 6))]
                with _env(FELICS_TEST_DECODE_LANES=switches[decodes % 5][0], FELICS_TEST_DECODE16_LANES=switches[decodes % 5][1]):
                    d = _decode_same(enc, src, [ims[i % len(ims)] for i in range(n)])
                decodes += 1
                forms.update({k: d[k] for k in ("wave8", "lanes8", "wave16", "lanes16")})
                assert d["streams"] == n and d["undecoded"] == 0, (what, d)
            elif family == "decode_images":
                ims = [_image(rng, *_shape(rng, step + k), bool(rng.integers(0, 2)), bool(rng.integers(0, 2))) for k in range(int(rng.integers(3, 7)))]
                for wide_wave in (False, True):  # a whole wave of one shape at either depth, for the lane forms
                    small = [_image(rng, 6, 11, False, wide_wave) for _ in range(3)]
                    ims += [small[i % 3] for i in range(64)]
                with _env(FELICS_TEST_DECODE_LANES=switches[decodes % 5][0], FELICS_TEST_DECODE16_LANES=switches[decodes % 5][1]):
                    d = _decode_mixed(enc, src, [ims[i] for i in rng.permutation(len(ims))])
                decodes += 1
                forms.update({k: d[k] for k in ("wave8", "lanes8", "wave16", "lanes16")})
                assert d["streams"] == len(ims) and d["undecoded"] == 0, (what, d)
            elif family == "decode_arrays":
                ims = [_image(rng, h, w, True, False), _image(rng, h, w, False, False), _image(rng, min(h, 9), min(w, 14), False, False)]
                dt = torch.uint8  # (8-bit: the tensors of the array interface)
                chw = torch.zeros((3, h, w), dtype=dt, device="cuda")
                mosaic = torch.zeros((h + 9, w + 14), dtype=dt, device="cuda")
                cell = torch.zeros(ims[2].shape, dtype=dt, device="cuda")
                streams = [src.stream(im) for im in ims]
                offs, blob = _blob(streams)
                d_in = torch.from_numpy(blob).cuda()
                torch.cuda.synchronize()
                _, status = enc.decompress_arrays_device(d_in.data_ptr(), offs, [len(s) for s in streams],
                                                         [chw.permute(1, 2, 0), mosaic[4:4 + h, 5:5 + w], cell])
                assert (status == 0).all(), (what, status)
                host = mosaic.cpu().numpy()
                assert (chw.cpu().numpy().transpose(1, 2, 0) == ims[0]).all(), what
                assert (host[4:4 + h, 5:5 + w] == ims[1]).all() and host.sum(dtype=np.uint64) == ims[1].sum(dtype=np.uint64), what
                assert (cell.cpu().numpy() == ims[2]).all(), what
            else:
                n = int(rng.integers(1, 5)) if h * w > 4000 else 66
                ims = [_image(rng, h, w, rgb, False) for _ in range(min(n, 4))]
                ims = [ims[i % len(ims)] for i in range(n)]
                streams = [src.stream(im) for im in ims]
                indexes = [api.index_build(s, 4096) for s in streams]
                if family == "decode_indexed":
                    with _env(FELICS_TEST_INDEX_LANES=[None, "0", "1"][int(rng.integers(0, 3))]):
                        status, frames = ic.decode_indexed(enc, streams, indexes, ims[0].nbytes, guard=64)
                    assert (np.asarray(status) == 0).all(), (what, status)
                    for i, im in enumerate(ims):
                        assert (frames[i].reshape(im.shape) == im).all(), (what, i)
                else:
                    regions = [(int(rng.integers(0, n)),) + r for r in rcm.random_regions(w, h, 5, step)]
                    blob, offs, lens = ic.pack_streams(streams)
                    stride, iblob = _index_blob(indexes)
                    d_in = torch.from_numpy(np.frombuffer(blob, dtype=np.uint8).copy()).cuda()
                    d_idx = torch.from_numpy(iblob).cuda()
                    planes = 3 if rgb else 1
                    total = sum(r[3] * r[4] * planes for r in regions)
                    d_px = torch.full((total + 64,), 0xA5, dtype=torch.uint8, device="cuda")
                    torch.cuda.synchronize()
                    _, status, out_offs = enc.decompress_regions_device_indexed(d_in.data_ptr(), offs, lens, d_idx.data_ptr(), stride, regions,
                                                                                d_px.data_ptr(), total)
                    assert (np.asarray(status) == 0).all(), (what, status)
                    host = d_px.cpu().numpy()
                    assert (host[total:] == 0xA5).all(), what
                    for r, o in zip(regions, out_offs):
                        want = rcm.crop(ims[r[0]], r[1:])
                        assert (host[int(o):int(o) + want.size].reshape(want.shape) == want).all(), (what, r)
        st = enc.stats()
        assert (st["lookback_fallbacks"], st["scatter_fallbacks"], st["tile_overflows"], st["failed"]) == (0, 0, 0, 0), st
    assert len(order) == 48 and all(seen[f] >= 1 for f in families), seen
    assert decodes >= 5 and all(forms[k] > 0 for k in ("wave8", "lanes8", "wave16", "lanes16")), forms
