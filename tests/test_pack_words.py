"""k_pack_t's placement and flush: four codes per OR of the bit window where a quad of codes fits 32 bits, code by code where it does
not, and a flush that visits only the words a tile holds.

Everything is byte-compared with the CPU oracle.  The shapes are the smallest at which this code can go wrong: one to three tiles of
4096 pixels (a tile is one workgroup: 256 threads of sixteen pixels, four quads each).  What a case is meant to reach -- bits per
pixel on both sides of the quad limit, a tile's bits at a word or window boundary -- is asserted from the oracle's own per-pixel
code lengths (trace_channel), never from the library under test."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TILE = 4096                    # pixels of a pack tile
WIN_BITS = (2048 - 1) * 32     # the most bits of a tile that take the one-window path ((FUSED_WIN_WORDS - 1) * 32)
SHAPES = [(128, 32), (128, 64), (97, 85), (256, 33)]  # (W, H): one tile, two tiles, tiles ending mid-row, an odd height
AMPLITUDES = [0, 1, 2, 4, 8, 16, 32, 64, 128]


@pytest.fixture(scope="module")
def enc():
    import felics_amd

    os.environ["FELICS_POISON"] = "1"  # the workspace is overwritten with garbage before every submission
    e = felics_amd.Encoder(0)
    del os.environ["FELICS_POISON"]
    yield e
    e.close()


def _planes(img):
    """The planes the encoder codes: the image itself, or Y / Co / Cg of an RGB image (the division truncates towards zero)."""
    if img.ndim == 2:
        return [img.astype(np.int32)]
    r, g, b = (img[..., i].astype(np.int32) for i in range(3))
    co = r - b
    t = b + np.trunc(co / 2).astype(np.int32)
    cg = g - t
    return [t + np.trunc(cg / 2).astype(np.int32), co, cg]


def _tile_bits(oracle, img):
    """Per plane, the bits of every tile as the oracle codes them (the file header belongs to the first tile of the first plane)."""
    h, w = img.shape[:2]
    out = []
    for i, p in enumerate(_planes(img)):
        nb = oracle.trace_channel(p, w, h, 0)["nbits"].astype(np.int64)
        t = [int(nb[a:a + TILE].sum()) for a in range(0, w * h, TILE)]
        if i == 0:
            t[0] += 8 * 14
        out.append(t)
    return out


def _check(enc, oracle, frames, what):
    """Every frame's stream against the oracle's; one compress_batch call per shape (a batch holds images of one shape and type)."""
    groups = {}
    for f in frames:
        groups.setdefault(f.shape, []).append(f)
    for shape, group in groups.items():
        got = enc.compress_batch(group)
        assert len(got) == len(group)
        for i, (g, f) in enumerate(zip(got, group)):
            want = oracle.compress(f)
            if g != want:
                n = min(len(g), len(want))
                diff = next((j for j in range(n) if g[j] != want[j]), n)
                raise AssertionError("%s frame %d of shape %s: differs from the oracle at byte %d (sizes %d vs %d)" % (what, i, shape, diff, len(g), len(want)))


def _ramp_noise(rng, w, h, a):
    """A smooth ramp plus uniform noise in [-a, a], modulo 256 (a = 128: every value as likely as any other)."""
    ramp = np.add.outer(np.arange(h), np.arange(w)) // 2
    return ((ramp + rng.integers(-a, a + 1, size=(h, w))) % 256).astype(np.uint8)


def _half_and_half(rng, w, h):
    """Left half quiet, right half loud: merged quads and quads placed code by code in the same wave."""
    img = _ramp_noise(rng, w, h, 1)
    img[:, w // 2:] = _ramp_noise(rng, w, h, 128)[:, w // 2:]
    return img


@pytest.mark.parametrize("w,h", SHAPES)
def test_quad_totals_on_both_sides_of_32(enc, oracle, w, h):
    """Sixteen-bit quads at the quiet end of the sweep, quads of more than 32 bits at the loud end (above 8 bits per pixel a quad's
    four codes do not fit a word), and everything between; then one frame with both in every row."""
    rng = np.random.default_rng(5)
    frames = [_ramp_noise(rng, w, h, a) for a in AMPLITUDES]
    bpp = [8.0 * len(oracle.compress(f)) / f.size for f in frames]
    assert bpp[0] < 6.0 and bpp[-1] > 9.0, bpp  # the sweep covers both sides (the oracle alone)
    # the limit itself: quads (four consecutive pixels from a multiple of four, as a thread takes them) of exactly 32 and of 33 bits
    totals = set()
    for f in frames:
        nb = oracle.trace_channel(f.astype(np.int32), w, h, 0)["nbits"].astype(np.int64)
        totals.update(nb[: w * h // 16 * 16].reshape(-1, 4).sum(1)[4 * ((w + 15) // 16):].tolist())  # (groups of sixteen below the first row)
    assert {31, 32, 33, 34} <= totals, sorted(totals)[:40]
    frames.append(_half_and_half(rng, w, h))
    _check(enc, oracle, frames, "noise sweep")


def test_quad_totals_rgb(enc, oracle):
    """The same through the int16 planes of RGB8 frames (chroma of noise: 9-bit differences)."""
    rng = np.random.default_rng(6)
    frames = []
    for w, h in ((128, 64), (97, 85)):
        for a in (0, 2, 16, 128):
            frames.append(np.stack([_ramp_noise(rng, w, h, a), _ramp_noise(rng, w, h, a // 2), _ramp_noise(rng, w, h, a)], axis=-1))
        frames.append(np.stack([_half_and_half(rng, w, h), _ramp_noise(rng, w, h, 1), _half_and_half(rng, w, h)], axis=-1))
    _check(enc, oracle, frames, "rgb noise sweep")


def _spikes(w, h, every, value=255, blip=0):
    """A zero frame with `value` in every `every`th pixel (and, blip != 0, a 1 in every `blip`th)."""
    img = np.zeros(w * h, np.uint8)
    if blip:
        img[blip - 1::blip] = 1
    img[every - 1::every] = value
    return img.reshape(h, w)


@pytest.mark.parametrize("w,h", SHAPES)
def test_sparse_spikes_in_a_flat_frame(enc, oracle, w, h):
    """One 255 in every 5th, 16th, 17th pixel of a zero frame: quads of one long and three 1-bit codes.  Every 2nd and 3rd pixel: more
    events than the word path takes, so the same on the k path.  Spikes that regular teach the estimator their size (no code beyond
    15 bits), so the long codes come from rare spikes among blips of 1, which keep k at 0: codes of 24 to 32 bits (too long for an
    event's word), of 62 and of 257 bits (the general path) beside merged quads."""
    frames = [_spikes(w, h, n) for n in (5, 16, 17, 2, 3)] + [_spikes(w, h, n, 40) for n in (5, 17, 2)]
    rare = [_spikes(w, h, 251, 30, blip=3), _spikes(w, h, 251, 60, blip=3), _spikes(w, h, 509, 255, blip=7)]
    longest = [int(oracle.trace_channel(f.astype(np.int32), w, h, 0)["nbits"][2:].max()) for f in rare]
    assert 23 < longest[0] <= 32 < longest[1] < longest[2], longest
    ones = oracle.trace_channel(frames[0].astype(np.int32), w, h, 0)["nbits"]
    assert int((ones == 1).sum()) > w * h // 3 and int(ones[2:].max()) > 8
    _check(enc, oracle, frames + rare, "spikes")
    _check(enc, oracle, [np.stack([f, f[::-1], 255 - f], axis=-1).copy() for f in frames[:4] + rare], "rgb spikes")


def _shared(tb):
    """(first word shared, last word shared) of every tile of a plane whose tiles hold tb bits"""
    out, lo = [], 0
    for b in tb:
        out.append((lo % 32 != 0, (lo + b) % 32 != 0))
        lo += b
    return out


def test_tile_totals_at_the_flush_boundaries(enc, oracle):
    """Constant frames: every code behind the first two samples is one bit, a full tile exactly 4096 bits = 128 words, the first tile
    4270 bits with the header -- so every later tile starts in the middle of a word.  The last tile holds 1, 31, 32, 33 and 4095 bits
    (8191 pixels behind the first tile); 18 bits end the stream on a word boundary; a first tile padded to whole words gives a
    tile that starts and ends on one.  (A tile of no bits at all cannot occur: every pixel costs at least one.)"""
    shapes = {(17, 241): 1, (127, 97): 31, (129, 32): 32, (35, 235): 33, (1117, 11): 4095, (22, 187): 18}
    frames, combos = [], set()
    for (w, h), last in shapes.items():
        f = np.full((h, w), 9, np.uint8)
        tb = _tile_bits(oracle, f)[0]
        assert tb[0] == 4270 and all(b == TILE for b in tb[1:-1]) and tb[-1] == last, ((w, h), tb)
        combos.update(_shared(tb))
        frames.append(f)
    # a first tile of whole words: two samples out of range, eighteen bits between them
    aligned = np.full((96, 128), 9, np.uint8)
    aligned[2, 5] = aligned[10, 50] = 11
    assert _tile_bits(oracle, aligned)[0] == [4288, TILE, TILE]
    combos.update(_shared(_tile_bits(oracle, aligned)[0]))
    frames.append(aligned)
    assert combos == {(False, False), (False, True), (True, False), (True, True)}, combos
    _check(enc, oracle, frames, "constant frames")
    _check(enc, oracle, [np.stack([f, f, f], axis=-1) for f in frames[:4]], "constant rgb frames")


def _chroma_checker(rows, amp_last):
    """16 x 256 RGB8, one tile a plane: red against blue in a checkerboard on the first `rows` rows (Co swings by 511 from pixel to
    pixel: more than 16 bits a pixel), the last of them with amplitude amp_last, grey below."""
    h, w = 256, 16
    yy, xx = np.indices((h, w))
    odd = ((xx + yy) & 1).astype(bool)
    img = np.full((h, w, 3), 128, np.uint8)
    for y in range(rows):
        a = 128 if y < rows - 1 else amp_last
        hi, lo = min(255, 128 + a), 128 - a
        img[y, :, 0] = np.where(odd[y], hi, lo)
        img[y, :, 2] = np.where(odd[y], lo, hi)
    return img


def test_near_full_and_over_full_windows(enc, oracle):
    """A Co tile just under (FUSED_WIN_WORDS - 1) * 32 bits -- the fullest window the one-window path places and flushes -- one just
    over it (the several-window path, one window), and one of 2836 words (two windows).  No 8-bit gray content reaches 16 bits per pixel;
    the chroma planes of a red / blue checkerboard do."""
    def co_bits(img):
        return _tile_bits(oracle, img)[1][0]

    rows = next(r for r in range(1, 257) if co_bits(_chroma_checker(r, 128)) > WIN_BITS)
    by_amp = {a: co_bits(_chroma_checker(rows, a)) for a in range(0, 129)}
    under = max((b, a) for a, b in by_amp.items() if b <= WIN_BITS)
    over = min((b, a) for a, b in by_amp.items() if b > WIN_BITS)
    assert WIN_BITS - 64 <= under[0] <= WIN_BITS < over[0] <= WIN_BITS + 64, (rows, under, over)
    full = _chroma_checker(256, 128)
    assert co_bits(full) > (2048 + 512) * 32  # a second window of more than 512 words
    _check(enc, oracle, [_chroma_checker(rows, under[1]), _chroma_checker(rows, over[1]), full], "chroma checker")


def test_pitched_and_mixed_instantiations(enc, oracle):
    """The same placement in the kernel's other forms: gray8 crops of a pitched device surface read in place
    (felics_compress_views_device) and images of different shapes and types in one call (felics_compress_images_device)."""
    import torch

    from felics_amd import api

    rng = np.random.default_rng(7)
    surface = np.zeros((100, 272), np.uint8)
    surface[:, :136] = _half_and_half(rng, 136, 100)
    surface[:, 136:] = _spikes(136, 100, 5)
    crops = [surface[3:88, 2:99], surface[1:65, 136:264], surface[0:33, 8:264]]  # 97 x 85, 128 x 64 (spikes), 256 x 33 (both)
    dev = torch.from_numpy(surface).cuda()
    torch.cuda.synchronize()
    base = surface.__array_interface__["data"][0]
    views = [(dev.data_ptr() + c.__array_interface__["data"][0] - base, c.shape[1], c.shape[0], 0, 0, c.strides[0], 1, 0) for c in crops]
    cap = sum(c.size * 2 + 4096 for c in crops)
    out = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    offs, lens = enc.compress_views_device(views, out.data_ptr(), cap)
    host = out.cpu().numpy()
    for c, o, n in zip(crops, offs, lens):
        assert host[int(o):int(o) + int(n)].tobytes() == oracle.compress(np.ascontiguousarray(c)), c.shape

    imgs = [_half_and_half(rng, 128, 64), _spikes(97, 85, 17), np.full((241, 17), 9, np.uint8),
            np.stack([_half_and_half(rng, 256, 33), _ramp_noise(rng, 256, 33, 2), _spikes(256, 33, 5)], axis=-1).copy(), _chroma_checker(256, 128)]
    tensors = [torch.from_numpy(im).cuda() for im in imgs]
    torch.cuda.synchronize()
    descs = []
    for im, t in zip(imgs, tensors):
        _, w, h, color, depth = api._describe(im)
        descs.append((t.data_ptr(), w, h, int(color), int(depth)))
    cap = sum(im.size * 4 + 4096 for im in imgs)
    out = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    offs, lens = enc.compress_images_device(descs, out.data_ptr(), cap)
    host = out.cpu().numpy()
    for im, o, n in zip(imgs, offs, lens):
        assert host[int(o):int(o) + int(n)].tobytes() == oracle.compress(im), im.shape
