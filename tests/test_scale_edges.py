"""The 32-bit edges: passes of more than 2^31 samples, the real pass split, decodes of more than 2^32 bytes, many tiny 8-bit frames.

Every expected byte comes from the CPU oracle (one call per DISTINCT frame of a batch), every expected pixel from the source frame,
every expected pass count from the bounds documented in felics_encode.cpp (restated below as constants); nothing is compared with
another output of the library.  The big batches are built on the device: frame[i] = base[i % 7] (seven contents, noise and flat
among them, so stream sizes differ widely and no power-of-two wrap lands on a frame of the same content), except for a few frames
with content of their own: the first, the last, and the two around every 2^31 / 2^32 boundary of the sample index and of the input's
byte offset.

The sizes below are module-level values, so the arithmetic (pass bounds, the frames at the boundaries, each test's memory need) can
be checked without a GPU.  A test whose stated need exceeds the free device memory skips with both numbers."""
import contextlib
import io
import os
import subprocess
import time

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
E_BUFFER_TOO_SMALL = -8
GIB = 1 << 30
K = 7  # distinct contents of a big batch

# ---- the library's constants (felics_kernels.h) and bounds (felics_encode.cpp, max_images_per_pass) -------------------------------
SORT_TILE = 4096           # felics_kernels.h: SORT_TILE == PACK_TILE
REC = 16                   # felics_kernels.h: events per record
PACK_THREADS = 256
SLICES = 12                # felics_host.h
STAGE_PAD = 64
NCTX = {1: 256, 3: 512}    # nctx_of<>: contexts per plane of gray8 / of the Y, Co, Cg planes of RGB8
NCTX_MAX = 512             # NCTX
PASS_MAX_SAMPLES_8 = 0xE0000000   # max_images_per_pass: samples and records of an 8-bit pass
PASS_MAX_SAMPLES_16 = 0x40000000  # max_images_per_pass: samples of a 16-bit pass
WIDE_MAX_PLANES = 1 << 16         # max_images_per_pass: planes of a 16-bit pass
PASS_MAX_CHAINS = 1 << 23         # felics_host.h, PASS_MAX_CHAINS: chains (plane x context) of an 8-bit pass
MIX_MAX_IMAGES = 8192             # felics_mixed.cpp: images of one mixed sub-batch
DECODE_LDS_LIMIT = 160 * 1024     # felics_kernels.h
DEC16_TABLE_BYTES = (2 * 65535 + 1) * 16 * 4  # felics_gpudecode.hip, decode16_table_bytes(1): 8.4 MB per stream of a pass
FALLBACKS = ("lookback_fallbacks", "scatter_fallbacks", "tile_overflows", "slot_overflows")


def cdiv(a, b):
    return -(-a // b)


def tile_cap_max(nctx, npix):
    px = min(npix, SORT_TILE)
    return (px + (REC - 1) * min(nctx, px) + REC - 1) // REC * REC


def tile_cap_default(nctx, npix):
    return min(6144 if nctx == 256 else 8192, tile_cap_max(nctx, npix))


def images_per_pass(npix, planes, sixteen=False):
    """max_images_per_pass (felics_encode.cpp)"""
    per_image = npix * planes
    if sixteen:
        return max(1, min(PASS_MAX_SAMPLES_16 // per_image, WIDE_MAX_PLANES // planes))
    rec_per_image = cdiv(npix, SORT_TILE) * planes * (tile_cap_max(NCTX_MAX, min(npix, SORT_TILE)) // REC)
    return max(1, min(PASS_MAX_SAMPLES_8 // per_image, PASS_MAX_SAMPLES_8 // rec_per_image, PASS_MAX_CHAINS // (planes * NCTX[planes])))


def decode16_lds_bytes(w):
    """felics_gpudecode.hip: DEC16_SLOTS * DEC16_ROW * 4 + DEC16_SLOTS * 4 + two rows of int32"""
    return 512 * 16 * 4 + 512 * 4 + 2 * ((w + 63) & ~63) * 4


def _reserved(b):
    return b + b // 8 + 256  # reserve(): a little slack


def lane_need_8(nimages, planes, npix, fused=True):
    """Device bytes one lane holds after an 8-bit pass of this geometry: run_lane's reserve calls (and launch_sub_batch's planes)."""
    nctx, et = NCTX[planes], (1 if planes == 1 else 2)
    nplanes, tiles = nimages * planes, cdiv(npix, SORT_TILE)
    ptiles = nplanes * tiles
    slots = ptiles * tile_cap_default(nctx, npix)
    recs, nchains = slots // REC, nplanes * nctx
    parts = [slots * et + STAGE_PAD, slots * 2 + STAGE_PAD, slots + STAGE_PAD, ptiles * nctx * 4, ptiles * 4, recs * 8 + 64, recs * 16 + 64,
             SLICES * nchains * 8, nchains * 32, 64 + 4 * (SLICES + 2) + 4 * SLICES, ptiles * 4, ptiles * 8, nplanes * 16, nimages * 8,
             (nimages + 1) * 8, ptiles * 8, ptiles * 4, ptiles * 4]
    if not fused:
        parts += [nplanes * npix + STAGE_PAD, ptiles * PACK_THREADS * 2]
    if planes == 3:
        parts.append(nplanes * npix * 2 + STAGE_PAD)
        if fused:
            parts.append(((npix + npix // 4 + 64 + 15) & ~15) * nimages * 2)
    return sum(_reserved(p) for p in parts)


def lane_need_16(nimages, npix):
    """run_wide's reserve calls for gray16 (wide_sizes: two record buffers and the heads at 8 bytes a sample, k_map, group_bits)."""
    ns, tiles = nimages * npix, cdiv(npix, SORT_TILE)
    parts = [ns * 8 + 512, ns * 8 + 512, ns * 8 + 64, ns + STAGE_PAD, nimages * tiles * PACK_THREADS * 4, nimages * tiles * 12,
             (ns // 2048 + nimages) * 256 * 4 * 2]
    return sum(_reserved(p) for p in parts)


def boundary_frames(n, samples_per_frame, bytes_per_frame):
    """Frames with content of their own: the first, the last, and around every 2^31 / 2^32 boundary (of the sample index and of the
    input's byte offset) the frame that holds the last unit below it and the frame after that one."""
    out = {0, n - 1}
    for per in (samples_per_frame, bytes_per_frame):
        for b in (1 << 31, 1 << 32):
            if n * per > b:
                a = (b - 1) // per
                out |= {a, min(a + 1, n - 1)}
    return sorted(out)


def slots_cap(n, frame_bytes):
    return int(n * 1.25 * frame_bytes) + (1 << 20)


W4K, H4K = 3840, 2160
NPIX_4K = W4K * H4K                                   # 8 294 400
N_GRAY8 = images_per_pass(NPIX_4K, 1)                 # 453: one pass of 3.757 G samples
N_RGB8 = images_per_pass(NPIX_4K, 3)                  # 151
N_GRAY16 = images_per_pass(NPIX_4K, 1, True)          # 129
W_ODD, H_ODD = 1919, 1081
NPIX_ODD = W_ODD * H_ODD                              # 2 074 439: 506.45 tiles, 2^31 / npix = 1035.2
N_ODD = 1205                                          # 2.4997 G samples, one pass (the bound is 1811)
SLACK = 2 * GIB  # torch's temporaries while frames are generated, the allocator's rounding
# input + output + one lane's workspace (the larger of the two geometries run on the context: fixed slots / exact placement)
NEED_GRAY8 = (N_GRAY8 + 1) * NPIX_4K + slots_cap(N_GRAY8 + 1, NPIX_4K) + max(lane_need_8(N_GRAY8, 1, NPIX_4K), lane_need_8(N_GRAY8, 1, NPIX_4K, False)) + SLACK
NEED_RGB8 = (N_RGB8 + 1) * NPIX_4K * 3 + slots_cap(N_RGB8 + 1, NPIX_4K * 3) + lane_need_8(N_RGB8, 3, NPIX_4K) + SLACK
NEED_ODD = N_ODD * NPIX_ODD + slots_cap(N_ODD, NPIX_ODD) + lane_need_8(N_ODD, 1, NPIX_ODD) + SLACK
NEED_GRAY16 = (N_GRAY16 + 1) * NPIX_4K * 2 + slots_cap(N_GRAY16 + 1, NPIX_4K * 2) + lane_need_16(N_GRAY16, NPIX_4K) + SLACK

N_DEC_WAVES = 520                                     # 4K gray8: 4.31 GB of pixels
N_DEC_LANES, WH_DEC_LANES = 70016, 256                # 256 x 256 gray8: 4.59 GB
N_DEC_RGB = 22016                                     # 256 x 256 RGB8: 4.33 GB of pixels, 8.66 GB of int16 planes
N_DEC16 = 300                                         # 4K gray16: 4.98 GB
NEED_DEC_WAVES = N_DEC_WAVES * NPIX_4K + K * 2 * NPIX_4K + SLACK
NEED_DEC_LANES = N_DEC_LANES * WH_DEC_LANES ** 2 + _reserved(N_DEC_LANES * 256 * 3 * 4) + SLACK
NEED_DEC_RGB = N_DEC_RGB * WH_DEC_LANES ** 2 * 3 + _reserved(N_DEC_RGB * WH_DEC_LANES ** 2 * 3 * 2) + _reserved(N_DEC_RGB * 3 * 512 * 3 * 4) + SLACK
NEED_DEC_FAR = (1 << 32) + (64 << 20) + SLACK
NEED_DEC_MIXED = 2 * (N_DEC_WAVES * NPIX_4K + (64 << 20)) + K * 2 * NPIX_4K + SLACK  # (the frames and a scratch copy for the gap check)
NEED_DEC16 = N_DEC16 * NPIX_4K * 2 + _reserved(N_DEC16 * DEC16_TABLE_BYTES) + K * 3 * NPIX_4K + SLACK

N_TINY_GRAY, N_TINY_RGB, TINY_CONTENTS = 200000, 70000, 257
N_TINY_MIXED, TINY_MIXED_CONTENTS = 40000, 300
TINY_PASSES_GRAY = cdiv(N_TINY_GRAY * 1 * NCTX[1], PASS_MAX_CHAINS)   # 7
TINY_PASSES_RGB = cdiv(N_TINY_RGB * 3 * NCTX[3], PASS_MAX_CHAINS)     # 13
MAX_LANES = 4                     # felics_host.h: submissions in flight, each with a workspace of its own (felics_compress_batch's chunks)
NEED_TINY = MAX_LANES * max(lane_need_8(images_per_pass(64, 1), 1, 64), lane_need_8(images_per_pass(64, 3), 3, 64)) + SLACK
# (a mixed job's geometry: one tile of SORT_TILE pixels a plane)
NEED_TINY_MIXED = MAX_LANES * max(lane_need_8(MIX_MAX_IMAGES, 1, SORT_TILE), lane_need_8(images_per_pass(SORT_TILE, 3), 3, SORT_TILE)) + SLACK
W_IDX2, H_IDX2, SEG_IDX2 = 64, 65, 4096                # two checkpoints a frame
N_IDX2 = images_per_pass(W_IDX2 * H_IDX2, 1) + 3      # 32 771 gray8 frames: two real passes, each with its indexes
MIXED_JOBS = sum(cdiv(N_TINY_MIXED // 2, min(MIX_MAX_IMAGES, images_per_pass(SORT_TILE, planes))) for planes in (1, 3))  # 3 + 4


@pytest.mark.gpu
def test_size_arithmetic():
    """The constants above against each other and against the figures the docstrings quote.  Marked like the rest of the file, but it
    touches no GPU: `python -c "from tests import test_scale_edges as t; t.test_size_arithmetic()"` checks it anywhere."""
    assert (N_GRAY8, N_RGB8, N_GRAY16) == (453, 151, 129)
    assert 1 << 31 < N_GRAY8 * NPIX_4K <= PASS_MAX_SAMPLES_8 < (N_GRAY8 + 1) * NPIX_4K
    assert 1 << 31 < N_RGB8 * 3 * NPIX_4K <= PASS_MAX_SAMPLES_8 < (N_RGB8 + 1) * 3 * NPIX_4K
    assert N_GRAY16 * NPIX_4K <= PASS_MAX_SAMPLES_16 < (N_GRAY16 + 1) * NPIX_4K
    assert N_GRAY8 * cdiv(NPIX_4K, SORT_TILE) * tile_cap_default(256, NPIX_4K) > 1 << 32  # slots of the pass
    assert 1 << 31 < N_ODD * NPIX_ODD < 1 << 32 and N_ODD <= images_per_pass(NPIX_ODD, 1) and NPIX_ODD % SORT_TILE and W_ODD % 64
    assert boundary_frames(N_GRAY8 + 1, NPIX_4K, NPIX_4K) == [0, 258, 259, 453]  # (2^32 is past the batch)
    assert boundary_frames(N_RGB8 + 1, 3 * NPIX_4K, 3 * NPIX_4K) == [0, 86, 87, 151]
    assert boundary_frames(N_GRAY16 + 1, NPIX_4K, 2 * NPIX_4K) == [0, 129]  # 2.16 G bytes: 2^31 lies in the last frame
    assert boundary_frames(N_ODD, NPIX_ODD, NPIX_ODD) == [0, 1035, 1036, 1204]
    assert images_per_pass(64, 1) == 1 << 15 and images_per_pass(64, 3) == 5461
    assert (TINY_PASSES_GRAY, TINY_PASSES_RGB, MIXED_JOBS) == (7, 13, 7)
    assert N_IDX2 == (1 << 15) + 3 and cdiv(N_IDX2, images_per_pass(W_IDX2 * H_IDX2, 1)) == 2 and cdiv(W_IDX2 * H_IDX2, SEG_IDX2) == 2
    assert TINY_PASSES_GRAY == cdiv(N_TINY_GRAY, images_per_pass(64, 1)) and TINY_PASSES_RGB == cdiv(N_TINY_RGB, images_per_pass(64, 3))
    for n, per in ((N_DEC_WAVES, NPIX_4K), (N_DEC_LANES, WH_DEC_LANES ** 2), (N_DEC_RGB, 3 * WH_DEC_LANES ** 2), (N_DEC16, 2 * NPIX_4K)):
        assert n * per > 1 << 32
    assert N_DEC_RGB * 3 * WH_DEC_LANES ** 2 * 2 > 1 << 33  # the int16 planes of the RGB decode
    assert decode16_lds_bytes(W4K) <= DECODE_LDS_LIMIT      # 4K gray16 rows are decoded on the device
    for need in (NEED_GRAY8, NEED_RGB8, NEED_ODD, NEED_GRAY16, NEED_DEC_WAVES, NEED_DEC_LANES, NEED_DEC_RGB, NEED_DEC_FAR, NEED_DEC_MIXED,
                 NEED_DEC16, NEED_TINY, NEED_TINY_MIXED):
        assert GIB < need < 120 * GIB, need


# ---- helpers -----------------------------------------------------------------------------------------------------------------

def _room(need):
    import torch

    torch.cuda.empty_cache()
    free, _ = torch.cuda.mem_get_info()
    if free < need:
        pytest.skip("needs %.1f GB of device memory, %.1f GB are free" % (need / 1e9, free / 1e9))


@contextlib.contextmanager
def _env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    os.environ.update(kv)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


@contextlib.contextmanager
def _fresh_encoder():
    """A context of its own, closed afterwards; torch's cache emptied so that the next test starts with the memory back."""
    import felics_amd
    import torch

    e = felics_amd.Encoder(0)
    try:
        yield e
    finally:
        e.close()
        torch.cuda.empty_cache()


def _content8(w, h, planes, frame, kind):
    """One 8-bit frame on the device: synth_torch's S1 / S2 / S3 (RGB: rgb8 for S1, the gray frame in all three channels otherwise)."""
    import torch
    from felics_amd import synth_torch

    if planes == 1:
        return synth_torch.gray8(w, h, frame, kind)
    if kind == "S1":
        return synth_torch.rgb8(w, h, frame)
    return torch.stack([synth_torch.gray8(w, h, frame, kind)] * 3, dim=-1)


BASE_KINDS = ("S1", "S2", "S3", "S1", "S1", "S2", "S1")  # base[k] = frame k of that kind: noise and flat among them


def _batch8(n, w, h, planes, special):
    """(frames on the device, key of every frame's content, {key: numpy frame})"""
    import torch

    shape = (n, h, w) if planes == 1 else (n, h, w, 3)
    frames = torch.empty(shape, dtype=torch.uint8, device="cuda")
    keys = [i % K for i in range(n)]
    content = {}
    for k in range(K):
        f = _content8(w, h, planes, k, BASE_KINDS[k])
        frames[k::K] = f
        content[k] = f.cpu().numpy()
    for j, i in enumerate(special):
        f = _content8(w, h, planes, 1000 + i, "S2" if j % 3 == 2 else "S1")
        frames[i] = f
        keys[i] = "own%d" % i
        content[keys[i]] = f.cpu().numpy()
    torch.cuda.synchronize()
    return frames, keys, content


def _batch16(n, w, h, special):
    """gray16: synth.gray16 frames, 12-bit noise and a flat frame uploaded once and replicated with torch (as int16 bit patterns)"""
    import torch
    from felics_amd import synth

    rng = np.random.default_rng(16)
    host = [synth.gray16(w, h, k) for k in range(K)]
    host[1] = (0x7000 + rng.integers(0, 4096, size=(h, w))).astype(np.uint16)
    host[2] = np.full((h, w), 0x8000, np.uint16)
    frames = torch.empty((n, h, w), dtype=torch.int16, device="cuda")
    keys = [i % K for i in range(n)]
    content = dict(enumerate(host))
    for k in range(K):
        frames[k::K] = torch.from_numpy(host[k].view(np.int16)).cuda()
    for i in special:
        f = synth.gray16(w, h, 1000 + i)
        frames[i] = torch.from_numpy(f.view(np.int16)).cuda()
        keys[i] = "own%d" % i
        content[keys[i]] = f
    torch.cuda.synchronize()
    return frames, keys, content


def _check_streams(d_out, offs, lens, keys, want, what=""):
    """Offsets 16-byte aligned, ascending, not overlapping; EVERY stream equal to the oracle's stream of its content, byte for byte
    (copied to the host in slices of about 1 GB)."""
    n = len(keys)
    offs, lens = np.asarray(offs).astype(np.int64), np.asarray(lens).astype(np.int64)
    assert len(offs) == n and len(lens) == n
    assert (offs % 16 == 0).all(), what
    assert (offs[1:] >= offs[:-1] + lens[:-1]).all(), what
    wl = np.array([len(want[k]) for k in keys], dtype=np.int64)
    bad = np.nonzero(lens != wl)[0]
    assert bad.size == 0, "%s stream %d (content %r): %d bytes, the oracle's has %d (%d streams differ in size)" % (
        what, bad[0], keys[bad[0]], lens[bad[0]], wl[bad[0]], bad.size)
    arrs = {k: np.frombuffer(v, np.uint8) for k, v in want.items()}
    i = 0
    while i < n:
        a, j = int(offs[i]), i + 1
        while j < n and int(offs[j] + lens[j]) - a <= GIB:
            j += 1
        host = d_out[a:int(offs[j - 1] + lens[j - 1])].cpu().numpy()
        for t in range(i, j):
            got = host[int(offs[t]) - a:int(offs[t] + lens[t]) - a]
            if not np.array_equal(got, arrs[keys[t]]):
                d = int(np.nonzero(got != arrs[keys[t]])[0][0])
                pytest.fail("%s stream %d of %d (content %r, offset %d): first differing byte %d of %d" % (what, t, n, keys[t], offs[t], d, lens[t]))
        i = j


def _delta(enc, before):
    now = enc.stats()
    return {k: now[k] - before[k] for k in ("submissions",) + FALLBACKS}


def _clean(passes):
    return dict({k: 0 for k in FALLBACKS}, submissions=passes)


@contextlib.contextmanager
def _pass_bound_and_split(make_batch, oracle, n1, w, h, color, depth, frame_bytes, entry_points=("batch",)):
    """n1 frames (the pass bound) in one submission, n1 + 1 in two: every stream against the oracle, no fallback."""
    import torch

    n2 = n1 + 1
    frames, keys, content = make_batch(n2)
    want = {k: oracle.compress(v) for k, v in content.items()}
    cap = slots_cap(n2, frame_bytes)
    d_out = torch.empty(cap, dtype=torch.uint8, device="cuda")
    with _fresh_encoder() as e:
        for n, passes in ((n1, 1), (n2, 2)):
            for entry in (entry_points if n == n2 else ("batch",)):
                d_out.zero_()
                torch.cuda.synchronize()
                before = e.stats()
                t0 = time.time()
                if entry == "batch":
                    offs, lens = e.compress_batch_device(frames.data_ptr(), n, w, h, color, depth, d_out.data_ptr(), cap)
                else:  # n > one pass: felics_submit_batch_device does it now and hands the result over at the wait
                    offs, lens = e.wait_batch(e.submit_batch_device(frames.data_ptr(), n, w, h, color, depth, d_out.data_ptr(), cap))
                print("%s n=%d: %.2f s, %s" % (entry, n, time.time() - t0, _delta(e, before)))
                assert _delta(e, before) == _clean(passes), (entry, n)
                _check_streams(d_out, offs, lens, keys[:n], want, "%s n=%d" % (entry, n))
        yield e, frames, keys, want, d_out
    del frames, d_out


# ---- 1. encoder: one pass between 2^31 samples and the bound, and the real split ----------------------------------------------

@pytest.mark.gpu
def test_gray8_4k_pass_bound_split_and_exact_placement(oracle):
    """453 4K gray8 frames are ONE pass of 3.757 G samples (5.6 G slots); 454 take two passes, through felics_compress_batch_device
    and through felics_submit_batch_device / felics_wait_batch ("not the plain case: do it now"); then the same 454 frames into a
    buffer of exactly sum((len + 15) // 16 * 16) bytes of the oracle's sizes (streams back to back across the pass join; the slots
    that capacity leaves overflow on purpose, so slot_overflows moves here), and 16 bytes less: FELICS_E_BUFFER_TOO_SMALL.
    Needs NEED_GRAY8 = 51 GB of device memory: 3.8 GB of frames, 4.7 GB of output, one lane's workspace for 453 frames (36 GB with
    fixed slots, 41 GB for exact placement)."""
    import torch
    from felics_amd import api

    _room(NEED_GRAY8)
    special = sorted(set(boundary_frames(N_GRAY8 + 1, NPIX_4K, NPIX_4K)) | {N_GRAY8 - 1})
    with _pass_bound_and_split(lambda n: _batch8(n, W4K, H4K, 1, special), oracle, N_GRAY8, W4K, H4K, 0, 0, NPIX_4K,
                               ("batch", "submit")) as (e, frames, keys, want, d_out):
        n = N_GRAY8 + 1
        exact = sum((len(want[k]) + 15) // 16 * 16 for k in keys)
        d_out.zero_()
        torch.cuda.synchronize()
        before = e.stats()
        offs, lens = e.compress_batch_device(frames.data_ptr(), n, W4K, H4K, 0, 0, d_out.data_ptr(), exact)
        d = _delta(e, before)
        print("exact placement:", d)
        assert d["submissions"] >= 2 and d["lookback_fallbacks"] == d["scatter_fallbacks"] == d["tile_overflows"] == 0, d
        _check_streams(d_out, offs, lens, keys, want, "exact")
        assert int(offs[0]) == 0 and all(int(offs[i + 1]) == int(offs[i]) + (int(lens[i]) + 15) // 16 * 16 for i in range(n - 1))
        assert int(offs[-1]) + (int(lens[-1]) + 15) // 16 * 16 == exact
        with pytest.raises(api.FelicsError) as ei:
            e.compress_batch_device(frames.data_ptr(), n, W4K, H4K, 0, 0, d_out.data_ptr(), exact - 16)
        assert ei.value.code == E_BUFFER_TOO_SMALL and ("need %d bytes" % exact) in str(ei.value)


@pytest.mark.gpu
def test_rgb8_4k_pass_bound_and_split(oracle):
    """151 4K RGB8 frames (453 planes, one pass; the int16 planes buffer is 7.5 GB: k_rgb8_to_planes and k_concat_planes past 2^32
    bytes) and 152 (two passes).  Needs NEED_RGB8 = 80 GB: 3.8 GB of frames, 4.7 GB of output, 69 GB of workspace."""
    _room(NEED_RGB8)
    special = sorted(set(boundary_frames(N_RGB8 + 1, 3 * NPIX_4K, 3 * NPIX_4K)) | {N_RGB8 - 1})
    with _pass_bound_and_split(lambda n: _batch8(n, W4K, H4K, 3, special), oracle, N_RGB8, W4K, H4K, 1, 0, 3 * NPIX_4K):
        pass


@pytest.mark.gpu
def test_gray8_odd_shape_past_2_31_samples(oracle):
    """1205 gray8 frames of 1919 x 1081 (506.45 tiles a frame, rows ending mid-tile, 2^31 / npix = 1035.2): one pass of 2.4997 G
    samples.  Needs NEED_ODD = 32 GB: 2.5 GB of frames, 3.1 GB of output, 24 GB of workspace."""
    import torch

    _room(NEED_ODD)
    n = N_ODD
    frames, keys, content = _batch8(n, W_ODD, H_ODD, 1, boundary_frames(n, NPIX_ODD, NPIX_ODD))
    want = {k: oracle.compress(v) for k, v in content.items()}
    cap = slots_cap(n, NPIX_ODD)
    d_out = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    with _fresh_encoder() as e:
        before = e.stats()
        offs, lens = e.compress_batch_device(frames.data_ptr(), n, W_ODD, H_ODD, 0, 0, d_out.data_ptr(), cap)
        assert _delta(e, before) == _clean(1)
        _check_streams(d_out, offs, lens, keys, want, "odd")
    del frames, d_out


@pytest.mark.gpu
def test_gray16_4k_pass_bound_and_split(oracle):
    """129 4K gray16 frames are one 16-bit pass (0x40000000 // 8 294 400), 130 two; the library's own choice of the four-lane chain
    kernel.  Needs NEED_GRAY16 = 39 GB: 2.2 GB of frames, 2.7 GB of output, 32 GB of workspace."""
    _room(NEED_GRAY16)
    special = sorted(set(boundary_frames(N_GRAY16 + 1, NPIX_4K, 2 * NPIX_4K)) | {N_GRAY16 - 1})
    with _pass_bound_and_split(lambda n: _batch16(n, W4K, H4K, special), oracle, N_GRAY16, W4K, H4K, 0, 1, 2 * NPIX_4K):
        pass


# ---- 2. decoder past 2^32 ----------------------------------------------------------------------------------------------------

def _streams_on_device(streams, pad_to=0):
    """The streams back to back at 16-byte aligned offsets in one device buffer: (tensor, offsets, lens)"""
    import torch

    offs, blob = [], bytearray()
    for s in streams:
        blob += bytes(-len(blob) % 16)
        offs.append(len(blob))
        blob += s
    blob += bytes(max(16, pad_to - len(blob)))
    return torch.from_numpy(np.frombuffer(bytes(blob), dtype=np.uint8).copy()).cuda(), offs, [len(s) for s in streams]


def _decode_repeated(enc, oracle, base, n, need, forms):
    """n streams referencing the oracle's K streams of `base` through offsets / lens, decoded in one felics_decompress_batch_device
    call per form; the pixels compared on the device with the source frames, group by group."""
    import torch

    _room(need)
    d_streams, so, sl = _streams_on_device([oracle.compress(b) for b in base])
    offs = np.array([so[i % K] for i in range(n)], np.uint64)
    lens = np.array([sl[i % K] for i in range(n)], np.uint64)
    dt = torch.int16 if base[0].dtype == np.uint16 else torch.uint8
    dev = [torch.from_numpy(b.view(np.int16) if b.dtype == np.uint16 else b).cuda() for b in base]
    d_px = torch.empty((n,) + base[0].shape, dtype=dt, device="cuda")
    for form in forms:
        d_px.fill_(0x5A)
        torch.cuda.synchronize()
        t0 = time.time()
        with (_env(FELICS_TEST_DECODE_LANES=form) if form else contextlib.nullcontext()):
            hdr, status = enc.decompress_batch_device(d_streams.data_ptr(), offs, lens, d_px.data_ptr(), d_px.numel() * d_px.element_size())
        print("decode n=%d form=%r: %.2f s" % (n, form, time.time() - t0))
        assert (status == 0).all() and (hdr.width, hdr.height) == (base[0].shape[1], base[0].shape[0])
        for k in range(K):
            assert bool((d_px[k::K] == dev[k]).all()), (form, k)
    del d_px


def _base8(w, h, planes):
    from felics_amd import synth

    if planes == 1:
        return [synth.gray8(w, h, k, BASE_KINDS[k]) for k in range(K)]
    rng = np.random.default_rng(3)
    base = [synth.rgb8(w, h, k) for k in range(K)]
    base[1] = rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)
    base[2] = np.full((h, w, 3), 128, np.uint8)
    return base


@pytest.mark.gpu
def test_decode_gray8_4k_one_wave_per_stream(oracle):
    """520 4K gray8 streams, one wave per stream (FELICS_TEST_DECODE_LANES=0): 4.31 GB of pixels.  Needs NEED_DEC_WAVES = 6.6 GB."""
    with _fresh_encoder() as e:
        _decode_repeated(e, oracle, _base8(W4K, H4K, 1), N_DEC_WAVES, NEED_DEC_WAVES, ("0",))


@pytest.mark.gpu
def test_decode_gray8_lane_form(oracle):
    """70 016 gray8 streams of 256 x 256, 64 to a wave: the library's own choice of form, and the form forced.  4.59 GB of pixels.
    Needs NEED_DEC_LANES = 7.0 GB."""
    with _fresh_encoder() as e:
        _decode_repeated(e, oracle, _base8(WH_DEC_LANES, WH_DEC_LANES, 1), N_DEC_LANES, NEED_DEC_LANES, (None, "1"))


@pytest.mark.gpu
def test_decode_rgb8_lane_form(oracle):
    """22 016 RGB8 streams of 256 x 256 in the lane form: 4.33 GB of pixels, 8.66 GB (> 2^33) of int16 planes.
    Needs NEED_DEC_RGB = 16.7 GB."""
    with _fresh_encoder() as e:
        _decode_repeated(e, oracle, _base8(WH_DEC_LANES, WH_DEC_LANES, 3), N_DEC_RGB, NEED_DEC_RGB, (None,))


@pytest.mark.gpu
def test_decode_streams_beyond_offset_2_32(oracle):
    """Copies of one stream at offset 0, at the first 16-byte aligned offset past 2^32 and at an odd offset past 2^32 of d_streams,
    decoded in one call: felics_decompress_batch_device (the aligned ones), felics_decompress_images_device and
    felics_read_headers_device (all three).  Needs NEED_DEC_FAR = 6.5 GB."""
    import torch
    from felics_amd import synth

    _room(NEED_DEC_FAR)
    img = synth.gray8(200, 96, 4, "S1")
    s = oracle.compress(img)
    far, odd = (1 << 32) + 16, (1 << 32) + 100001
    d = torch.zeros((1 << 32) + (64 << 20), dtype=torch.uint8, device="cuda")
    src = torch.from_numpy(np.frombuffer(s, np.uint8).copy()).cuda()
    for o in (0, far, odd):
        d[o:o + len(s)] = src
    d_img = torch.from_numpy(img).cuda()
    with _fresh_encoder() as e:
        offs, lens = np.array([0, far], np.uint64), np.array([len(s)] * 2, np.uint64)
        px = torch.zeros((2,) + img.shape, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        hdr, status = e.decompress_batch_device(d.data_ptr(), offs, lens, px.data_ptr(), px.numel())
        assert (status == 0).all() and bool((px == d_img).all())
        offs, lens = np.array([far, 0, odd], np.uint64), np.array([len(s)] * 3, np.uint64)
        hdrs, status = e.read_headers_device(d.data_ptr(), offs, lens)
        assert (status == 0).all() and all((h.width, h.height, int(h.color_type), int(h.pixel_depth)) == (200, 96, 0, 0) for h in hdrs)
        px = torch.zeros((3,) + img.shape, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        po, hdrs, status = e.decompress_images_device(d.data_ptr(), offs, lens, px.data_ptr(), px.numel())
        assert (status == 0).all() and [int(o) for o in po] == [0, img.size, 2 * img.size]
        assert bool((px == d_img).all())
    del d, px


FILL = 0xA5


def _decode_images(e, d_streams, offs, lens, imgs):
    """One felics_decompress_images_device call into a buffer of the capacity the library asks for (between the frames' bytes and
    those bytes with every frame rounded up to 16), filled with FILL and 64 bytes longer: (pixels on the device, pix_offsets,
    capacity).  Status, headers, and the placement felics.h promises are checked here: offsets 16-byte aligned, ascending in
    stream order, frames not overlapping and inside the capacity."""
    import torch
    from felics_amd import api

    offs, lens = np.array(offs, np.uint64), np.array(lens, np.uint64)
    with pytest.raises(api.FelicsError) as ei:
        e.decompress_images_device(d_streams.data_ptr(), offs, lens, 0, 0)
    assert ei.value.code == E_BUFFER_TOO_SMALL
    cap = int(str(ei.value).split("need ")[1].split(" bytes")[0])
    sizes = [im.nbytes for im in imgs]
    assert sum(sizes) <= cap <= sum((b + 15) // 16 * 16 for b in sizes)
    px = torch.full((cap + 64,), FILL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    t0 = time.time()
    po, hdrs, status = e.decompress_images_device(d_streams.data_ptr(), offs, lens, px.data_ptr(), cap)
    print("mixed decode n=%d: %.2f s" % (len(imgs), time.time() - t0))
    assert (status == 0).all()
    for h, im in zip(hdrs, imgs):
        assert (int(h.color_type), int(h.pixel_depth), h.width, h.height) == (int(im.ndim == 3), int(im.dtype == np.uint16), im.shape[1], im.shape[0])
    po = [int(o) for o in po]
    assert all(o % 16 == 0 for o in po)
    assert all(po[i + 1] >= po[i] + sizes[i] for i in range(len(po) - 1))
    assert po[-1] + sizes[-1] <= cap
    return px, po, cap


@pytest.mark.gpu
def test_decode_mixed_list_with_pixel_offsets_past_2_32(oracle):
    """felics_decompress_images_device on 520 4K gray8 streams with small gray8 / RGB8 / gray16 streams and a zero-sized image among
    them: 4.31 GB of frames, pix_offsets past 2^32.  Frames equal their sources, offsets ascending and 16-byte aligned, the fill byte
    intact in every gap and in the 64 bytes behind the end (checked on the device).  Needs NEED_DEC_MIXED = 11 GB."""
    import torch

    _room(NEED_DEC_MIXED)
    rng = np.random.default_rng(41)
    big = _base8(W4K, H4K, 1)
    small = [rng.integers(0, 256, size=(37, 51), dtype=np.uint8), rng.integers(0, 256, size=(20, 33, 3), dtype=np.uint8),
             rng.integers(0, 65536, size=(9, 13), dtype=np.uint16), np.zeros((0, 5), np.uint8), rng.integers(0, 256, size=(1, 1), dtype=np.uint8),
             rng.integers(0, 40, size=(129, 65, 3), dtype=np.uint8)]
    distinct = big + small
    d_streams, so, sl = _streams_on_device([oracle.compress(b) for b in distinct])
    which = []
    for i in range(N_DEC_WAVES):
        which.append(i % K)
        if i % 40 == 7:
            which.append(K + (i // 40) % len(small))
    which.append(K + 3)  # (the zero-sized image last as well)
    imgs = [distinct[k] for k in which]
    n = len(which)
    offs, lens = np.array([so[k] for k in which], np.uint64), np.array([sl[k] for k in which], np.uint64)
    dev = {k: torch.from_numpy(distinct[k].view(np.uint8).reshape(-1) if distinct[k].size else np.zeros(0, np.uint8)).cuda() for k in set(which)}
    with _fresh_encoder() as e:
        px, po, cap = _decode_images(e, d_streams, offs, lens, imgs)
        assert cap > 4.3e9 and po[-1] > 1 << 32
        ok = torch.ones((), dtype=torch.bool, device="cuda")
        for i, (o, k) in enumerate(zip(po, which)):
            nb = distinct[k].nbytes
            ok &= (px[o:o + nb] == dev[k]).all()
            end = po[i + 1] if i + 1 < n else cap + 64
            if end > o + nb:  # the gap behind the frame; behind the last one, up to 64 bytes past the capacity
                ok &= (px[o + nb:end] == FILL).all()
            if i % 64 == 63 or i == n - 1:
                assert bool(ok), "a frame or a gap among images %d..%d" % (i - i % 64, i)
    del px


@pytest.mark.gpu
def test_decode_gray16_4k(oracle):
    """300 4K gray16 streams, one wave per stream, one pass of estimator tables (300 x 8.4 MB = 2.5 GB): 4.98 GB of pixels.  The
    width is decoded on the device (decode16_lds_bytes(3840) = 64 KB <= DECODE_LDS_LIMIT, test_size_arithmetic).  32 streams first,
    timed, so that a rate far below the documented 1.7 MPix/s per wave shows before the long call.  Needs NEED_DEC16 = 10 GB."""
    from felics_amd import synth

    rng = np.random.default_rng(16)
    base = [synth.gray16(W4K, H4K, k) for k in range(K)]
    base[1] = (0x7000 + rng.integers(0, 4096, size=(H4K, W4K))).astype(np.uint16)
    base[2] = np.full((H4K, W4K), 0x8000, np.uint16)
    with _fresh_encoder() as e:
        t0 = time.time()
        _decode_repeated(e, oracle, base, 32, NEED_DEC16, (None,))
        t32 = time.time() - t0
        assert t32 * N_DEC16 / 32 < 200, "32 streams took %.1f s: 300 would not fit the test's time limit" % t32
        _decode_repeated(e, oracle, base, N_DEC16, NEED_DEC16, (None,))


# ---- 3. many tiny 8-bit frames -------------------------------------------------------------------------------------------------

def _tiny(planes, n):
    rng = np.random.default_rng(11 + planes)
    shape = (8, 8) if planes == 1 else (8, 8, 3)
    base = [rng.integers(0, 256, size=shape, dtype=np.uint8) for _ in range(TINY_CONTENTS)]
    base[3] = np.full(shape, 77, np.uint8)
    base[5] = (base[5] // 32 + 100).astype(np.uint8)
    return base, [i % TINY_CONTENTS for i in range(n)]


@pytest.mark.gpu
@pytest.mark.parametrize("planes,n", [(1, N_TINY_GRAY), (3, N_TINY_RGB)])
def test_many_tiny_8bit_frames_host(oracle, planes, n):
    """200 000 gray8 / 70 000 RGB8 frames of 8 x 8 (257 contents) through felics_compress_batch: ALL streams equal the oracle's, a
    sample decodes back.  Needs NEED_TINY = 8.0 GB: four lanes with the workspace of a full pass each (the chunks of a host batch are no larger than a pass: at most
    2^23 chains, 1.5 GB)."""
    import felics_amd

    _room(NEED_TINY)
    base, keys = _tiny(planes, n)
    want = [oracle.compress(b) for b in base]
    with _fresh_encoder() as e:
        got = e.compress_batch([base[k] for k in keys])
        assert {k: e.stats()[k] for k in FALLBACKS} == {k: 0 for k in FALLBACKS}
    bad = [i for i in range(n) if got[i] != want[keys[i]]]
    assert not bad, "%d streams differ, the first is %d" % (len(bad), bad[0])
    for i in range(0, n, 4999):
        assert (felics_amd.decompress_image(io.BytesIO(got[i])) == base[keys[i]]).all(), i


@pytest.mark.gpu
@pytest.mark.parametrize("planes,n,passes", [(1, N_TINY_GRAY, TINY_PASSES_GRAY), (3, N_TINY_RGB, TINY_PASSES_RGB)])
def test_many_tiny_8bit_frames_device(oracle, planes, n, passes):
    """The same frames through felics_compress_batch_device: a submission carries at most PASS_MAX_CHAINS = 2^23 chains (plane x
    context; felics_encode.cpp, max_images_per_pass), so `submissions` grows by ceil(n * planes * nctx / 2^23) = 7 (gray) / 13 (RGB), and
    every stream is exact across the pass joins.  Prints the device memory the library holds after the call.
    Needs NEED_TINY = 8.0 GB (one lane's workspace of a full pass is 1.5 GB; the need is stated for four lanes)."""
    import felics_amd
    import torch

    _room(NEED_TINY)
    base, keys = _tiny(planes, n)
    want = {k: oracle.compress(b) for k, b in enumerate(base)}
    d_base = torch.from_numpy(np.stack(base)).cuda()
    frames = d_base[torch.arange(n, device="cuda") % TINY_CONTENTS].contiguous()
    slot = 256 * planes  # (noise does not compress: a stream of 8 x 8 noise is up to ~100 bytes a plane)
    d_out = torch.zeros(n * slot, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    free0, _ = torch.cuda.mem_get_info()
    with _fresh_encoder() as e:
        before = e.stats()
        t0 = time.time()
        offs, lens = e.compress_batch_device(frames.data_ptr(), n, 8, 8, int(planes == 3), 0, d_out.data_ptr(), d_out.numel())
        dt = time.time() - t0
        free1, _ = torch.cuda.mem_get_info()
        print("tiny device planes=%d n=%d: %.2f s, %s, the library holds %.1f MB" % (planes, n, dt, _delta(e, before), (free0 - free1) / 1e6))
        _check_streams(d_out, offs, lens, keys, want, "tiny")
        assert _delta(e, before) == _clean(passes)
    host = d_out.cpu().numpy()
    for i in range(0, n, 4999):
        back = felics_amd.decompress_image(io.BytesIO(host[int(offs[i]):int(offs[i] + lens[i])].tobytes()))
        assert (back == base[keys[i]]).all(), i


@pytest.mark.gpu
def test_forty_thousand_tiny_mixed_images(oracle):
    """40 000 images of w, h in 1..12, half gray8 and half RGB8 (300 contents), in one felics_compress_images call: all images of a
    colour share one tile-count bucket, cut into jobs of at most MIX_MAX_IMAGES = 8192 images and at most one pass (2^23 chains: 5 461
    RGB images): three gray jobs, two of them full, and four RGB jobs, three of them full.
    Every stream equals the oracle's; all 40 000 decode back in ONE felics_decompress_images_device call.
    Needs NEED_TINY_MIXED = 11.9 GB: four lanes with the workspace of a full RGB job (2.4 GB: slots for a whole tile a plane)."""
    import torch

    _room(NEED_TINY_MIXED)
    rng = np.random.default_rng(12)
    base = []
    for c in range(TINY_MIXED_CONTENTS):
        h, w = int(rng.integers(1, 13)), int(rng.integers(1, 13))
        base.append(rng.integers(0, 256, size=(h, w, 3) if c % 2 else (h, w), dtype=np.uint8))
    keys = [int(k) for k in rng.integers(0, TINY_MIXED_CONTENTS // 2, size=N_TINY_MIXED) * 2 + np.arange(N_TINY_MIXED) % 2]
    assert sum(k % 2 for k in keys) == N_TINY_MIXED // 2
    want = [oracle.compress(b) for b in base]
    with _fresh_encoder() as e:
        before = e.stats()
        got = e.compress_images([base[k] for k in keys])
        assert _delta(e, before) == _clean(MIXED_JOBS)
        bad = [i for i in range(N_TINY_MIXED) if got[i] != want[keys[i]]]
        assert not bad, "%d streams differ, the first is %d" % (len(bad), bad[0])
        d_streams, offs, lens = _streams_on_device(got)
        imgs = [base[k] for k in keys]
        px, po, cap = _decode_images(e, d_streams, offs, lens, imgs)
    host = px.cpu().numpy()
    used = np.zeros(len(host), bool)
    for i, (o, b) in enumerate(zip(po, imgs)):
        assert (host[o:o + b.nbytes].reshape(b.shape) == b).all(), i
        used[o:o + b.nbytes] = True
    assert (host[~used] == FILL).all()


@pytest.mark.gpu
def test_two_real_passes_with_an_index(oracle):
    """32 771 gray8 frames of 64 x 65 (2^23 chains are 32 768 of them; K = 2 at 4096 pixels per segment), seven contents in turn, in
    ONE felics_compress_batch_device_indexed call with no test switch: two submissions, the second pass's indexes behind the first's.
    Every stream equals the oracle's stream of its content, every index felics_index_build's of it, 0x5A guards around both intact.
    Holds about 0.6 GB on the device."""
    import torch
    from felics_amd import api
    from tests import index_common as ic

    n, w, h, seg, guard = N_IDX2, W_IDX2, H_IDX2, SEG_IDX2, 256
    base = ic.images(w, h, 0, 4) + [ic.banded(w, h, 0, loud) for loud in ((0,), (1,), ())]
    assert len(base) == K and len({b.tobytes() for b in base}) == K
    streams = [oracle.compress(b) for b in base]
    want = [(np.frombuffer(s, np.uint8), np.frombuffer(api.index_build(s, seg), np.uint8)) for s in streams]
    isize = api.index_size(w, h, 0, 0, seg)
    assert all(len(x) == isize for _, x in want)
    frames = torch.from_numpy(np.stack(base)).cuda()[torch.arange(n, device="cuda") % K].contiguous()
    cap = n * ((w * h * 5 // 4 + 64 + 15) // 16 * 16)
    d_out = torch.full((guard + cap + guard,), 0x5A, dtype=torch.uint8, device="cuda")
    d_idx = torch.full((guard + n * isize + guard,), 0x5A, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    with _fresh_encoder() as e:
        before = e.stats()
        offs, lens = e.compress_batch_device_indexed(frames.data_ptr(), n, w, h, 0, 0, d_out.data_ptr() + guard, cap, seg,
                                                     d_idx.data_ptr() + guard, n * isize)
        assert _delta(e, before) == _clean(2)
    out, idx = d_out.cpu().numpy(), d_idx.cpu().numpy()
    for buf, size in ((out, cap), (idx, n * isize)):
        assert (buf[:guard] == 0x5A).all() and (buf[guard + size:] == 0x5A).all()
    idx = idx[guard:guard + n * isize].reshape(n, isize)
    for i in range(n):
        s, x = want[i % K]
        got = out[guard + int(offs[i]):guard + int(offs[i]) + int(lens[i])]
        assert len(got) == len(s) and (got == s).all(), "stream %d of %d (content %d)" % (i, n, i % K)
        if not (idx[i] == x).all():
            d = int(np.flatnonzero(idx[i] != x)[0])
            pytest.fail("index %d of %d (content %d) differs at byte %d: %s" % (i, n, i % K, d, ic.where_in_index(x.tobytes(), d)))
    del frames, d_out, d_idx


# ---- 4. the stage-by-stage check of the tile-local pipeline ----------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("args", [(), ("big",)], ids=["default", "big"])
def test_tl_check(args):
    """tests/native/tl_check (built by build()): k_front, k_enum, k_spine3 and k_assign3 stage by stage against its CPU model, in a
    process of its own."""
    exe = os.path.join(ROOT, "felics_amd", "_build", "tl_check")
    assert os.path.exists(exe), "felics_amd/_build/tl_check is missing: build() makes it"
    r = subprocess.run([exe, *args], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=400)
    out = r.stdout.decode(errors="replace")
    assert r.returncode == 0, out[-2000:]
    assert "all stages match the CPU model" in out.splitlines()[-1], out[-2000:]
