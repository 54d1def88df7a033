"""The encode and decode paths under a cap on the hardware queues (GPU_MAX_HW_QUEUES).

The HIP runtime pools hardware queues per stream priority, each pool capped by GPU_MAX_HW_QUEUES (4 by default); streams beyond
the cap share an in-order queue.  The library's stage graph fits the default with two lanes (felics_ctx_create), and with four
lanes its streams still fit; whatever shares a queue may only ever cost time, never order.  So every case runs at a cap of 4 and
at a cap of 8, through 2 lanes and through 4, in a child process of its own (the runtime reads the cap when it starts), with
FELICS_POISON set, and is byte-compared with the CPU oracle.  The single-pass pack's look-back assumes that a tile's
predecessors run: no case may need a remedy (felics_stats: no look-back fallback, no ticket retry, no batch redone).

No timing is asserted here: the times are in profiles/hw_queues.txt."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ("gray8", "rgb8", "gray16", "host", "mixed", "decode")
CHILD_TIMEOUT_S = 420  # (the first `import torch` of a process on a fresh box can take minutes)
CLEAN = {"ticket_retries": 0, "slot_overflows": 0, "lookback_fallbacks": 0, "two_pass": 0, "failed": 0, "scatter_fallbacks": 0,
         "tile_overflows": 0}


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("lanes", (2, 4))
@pytest.mark.parametrize("cap", (4, 8))
def test_streams_equal_the_oracle_under_the_cap(cap, lanes, case):
    env = dict(os.environ, GPU_MAX_HW_QUEUES=str(cap), FELICS_LANES=str(lanes), FELICS_POISON="1")
    r = subprocess.run([sys.executable, "-s", os.path.abspath(__file__), case, str(cap), str(lanes)], env=env, cwd=ROOT,
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=CHILD_TIMEOUT_S)
    out = r.stdout.decode(errors="replace")
    assert r.returncode == 0, out[-3000:]
    assert out.strip().splitlines()[-1].startswith("ok %s cap=%d lanes=%d" % (case, cap, lanes)), out[-3000:]


# ---- the child --------------------------------------------------------------------------------------------------------------

def _frames(kind, w, h, n, seed):
    from felics_amd import synth

    if kind == "gray8":
        return [synth.gray8(w, h, seed + i, "S1") for i in range(n)]
    if kind == "rgb8":
        return [synth.rgb8(w, h, seed + i) for i in range(n)]
    return [synth.gray16(w, h, seed + i) for i in range(n)]


def _queued(enc, oracle, kind, lanes):
    """3 * lanes + 1 submissions of three different batches, `lanes` of them in flight, each into a buffer of its own."""
    import torch

    w, h, n = 1000, 562, 5  # (five frames of 1000 x 562: several sort tiles per plane, a last tile that is not full)
    color, depth = int(kind == "rgb8"), int(kind == "gray16")
    batches = [_frames(kind, w, h, n, 100 * b) for b in range(3)]
    want = [[oracle.compress(im) for im in b] for b in batches]
    dev = [torch.from_numpy(np.stack(b)).cuda() for b in batches]
    cap = n * (dev[0][0].numel() * dev[0].element_size() * 3 // 2 + 4096)
    nsub = 3 * lanes + 1
    outs = [torch.full((cap,), 0xA5, dtype=torch.uint8, device="cuda") for _ in range(nsub)]
    torch.cuda.synchronize()
    assert enc.lane_count() == lanes
    flying, done = [], []
    for i in range(nsub):
        if len(flying) == lanes:
            j, sub = flying.pop(0)
            done.append((j,) + enc.wait_batch(sub))
        flying.append((i, enc.submit_batch_device(dev[i % 3].data_ptr(), n, w, h, color, depth, outs[i].data_ptr(), cap)))
    for j, sub in flying:
        done.append((j,) + enc.wait_batch(sub))
    torch.cuda.synchronize()
    assert [d[0] for d in done] == list(range(nsub))
    for j, offs, lens in done:
        host = outs[j].cpu().numpy()
        for k in range(n):
            got = host[int(offs[k]): int(offs[k]) + int(lens[k])].tobytes()
            assert got == want[j % 3][k], "%s submission %d frame %d: %d vs %d bytes" % (kind, j, k, len(got), len(want[j % 3][k]))
    return nsub * n


def _host(enc, oracle):
    """The host-buffer entry point (felics_compress_batch): chunks through the submission queue, two copy streams beside the lanes."""
    total = 0
    for kind, w, h, n in (("gray8", 1000, 562, 24), ("rgb8", 640, 360, 12), ("gray16", 640, 360, 6)):
        imgs = _frames(kind, w, h, n, 7)
        got = enc.compress_batch(imgs)
        for k, (g, im) in enumerate(zip(got, imgs)):
            assert g == oracle.compress(im), (kind, k)
        total += n
    return total


def _mixed_images():
    rng = np.random.default_rng(11)
    imgs = _frames("gray8", 1000, 562, 3, 1) + _frames("rgb8", 640, 360, 2, 2) + _frames("gray16", 320, 180, 2, 3)
    for hh, ww in ((1, 1), (3, 700), (700, 3), (257, 255), (64, 64), (129, 513)):
        imgs.append(rng.integers(100, 132, size=(hh, ww), dtype=np.uint8))  # (five bits of noise: no stream outgrows its slot)
        imgs.append(rng.integers(100, 132, size=(hh, ww, 3), dtype=np.uint8))
    imgs.append(rng.integers(1000, 3048, size=(33, 65, 3), dtype=np.uint16))
    return [imgs[i] for i in rng.permutation(len(imgs))]


def _mixed(enc, oracle):
    imgs = _mixed_images()
    got = enc.compress_images(imgs)
    for k, (g, im) in enumerate(zip(got, imgs)):
        assert g == oracle.compress(im), (k, im.shape, im.dtype)
    return len(imgs)


def _decode(enc, oracle):
    """One mixed-shape decode call (its launches go to the lanes' streams) of the oracle's streams."""
    import torch

    imgs = _mixed_images()
    streams = [oracle.compress(im) for im in imgs]
    offs, blob = [], bytearray()
    for s in streams:
        offs.append(len(blob))
        blob += s
    d = torch.from_numpy(np.frombuffer(bytes(blob) + bytes(16), dtype=np.uint8).copy()).cuda()
    cap = sum((im.nbytes + 15) // 16 * 16 for im in imgs) + 64
    px = torch.full((cap,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    po, _, st = enc.decompress_images_device(d.data_ptr(), offs, [len(s) for s in streams], px.data_ptr(), cap)
    assert (st == 0).all(), st
    host = px.cpu().numpy()
    for k, (o, im) in enumerate(zip(po, imgs)):
        back = host[int(o): int(o) + im.nbytes].view(im.dtype).reshape(im.shape)
        assert (back == im).all(), (k, im.shape, im.dtype)
    return len(imgs)


def _child(case, cap, lanes):
    assert os.environ.get("GPU_MAX_HW_QUEUES") == str(cap) and os.environ.get("FELICS_LANES") == str(lanes)
    assert os.environ.get("FELICS_POISON")
    if ROOT not in sys.path:
        sys.path.insert(0, ROOT)
    import felics_amd
    from tests import oracle_lib

    oracle = oracle_lib.load()
    with felics_amd.Encoder(0) as enc:
        assert os.environ.get("GPU_MAX_HW_QUEUES") == str(cap)  # (nothing on the way replaced the caller's value)
        if case in ("gray8", "rgb8", "gray16"):
            n = _queued(enc, oracle, case, lanes)
        else:
            n = {"host": _host, "mixed": _mixed, "decode": _decode}[case](enc, oracle)
        st = enc.stats()
        bad = {k: st[k] for k, v in CLEAN.items() if st[k] != v}
        assert not bad, "a remedy was needed: %s" % bad
    print("ok %s cap=%d lanes=%d (%d images, stats %s)" % (case, cap, lanes, n, st))


if __name__ == "__main__":
    _child(sys.argv[1], int(sys.argv[2]), int(sys.argv[3]))
