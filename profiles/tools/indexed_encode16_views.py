"""Restart index of 16-bit streams, written while encoding views and mixed shapes: felics_compress_views_device_indexed16 against what
a caller had before it, on one GPU.

    python profiles/tools/indexed_encode16_views.py [--rounds 7] [--part gray,rgb] [--out FILE]

Protocol (that of indexed_views16.py).  One process; the forms alternate within a round; one untimed call of each form first
(allocations, code objects, the index buffer sized by the two-call pattern).  A time is what two device events around the blocking
call(s) measure; medians and each form's own spread (min .. max) are reported.  After EVERY timed call the streams and the indexes are
compared on the device: the streams with those of felics_compress_views_device, the indexes with those of
felics_compress_batch_device_indexed16 on the gathered frames (which the test suite holds to the host builder byte for byte).

gray.  The 16 gray16 frames of indexed_views16.py's mixed part -- four shapes (1920 x 1080, 2560 x 1440, 3200 x 1800, 3840 x 2160; four
each), synth.gray16 -- each in its own pitched surface (pitch = width + 64 pixels), K = 64 per frame.  Three forms:
    views            felics_compress_views_device on the 16 views: the same streams, no index.  new - views = what the index costs.
    per shape        what a caller did before: per shape a strided copy of its four surfaces into a dense batch, then one
                     felics_compress_batch_device_indexed16 call -- four gathers and four calls.
    views indexed    the new call: the 16 views in ONE call.
rgb.  The same three forms on 4 RGB16 frames of two shapes (1920 x 1080, 2560 x 1440; two each)."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
GRANULE = 4096


class U16:
    """uint16 samples held in an int16 tensor (not every torch build has a uint16 dtype on the device), as the library sees them"""

    def __init__(self, t):
        self.__cuda_array_interface__ = {"shape": tuple(t.shape), "typestr": "<u2", "data": (t.data_ptr(), False), "version": 2,
                                         "strides": tuple(2 * v for v in t.stride())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--part", default="gray,rgb")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import numpy as np
    import torch

    import felics_amd
    from felics_amd import api, build, synth

    enc = felics_amd.Encoder(0)
    lines = []

    def say(s):
        lines.append(s)
        print(s, flush=True)
        if a.out:  # (kept up to date: a run that is cut short leaves what it measured)
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    def timed(fn):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0.record()
        fn()
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1)

    def stat(ts):
        return "%9.2f ms (%.2f .. %.2f, %d calls)" % (statistics.median(ts), min(ts), max(ts), len(ts))

    def seg_for(w, h, k=64):
        return ((w * h + k - 1) // k + GRANULE - 1) // GRANULE * GRANULE

    def frame_of(w, h, f, rgb):
        g = synth.gray16(w, h, f)
        if not rgb:
            return g
        r = np.clip(g.astype(np.int64) + (g & 3) * 16 - 24, 0, 65535)
        b = np.clip(g.astype(np.int64) - ((g >> 2) & 3) * 16 + 24, 0, 65535)
        return np.stack([r, g, b], -1).astype(np.uint16)

    def alloc(nbytes):
        return torch.zeros(max(int(nbytes), 64), dtype=torch.uint8, device="cuda")

    def part(name, shapes, per_shape, rgb):
        c = 3 if rgb else 1
        surfs, views, segs, groups = [], [], [], []
        for w, h in shapes:
            first = len(surfs)
            for f in range(per_shape):
                s = torch.zeros((h, w + 64, 3) if rgb else (h, w + 64), dtype=torch.int16, device="cuda")
                s[:, :w] = torch.from_numpy(frame_of(w, h, f, rgb).view(np.int16)).cuda()
                surfs.append(s)
                views.append(api.view_of_array(U16(s[:, :w])))
                segs.append(seg_for(w, h))
            groups.append((w, h, first, torch.zeros((per_shape, h, w, 3) if rgb else (per_shape, h, w), dtype=torch.int16, device="cuda")))
        n = len(views)
        out_cap = sum(w * h * 2 * c * 5 // 4 + 96 for (w, h) in shapes) * per_shape + 4096
        mpix = sum(w * h for w, h in shapes) * per_shape / 1e6
        say("%s: %d %s frames of %d shapes (%s), K = 64 each, every frame in its own pitched surface (pitch = width + 64 pixels), %.1f MPix"
            % (name, n, "RGB16" if rgb else "gray16", len(shapes), ", ".join("%d x %d" % s for s in shapes), mpix))

        # the references, untimed: the streams of the plain views call, the indexes of the per-shape route
        ref_out = alloc(out_cap)
        torch.cuda.synchronize()
        ref_offs, ref_lens = enc.compress_views_device(views, ref_out.data_ptr(), out_cap)
        ref_streams = [ref_out[int(o):int(o) + int(ln)].clone() for o, ln in zip(ref_offs, ref_lens)]

        def per_shape_route(state):
            """state: per group its (streams buffer, index buffer, index capacity); the result per group for the comparison"""
            res = []
            for (w, h, first, dense), st in zip(groups, state):
                for k in range(per_shape):
                    dense[k].copy_(surfs[first + k][:, :w])
                res.append(enc.compress_batch_device_indexed16_raw(dense.data_ptr(), per_shape, w, h, rgb, st[0].data_ptr(), st[0].numel(),
                                                                   segs[first], st[1].data_ptr(), st[2]))
            return res

        # size the per-shape route's index buffers by its two-call pattern, then take its indexes as the reference
        state = [[alloc(per_shape * (w * h * 2 * c * 5 // 4 + 96)), alloc(64), 0] for w, h in shapes]
        for st, r in zip(state, per_shape_route(state)):
            assert r[0] == -8 and r[5] > 0
            st[1], st[2] = alloc(r[5]), r[5]
        torch.cuda.synchronize()
        ref_idx = []
        for (w, h, first, _), st, r in zip(groups, state, per_shape_route(state)):
            assert r[0] == 0
            for k in range(per_shape):
                ref_idx.append(st[1][int(r[3][k]):int(r[3][k]) + int(r[4][k])].clone())
                assert torch.equal(st[0][int(r[1][k]):int(r[1][k]) + int(r[2][k])], ref_streams[first + k])
        need = sum(x.numel() for x in ref_idx)

        new_out, new_idx = alloc(out_cap), alloc(need)
        plain_out = alloc(out_cap)
        torch.cuda.synchronize()

        def check_new(r):
            rc, offs, lens, ioffs, ilens, total = r
            assert rc == 0 and total == need, (rc, total, need)
            for i in range(n):
                assert torch.equal(new_out[int(offs[i]):int(offs[i]) + int(lens[i])], ref_streams[i]), i
                assert torch.equal(new_idx[int(ioffs[i]):int(ioffs[i]) + int(ilens[i])], ref_idx[i]), i

        def run_new():
            new_idx.fill_(0x5A)
            box = []
            t = timed(lambda: box.append(enc.compress_views_device_indexed16_raw(views, segs, new_out.data_ptr(), out_cap, new_idx.data_ptr(), need)))
            check_new(box[0])
            return t

        def run_plain():
            box = []
            t = timed(lambda: box.append(enc.compress_views_device(views, plain_out.data_ptr(), out_cap)))
            for i, (o, ln) in enumerate(zip(*box[0])):
                assert torch.equal(plain_out[int(o):int(o) + int(ln)], ref_streams[i]), i
            return t

        def run_per_shape():
            box = []
            t = timed(lambda: box.append(per_shape_route(state)))
            i = 0
            for (w, h, first, _), st, r in zip(groups, state, box[0]):
                assert r[0] == 0
                for k in range(per_shape):
                    assert torch.equal(st[0][int(r[1][k]):int(r[1][k]) + int(r[2][k])], ref_streams[i])
                    assert torch.equal(st[1][int(r[3][k]):int(r[3][k]) + int(r[4][k])], ref_idx[i])
                    i += 1
            return t

        before = enc.index16_view_emit_stats()
        run_plain(), run_per_shape(), run_new()
        plain, old, new = [], [], []
        for _ in range(a.rounds):
            plain.append(run_plain())
            old.append(run_per_shape())
            new.append(run_new())
        after = enc.index16_view_emit_stats()
        say("  streams %.2f MB, indexes %.2f MB (%d state rows per call)"
            % (sum(int(x) for x in ref_lens) / 1e6, need / 1e6, (after["rows_written"] - before["rows_written"]) // (a.rounds + 1)))
        say("  views call, no index (a)                       : %s" % stat(plain))
        say("  a gather and one indexed batch call per shape (b): %s" % stat(old))
        say("  one indexed views call                         : %s" % stat(new))
        mp, mo, mn = statistics.median(plain), statistics.median(old), statistics.median(new)
        say("  the index costs %+.2f ms per call, %+.3f ms per frame (%+.1f %% of the views call); the one call takes %.2fx the per-shape route's time"
            % (mn - mp, (mn - mp) / n, 100 * (mn - mp) / mp, mn / mo))
        say("  %.1f / %.1f / %.1f MPix/s (a / b / new); every timed call's streams and indexes compared on the device: equal" % (
            mpix * 1e3 / mp, mpix * 1e3 / mo, mpix * 1e3 / mn))
        say("  felics_index16_view_emit_stats of the part: %s" % {k: after[k] - before[k] if k != "shapes_max" else after[k] for k in after})

    say("indexed_encode16_views.py: source %s, device %s, %d rounds" % (build.source_hash(), torch.cuda.get_device_name(0), a.rounds))
    if "gray" in a.part:
        part("gray", [(1920, 1080), (2560, 1440), (3200, 1800), (3840, 2160)], 4, 0)
        torch.cuda.empty_cache()
    if "rgb" in a.part:
        part("rgb", [(1920, 1080), (2560, 1440)], 2, 1)
    enc.close()


if __name__ == "__main__":
    main()
