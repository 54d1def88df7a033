"""Restart index of 16-bit streams on one GPU: felics_decompress_views_device_indexed16 against the calls a caller had before it.

    python profiles/tools/indexed_views16.py [--rounds 7] [--slow-rounds 1] [--part frame,mixed] [--out FILE]

Protocol (that of indexed_views.py).  One process; the forms alternate within a round; one untimed call of each form first
(allocations, code objects).  A time is what two device events around the blocking call(s) measure; the pixels are compared with the
frames after every call; medians and each form's own spread (min .. max) are reported.

frame.  One 3840 x 2160 frame at K = 64 (segment_pixels 4096 x 32), gray16 and RGB16 (synth.gray16; RGB: the same with two chroma
offsets, as indexed_decode16.py has it), encoded with its version-2 index on the GPU.  A round is four calls: the dense indexed call
(felics_decompress_batch_device_indexed16 into a dense frame: existing code, the yardstick), the new call into a PITCHED view (pitch =
width + 64 pixels), the dense call again, and -- in the first --slow-rounds rounds only, it takes seconds -- the unindexed
felics_decompress_views_device into the same view.  The dense call sits in two seats so that the difference of the two seats' medians
says what the protocol cannot tell apart: the MARGIN.  The walk is the same and only the store differs, so the new call is expected
within the margin of the dense one; the tool says whether it is and by how much it is not.

mixed.  16 gray16 frames of four shapes (1920 x 1080, 2560 x 1440, 3200 x 1800, 3840 x 2160; four each) at K = 64, every one into its
own pitched surface.  The new call takes them in ONE call; the only route the parent offers is one dense indexed call per shape plus
a strided device copy per frame into the views.  Both are reported; no ratio is fixed in advance."""
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
    ap.add_argument("--slow-rounds", type=int, default=1)
    ap.add_argument("--part", default="frame,mixed")
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

    class Group:
        """n frames of one shape, encoded with their version-2 indexes on the GPU: streams and indexes where the encoder left them"""

        def __init__(self, n, w, h, rgb):
            self.n, self.w, self.h, self.rgb = n, w, h, rgb
            self.frames = torch.from_numpy(np.stack([frame_of(w, h, f, rgb) for f in range(n)]).view(np.int16)).cuda()
            self.seg = seg_for(w, h)
            self.dense = torch.zeros_like(self.frames)
            torch.cuda.synchronize()
            self.enc = enc.compress_batch_device_indexed16(U16(self.frames), self.seg)
            # every frame's own pitched surface: pitch = width + 64 pixels
            self.surf = [torch.zeros((h, w + 64, 3) if rgb else (h, w + 64), dtype=torch.int16, device="cuda") for _ in range(n)]
            self.views = [s[:, :w] for s in self.surf]

        def dense_call(self):
            e = self.enc
            self.dense.zero_()
            t = timed(lambda: enc.decompress_batch_device_indexed16(e.streams.data_ptr(), e.offsets, e.lens, e.index.data_ptr(), e.idx_offsets,
                                                                    e.idx_lens, self.dense.data_ptr(), self.dense.numel() * 2))
            assert torch.equal(self.dense, self.frames)
            return t

        def check_views(self):
            for v, f, s in zip(self.views, self.frames, self.surf):
                assert torch.equal(v, f) and not s[:, self.w:].any()

        def clear_views(self):
            for s in self.surf:
                s.zero_()

    def views_indexed(groups):
        """the new call over all frames of all groups, in one call (addresses relative to the lowest buffer; the encoder's buffers are
        64-byte aligned, so every index address is)"""
        base_s = min(g.enc.streams.data_ptr() for g in groups)
        base_i = min(g.enc.index.data_ptr() for g in groups)
        offs, lens, ioffs, ilens, views = [], [], [], [], []
        for g in groups:
            for k in range(g.n):
                offs.append(g.enc.streams.data_ptr() - base_s + int(g.enc.offsets[k]))
                lens.append(int(g.enc.lens[k]))
                ioffs.append(g.enc.index.data_ptr() - base_i + int(g.enc.idx_offsets[k]))
                ilens.append(int(g.enc.idx_lens[k]))
                views.append(api.view_of_array(U16(g.views[k])))
            g.clear_views()
        t = timed(lambda: enc.decompress_views_device_indexed16(base_s, offs, lens, base_i, ioffs, ilens, views))
        for g in groups:
            g.check_views()
        return t

    say("indexed_views16.py: source %s, device %s, %d rounds" % (build.source_hash(), torch.cuda.get_device_name(0), a.rounds))
    if "frame" in a.part:
        for rgb in (0, 1):
            g = Group(1, 3840, 2160, rgb)
            say("one %s 3840 x 2160 frame, K = %d, stream %.2f MB, index %.2f MB, pitched view (pitch %d pixels)"
                % ("RGB16" if rgb else "gray16", (3840 * 2160 + g.seg - 1) // g.seg, int(g.enc.lens[0]) / 1e6, int(g.enc.idx_lens[0]) / 1e6, 3840 + 64))
            view = [api.view_of_array(U16(g.views[0]))]

            def unindexed():
                g.clear_views()
                t = timed(lambda: enc.decompress_views_device(g.enc.streams.data_ptr(), g.enc.offsets, g.enc.lens, view))
                g.check_views()
                return t

            g.dense_call()
            views_indexed([g])
            seat_a, seat_b, seat_c, slow = [], [], [], []
            for r in range(a.rounds):
                seat_a.append(g.dense_call())
                seat_b.append(views_indexed([g]))
                seat_c.append(g.dense_call())
                if r < a.slow_rounds:
                    slow.append(unindexed())
            dense = statistics.median(seat_a + seat_c)
            margin = abs(statistics.median(seat_a) - statistics.median(seat_c))
            new = statistics.median(seat_b)
            say("  dense indexed call, seat 1         : %s" % stat(seat_a))
            say("  dense indexed call, seat 2         : %s" % stat(seat_c))
            say("  indexed into the pitched view      : %s" % stat(seat_b))
            if slow:
                say("  unindexed into the pitched view    : %s  (%.1fx the indexed call)" % (stat(slow), statistics.median(slow) / new))
            say("  margin %.3f ms; the new call is %+.3f ms (%+.1f %%) off the dense call: %s"
                % (margin, new - dense, 100 * (new - dense) / dense, "WITHIN the margin" if abs(new - dense) <= margin else "OUTSIDE the margin"))
            del g
            torch.cuda.empty_cache()
    if "mixed" in a.part:
        shapes = [(1920, 1080), (2560, 1440), (3200, 1800), (3840, 2160)]
        groups = [Group(4, w, h, 0) for w, h in shapes]
        say("16 gray16 frames of four shapes (%s), K = 64 each, every frame into its own pitched surface"
            % ", ".join("%d x %d" % s for s in shapes))

        def parent_route():
            for g in groups:
                g.clear_views()
                g.dense.zero_()

            def run():
                for g in groups:
                    e = g.enc
                    enc.decompress_batch_device_indexed16(e.streams.data_ptr(), e.offsets, e.lens, e.index.data_ptr(), e.idx_offsets, e.idx_lens,
                                                          g.dense.data_ptr(), g.dense.numel() * 2)
                    for k in range(g.n):
                        g.views[k].copy_(g.dense[k])

            t = timed(run)
            for g in groups:
                g.check_views()
            return t

        parent_route()
        views_indexed(groups)
        old, new = [], []
        for _ in range(a.rounds):
            old.append(parent_route())
            new.append(views_indexed(groups))
        say("  one dense indexed call per shape + a strided copy per frame : %s" % stat(old))
        say("  one indexed views call                                      : %s" % stat(new))
        mpix = sum(g.n * g.w * g.h for g in groups) / 1e3
        say("  %.1f MPix: %.1f against %.1f MPix/s, the one call takes %.2fx the parent route's time"
            % (mpix / 1e3, mpix / statistics.median(old), mpix / statistics.median(new), statistics.median(new) / statistics.median(old)))
        say("  felics_index16_view_stats so far: %s" % enc.index16_view_stats())
    enc.close()


if __name__ == "__main__":
    main()
