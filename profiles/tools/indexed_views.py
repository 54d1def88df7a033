"""Restart index on one GPU: felics_decompress_views_device_indexed against the calls a caller had before it.

    python profiles/tools/indexed_views.py [--rounds 7] [--slow-rounds 2] [--part frame,mixed] [--out FILE]

Protocol.  One process; the forms alternate within a round; one untimed call of each form first (allocations, code objects).  A
time is what two device events around the blocking call(s) measure; the pixels are compared with the frames after every call;
medians and each form's own spread (min .. max) are reported.

frame.  One 3840 x 2160 frame at K = 64 (segment_pixels 4096 x 32), gray8 and RGB8, S1 content.  A round is four calls: the dense
indexed call (felics_decompress_batch_device_indexed into a dense frame: existing code, the yardstick), the new call into a PITCHED
view (pitch = width + 64 pixels), the dense call again, and -- in the first --slow-rounds rounds only, it takes seconds -- the unindexed
felics_decompress_views_device into the same view.  The dense call sits in two seats so that the difference of the two seats'
medians says what the protocol cannot tell apart: the MARGIN.  The walk is the same and only the store differs, so the new call is
expected within the margin of the dense one; the tool says whether it is and by how much it is not.

mixed.  16 gray8 frames of four shapes (1920 x 1080, 2560 x 1440, 3200 x 1800, 3840 x 2160; four each) at K = 64, every one into its
own pitched surface.  The new call takes them in ONE call; the only route the parent offers is one dense indexed call per shape
plus a strided device copy per frame into the views.  Both are reported; no ratio is fixed in advance."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
GRANULE = 4096


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--slow-rounds", type=int, default=2)
    ap.add_argument("--part", default="frame,mixed")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch

    import felics_amd
    from felics_amd import api, build, synth_torch

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

    class Group:
        """n frames of one shape, encoded with their indexes on the GPU: streams and indexes where the encoder left them"""

        def __init__(self, n, w, h, rgb):
            self.n, self.w, self.h, self.rgb = n, w, h, rgb
            self.frames = torch.stack([synth_torch.rgb8(w, h, f) if rgb else synth_torch.gray8(w, h, f, "S1") for f in range(n)]).cuda()
            self.seg = seg_for(w, h)
            self.isize = api.index_size(w, h, rgb, 0, self.seg)
            cap = n * ((self.frames[0].numel() * 5 // 4 + 64 + 15) // 16 * 16)
            self.d_out = torch.empty(cap, dtype=torch.uint8, device="cuda")
            self.d_idx = torch.empty(n * self.isize, dtype=torch.uint8, device="cuda")
            self.dense = torch.zeros_like(self.frames)
            torch.cuda.synchronize()
            self.offs, self.lens = enc.compress_batch_device_indexed(self.frames.data_ptr(), n, w, h, rgb, 0, self.d_out.data_ptr(), cap, self.seg,
                                                                     self.d_idx.data_ptr(), n * self.isize)
            # every frame's own pitched surface: pitch = width + 64 pixels
            self.surf = [torch.zeros((h, w + 64, 3) if rgb else (h, w + 64), dtype=torch.uint8, device="cuda") for _ in range(n)]
            self.views = [s[:, :w] for s in self.surf]

        def dense_call(self):
            self.dense.zero_()
            t = timed(lambda: enc.decompress_batch_device_indexed(self.d_out.data_ptr(), self.offs, self.lens, self.d_idx.data_ptr(), self.isize,
                                                                  self.dense.data_ptr(), self.dense.numel()))
            assert torch.equal(self.dense, self.frames)
            return t

        def check_views(self):
            for v, f, s in zip(self.views, self.frames, self.surf):
                assert torch.equal(v, f) and not s[:, self.w:].any()

        def clear_views(self):
            for s in self.surf:
                s.zero_()

    def views_indexed(groups):
        """the new call over all frames of all groups, in one call (addresses relative to the lowest buffer)"""
        base_s = min(g.d_out.data_ptr() for g in groups)
        base_i = min(g.d_idx.data_ptr() for g in groups)
        offs, lens, ioffs, ilens, views = [], [], [], [], []
        for g in groups:
            for k in range(g.n):
                offs.append(g.d_out.data_ptr() - base_s + int(g.offs[k]))
                lens.append(int(g.lens[k]))
                ioffs.append(g.d_idx.data_ptr() - base_i + k * g.isize)
                ilens.append(g.isize)
                views.append(api.view_of_array(g.views[k]))
            g.clear_views()
        t = timed(lambda: enc.decompress_views_device_indexed(base_s, offs, lens, base_i, ioffs, ilens, views))
        for g in groups:
            g.check_views()
        return t

    say("indexed_views.py: source %s, device %s, %d rounds" % (build.source_hash(), torch.cuda.get_device_name(0), a.rounds))
    if "frame" in a.part:
        for rgb in (0, 1):
            g = Group(1, 3840, 2160, rgb)
            say("one %s 3840 x 2160 S1 frame, K = %d, stream %.2f MB, index %.2f MB, pitched view (pitch %d pixels)"
                % ("RGB8" if rgb else "gray8", (3840 * 2160 + g.seg - 1) // g.seg, int(g.lens[0]) / 1e6, g.isize / 1e6, 3840 + 64))
            view = [api.view_of_array(g.views[0])]

            def unindexed():
                g.clear_views()
                t = timed(lambda: enc.decompress_views_device(g.d_out.data_ptr(), g.offs, g.lens, view))
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
        say("16 gray8 S1 frames of four shapes (%s), K = 64 each, every frame into its own pitched surface"
            % ", ".join("%d x %d" % s for s in shapes))

        def parent_route():
            for g in groups:
                g.clear_views()
                g.dense.zero_()

            def run():
                for g in groups:
                    enc.decompress_batch_device_indexed(g.d_out.data_ptr(), g.offs, g.lens, g.d_idx.data_ptr(), g.isize, g.dense.data_ptr(), g.dense.numel())
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
        st = enc.index_view_stats()
        say("  felics_index_view_stats so far: %s" % st)
    enc.close()


if __name__ == "__main__":
    main()
