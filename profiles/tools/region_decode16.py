"""Regions of 16-bit streams through the version-2 restart index on one GPU: what a window costs against the whole frame.

    python profiles/tools/region_decode16.py [--reps 5] [--out FILE]

Workloads: one 3840 x 2160 gray16 frame (synth.gray16), 16 of them, one RGB16 frame (the same with two chroma offsets), each at
segment_pixels = 4096 (K = 2025) and 4096 x 32 (K = 64), streams and indexes written by felics_compress_batch_device_indexed16.
Forms, alternating in one process, --reps rounds of
    full (seat A) | 256 x 256 window | full (seat B) | 1024 x 1024 window
after one untimed call of each: `full` is felics_decompress_batch_device_indexed16 of the same buffers, a window is
felics_decompress_regions_device_indexed16 with one request per stream, the window in the middle of the frame.  The full call sits
in two seats of the round: the difference of their medians is the run's own spread, and the margin a window's time is judged by.  A
time is what two device events around the blocking call measure, reported as median (min .. max).  Pixels are compared after every
call: the frames, or the windows of the frames."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
W, H = 3840, 2160
SEGS = (4096, 4096 * 32)
WINDOWS = (256, 1024)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
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

    def timed(fn):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0.record()
        fn()
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1)

    def fmt(ts):
        return "%9.2f ms (%.2f .. %.2f, %d calls)" % (statistics.median(ts), min(ts), max(ts), len(ts))

    def frame_of(f, rgb):
        g = synth.gray16(W, H, f)
        if not rgb:
            return g
        r = np.clip(g.astype(np.int64) + (g & 3) * 16 - 24, 0, 65535)
        b = np.clip(g.astype(np.int64) - ((g >> 2) & 3) * 16 + 24, 0, 65535)
        return np.stack([r, g, b], -1).astype(np.uint16)

    say("region_decode16.py: source %s, device %s, %d rounds" % (build.source_hash(), torch.cuda.get_device_name(0), a.reps))
    worst = None
    for name, n, rgb in (("1 gray16 4K frame", 1, 0), ("16 gray16 4K frames", 16, 0), ("1 RGB16 4K frame", 1, 1)):
        planes = 3 if rgb else 1
        frames = torch.from_numpy(np.stack([frame_of(f, rgb) for f in range(n)]).view(np.int16)).cuda()  # (torch compares int16; the bits are the samples')
        cap = n * ((frames[0].numel() * 2 * 5 // 4 + 64 + 15) // 16 * 16)
        d_out = torch.empty(cap, dtype=torch.uint8, device="cuda")
        d_px = torch.zeros_like(frames)
        for seg in SEGS:
            k = (W * H + seg - 1) // seg
            icap = 64
            for _ in range(2):  # the two-call pattern: the second call has idx_total bytes
                d_idx = torch.empty(icap, dtype=torch.uint8, device="cuda")
                torch.cuda.synchronize()
                rc, offs, lens, ioffs, ilens, icap = enc.compress_batch_device_indexed16_raw(frames.data_ptr(), n, W, H, rgb, d_out.data_ptr(), cap, seg,
                                                                                             d_idx.data_ptr(), icap)
                if rc == 0:
                    break
            assert rc == 0 and d_idx.data_ptr() % 64 == 0, rc
            say("%s, segment %d px (K = %d), indexes %.1f MB" % (name, seg, k, sum(int(x) for x in ilens) / 1e6))

            def full():
                d_px.zero_()
                t = timed(lambda: enc.decompress_batch_device_indexed16(d_out.data_ptr(), offs, lens, d_idx.data_ptr(), ioffs, ilens, d_px.data_ptr(),
                                                                        d_px.numel() * 2))
                assert torch.equal(d_px, frames)
                return t

            def window(side):
                x, y = (W - side) // 2, (H - side) // 2
                crop = side * side * planes
                d_crops = torch.zeros(n * crop, dtype=torch.int16, device="cuda")
                reqs = [(i, x, y, side, side) for i in range(n)]
                t = timed(lambda: enc.decompress_regions_device_indexed16(d_out.data_ptr(), offs, lens, d_idx.data_ptr(), ioffs, ilens, reqs,
                                                                           d_crops.data_ptr(), d_crops.numel() * 2))
                want = frames[:, y:y + side, x:x + side].reshape(n, -1)
                assert torch.equal(d_crops.view(n, crop), want)
                return t

            full()
            for side in WINDOWS:
                window(side)
            ts = {"A": [], "B": [], 256: [], 1024: []}
            stats = {}
            for _ in range(a.reps):
                ts["A"].append(full())
                for side, seat in ((256, "B"), (1024, None)):
                    before = enc.region16_stats()
                    ts[side].append(window(side))
                    after = enc.region16_stats()
                    stats[side] = {key: after[key] - before[key] for key in after}
                    if seat:
                        ts[seat].append(full())
            ma, mb = statistics.median(ts["A"]), statistics.median(ts["B"])
            spread = abs(ma - mb)
            say("  full frame(s), seat A                 : %s" % fmt(ts["A"]))
            say("  full frame(s), seat B                 : %s   spread of the two medians %.3f ms (%.2f %%)" % (fmt(ts["B"]), spread, 100 * spread / min(ma, mb)))
            for side in WINDOWS:
                m = statistics.median(ts[side])
                share = len(api.region_segments(W, H, seg, (W - side) // 2, (H - side) // 2, side, side)) / k
                over = m - (max(ma, mb) + spread)
                say("  %4d x %4d window per frame           : %s   %.3f of the full call, segments walked / (C K) = %.3f, rows loaded %d   %s"
                    % (side, side, fmt(ts[side]), m / min(ma, mb), share, stats[side]["rows_loaded"],
                       "within the margin" if over <= 0 else "SLOWER than full + spread by %.3f ms" % over))
                say("      counters of one call: %s" % stats[side])
                if worst is None or over > worst[0]:
                    worst = (over, name, seg, side)
            del d_idx
            torch.cuda.empty_cache()
        del frames, d_out, d_px
        torch.cuda.empty_cache()
    say("acceptance (no window call slower than the full call by more than the spread): %s"
        % ("met" if worst[0] <= 0 else "MISSED: %s, segment %d, %d x %d window, by %.3f ms" % (worst[1], worst[2], worst[3], worst[3], worst[0])))
    enc.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
