"""Restart index on one GPU: what it buys the decoder and what it costs the encoder.

    python profiles/tools/indexed_decode.py [--rounds 3] [--fast-per-round 4] [--out FILE] [--part decode,encode] [--encode-reps 12]

1. Decode.  Workloads: one 3840 x 2160 gray8 S1 frame, 64 of them, one 3840 x 2160 RGB8 frame.  felics_decompress_batch_device (a
   wave per stream) against felics_decompress_batch_device_indexed at segment_pixels = 4096 x {1, 8, 32, 128}, the indexes written
   by felics_compress_batch_device_indexed.  One untimed call of every form first; then --rounds rounds, each one unindexed call
   (seconds) followed by --fast-per-round calls of every indexed setting, so the forms alternate in one process and an indexed
   setting is timed rounds x fast-per-round >= 10 times.  A time is what two device events around the blocking call measure,
   reported as median (min .. max).  Pixels are compared with the frames after every call.
2. Encode.  64 3840 x 2160 gray8 S1 frames per blocking call: felics_compress_batch_device against
   felics_compress_batch_device_indexed at K = 64 (segment_pixels = 4096 x 32), alternating, --encode-reps calls each after one
   untimed call each.  (The emit kernels' own time comes from a kernel trace of `--part encode`: the job that ran this says so.)"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
W, H = 3840, 2160
SEGS = (4096, 4096 * 8, 4096 * 32, 4096 * 128)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--fast-per-round", type=int, default=4)
    ap.add_argument("--encode-reps", type=int, default=12)
    ap.add_argument("--part", default="decode,encode")
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

    say("indexed_decode.py: source %s, device %s, %d rounds x %d indexed calls per unindexed call"
        % (build.source_hash(), torch.cuda.get_device_name(0), a.rounds, a.fast_per_round))

    def frames_of(n, rgb):
        return torch.stack([synth_torch.rgb8(W, H, f) if rgb else synth_torch.gray8(W, H, f, "S1") for f in range(n)]).cuda()

    if "decode" in a.part:
        for name, n, rgb in (("1 gray8 4K S1 frame", 1, 0), ("64 gray8 4K S1 frames", 64, 0), ("1 RGB8 4K frame", 1, 1)):
            frames = frames_of(n, rgb)
            cap = n * ((frames[0].numel() * 5 // 4 + 64 + 15) // 16 * 16)
            d_out = torch.empty(cap, dtype=torch.uint8, device="cuda")
            d_px = torch.zeros_like(frames)
            sets = {}
            for seg in SEGS:
                isize = api.index_size(W, H, rgb, 0, seg)
                d_idx = torch.empty(n * isize, dtype=torch.uint8, device="cuda")
                torch.cuda.synchronize()
                offs, lens = enc.compress_batch_device_indexed(frames.data_ptr(), n, W, H, rgb, 0, d_out.data_ptr(), cap, seg, d_idx.data_ptr(), n * isize)
                sets[seg] = (isize, d_idx)
            bits = 8.0 * float(sum(int(x) for x in lens)) / frames.numel()
            say("%s (%.1f MPix, %.2f bits per sample)" % (name, n * W * H / 1e6, bits))

            def plain():
                enc.decompress_batch_device(d_out.data_ptr(), offs, lens, d_px.data_ptr(), d_px.numel())

            def indexed(seg):
                isize, d_idx = sets[seg]
                enc.decompress_batch_device_indexed(d_out.data_ptr(), offs, lens, d_idx.data_ptr(), isize, d_px.data_ptr(), d_px.numel())

            def checked(fn):  # the call alone between the events; the frame zeroed before it, compared after it
                d_px.zero_()
                t = timed(fn)
                assert torch.equal(d_px, frames)
                return t

            checked(plain)  # untimed: allocations, code objects
            for seg in SEGS:
                checked(lambda: indexed(seg))
            t_plain, t_idx = [], {seg: [] for seg in SEGS}
            for _ in range(a.rounds):
                t_plain.append(checked(plain))
                for _ in range(a.fast_per_round):
                    for seg in SEGS:
                        t_idx[seg].append(checked(lambda: indexed(seg)))
            base = statistics.median(t_plain)
            say("  unindexed (a wave per stream)            : %s  %7.1f MPix/s" % (fmt(t_plain), n * W * H / base / 1e3))
            for seg in SEGS:
                m = statistics.median(t_idx[seg])
                k = (W * H + seg - 1) // seg
                say("  indexed, segment %6d px (K = %4d)    : %s  %7.1f MPix/s  %6.1fx  index %8d bytes per frame"
                    % (seg, k, fmt(t_idx[seg]), n * W * H / m / 1e3, base / m, sets[seg][0]))
            if n == 1 and not rgb:
                sp = base / statistics.median(t_idx[4096 * 32])
                say("  acceptance (K = 64, one gray frame, at least 32x): %.1fx -- %s" % (sp, "met" if sp >= 32 else "MISSED by %.1fx" % (32 / sp)))
            del frames, d_out, d_px, sets
            torch.cuda.empty_cache()

    if "encode" in a.part:
        n, seg = 64, 4096 * 32
        frames = frames_of(n, 0)
        cap = n * ((frames[0].numel() * 5 // 4 + 64 + 15) // 16 * 16)
        d_out = torch.empty(cap, dtype=torch.uint8, device="cuda")
        isize = api.index_size(W, H, 0, 0, seg)
        d_idx = torch.empty(n * isize, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()

        def plain():
            enc.compress_batch_device(frames.data_ptr(), n, W, H, 0, 0, d_out.data_ptr(), cap)

        def indexed():
            enc.compress_batch_device_indexed(frames.data_ptr(), n, W, H, 0, 0, d_out.data_ptr(), cap, seg, d_idx.data_ptr(), n * isize)

        plain()
        indexed()
        t_plain, t_idx = [], []
        for _ in range(a.encode_reps):
            t_plain.append(timed(plain))
            t_idx.append(timed(indexed))
        p, i = statistics.median(t_plain), statistics.median(t_idx)
        say("encode, 64 gray8 4K S1 frames per blocking call, alternating")
        say("  felics_compress_batch_device              : %s" % fmt(t_plain))
        say("  felics_compress_batch_device_indexed K=64 : %s  index %d bytes per frame, %.1f MB per call" % (fmt(t_idx), isize, n * isize / 1e6))
        say("  overhead: %.3f ms = %.1f %% of the plain call" % (i - p, 100.0 * (i - p) / p))
    enc.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
