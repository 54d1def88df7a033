"""Restart index for 16-bit streams on one GPU: what it buys the decoder.

    python profiles/tools/indexed_decode16.py [--rounds 2] [--fast-per-round 3] [--out FILE]

Workloads: one synthetic 3840 x 2160 gray16 frame (synth.gray16), one RGB16 frame (the same with two chroma offsets), 16 gray16
frames.  felics_decompress_batch_device (a wave per stream, k_decode16) against felics_decompress_batch_device_indexed16 at
segment_pixels = 4096 x {127, 32, 8, 1} (K = 16, 64, 254, 2025; the 16 frames at K = 64 only), the streams written by the GPU encoder,
the indexes by felics_index16_build.  One untimed call of every form first; then --rounds rounds, each one unindexed call (seconds)
followed by --fast-per-round calls of every indexed setting, so the forms alternate in one process.  A time is what two device
events around the blocking call measure, reported as median (min .. max).  Pixels are compared with the frames after every call.
Beside every K: the index's size against felics_index16_size_max, the table memory of a pass and the passes of a call."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
W, H = 3840, 2160
SEGS = (4096 * 127, 4096 * 32, 4096 * 8, 4096)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--fast-per-round", type=int, default=3)
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

    say("indexed_decode16.py: source %s, device %s, %d rounds x %d indexed calls per unindexed call"
        % (build.source_hash(), torch.cuda.get_device_name(0), a.rounds, a.fast_per_round))

    def frame_of(f, rgb):
        g = synth.gray16(W, H, f)
        if not rgb:
            return g
        r = np.clip(g.astype(np.int64) + (g & 3) * 16 - 24, 0, 65535)
        b = np.clip(g.astype(np.int64) - ((g >> 2) & 3) * 16 + 24, 0, 65535)
        return np.stack([r, g, b], -1).astype(np.uint16)

    for name, n, rgb, segs in (("1 gray16 4K frame", 1, 0, SEGS), ("1 RGB16 4K frame", 1, 1, SEGS), ("16 gray16 4K frames", 16, 0, SEGS[1:2])):
        frames = torch.from_numpy(np.stack([frame_of(f, rgb) for f in range(n)]).view(np.int16)).cuda()
        ref = frames.clone()
        cap = n * ((frames[0].numel() * 2 * 5 // 4 + 64 + 15) // 16 * 16)
        d_out = torch.empty(cap, dtype=torch.uint8, device="cuda")
        d_px = torch.zeros_like(frames)
        torch.cuda.synchronize()
        offs, lens = enc.compress_batch_device(frames.data_ptr(), n, W, H, rgb, 1, d_out.data_ptr(), cap)
        host = d_out.cpu().numpy()
        streams = [host[int(o):int(o) + int(l)].tobytes() for o, l in zip(offs, lens)]
        sets = {}
        for seg in segs:
            indexes = [api.index16_build(s, seg) for s in streams]
            blob, ioffs = bytearray(), []
            for ix in indexes:
                ioffs.append(len(blob))
                blob += ix + bytes((-len(ix)) % 64)
            d_idx = torch.from_numpy(np.frombuffer(bytes(blob), np.uint8).copy()).cuda()
            assert d_idx.data_ptr() % 64 == 0
            sets[seg] = (d_idx, ioffs, [len(ix) for ix in indexes])
        bits = 8.0 * float(sum(int(x) for x in lens)) / frames.numel()
        say("%s (%.1f MPix, %.2f bits per sample)" % (name, n * W * H / 1e6, bits))

        def plain():
            enc.decompress_batch_device(d_out.data_ptr(), offs, lens, d_px.data_ptr(), d_px.numel() * 2)

        def indexed(seg):
            d_idx, ioffs, ilens = sets[seg]
            enc.decompress_batch_device_indexed16(d_out.data_ptr(), offs, lens, d_idx.data_ptr(), ioffs, ilens, d_px.data_ptr(), d_px.numel() * 2)

        def checked(fn):  # the call alone between the events; the frames zeroed before it, compared after it
            d_px.zero_()
            t = timed(fn)
            assert torch.equal(d_px, ref)
            return t

        checked(plain)  # untimed: allocations (the tables are zeroed once), code objects
        info = {}
        for seg in segs:
            before = enc.index16_stats()
            checked(lambda: indexed(seg))
            after = enc.index16_stats()
            info[seg] = (after["passes"] - before["passes"], after["table_bytes"], after["rows_loaded"] - before["rows_loaded"])
        t_plain, t_idx = [], {seg: [] for seg in segs}
        for _ in range(a.rounds):
            t_plain.append(checked(plain))
            for _ in range(a.fast_per_round):
                for seg in segs:
                    t_idx[seg].append(checked(lambda: indexed(seg)))
        base = statistics.median(t_plain)
        say("  unindexed (a wave per stream)            : %s  %7.1f MPix/s" % (fmt(t_plain), n * W * H / base / 1e3))
        for seg in segs:
            m = statistics.median(t_idx[seg])
            k = (W * H + seg - 1) // seg
            passes, table_bytes, loaded = info[seg]
            say("  indexed, segment %6d px (K = %4d)    : %s  %7.1f MPix/s  %6.1fx" % (seg, k, fmt(t_idx[seg]), n * W * H / m / 1e3, base / m))
            say("      index %d bytes per frame (felics_index16_size_max: %d), %d rows loaded per call; %d pass(es), tables of a pass %.1f MB"
                % (max(sets[seg][2]), api.index16_size_max(W, H, rgb, seg), loaded, passes, table_bytes / 1e6))
        if n == 1 and not rgb:
            sp = base / statistics.median(t_idx[4096 * 32])
            say("  acceptance (K = 64, one gray16 frame, at least 32x): %.1fx -- %s" % (sp, "met" if sp >= 32 else "MISSED by %.1fx" % (32 / sp)))
        del frames, ref, d_out, d_px, sets
        torch.cuda.empty_cache()
    enc.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
