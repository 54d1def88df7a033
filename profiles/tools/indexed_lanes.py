"""Restart index on one GPU: the two forms of felics_decompress_batch_device_indexed against each other -- a wave per segment
(k_decode8_seg) and 64 segments per wave, a lane per stream (k_decode8_seg_lanes).

    python profiles/tools/indexed_lanes.py [--rounds 5] [--sweep-rounds 9] [--part frames,noise,rgb,sweep] [--out FILE]

Protocol.  One process; the form is forced per call through FELICS_TEST_INDEX_LANES and the forms alternate.  A round is three
calls in three seats: wave form, lane form, wave form again.  The wave form sits in two seats so that the difference of the two
seats' medians -- the same kernel on the same data, a call apart -- says what the protocol itself cannot tell apart: the MARGIN.
One untimed call of each form first (allocations, code objects).  A time is what two device events around the blocking call
measure; the pixels are compared with the frames after every call; medians are reported.

Legs.  64 and 256 3840 x 2160 gray8 S1 frames at K = 64, 254 and 2025 (segment_pixels = 4096 x 32, x 8, x 1); the same as noise;
64 RGB8 1920 x 1080 frames at K = 64 (segment_pixels 32768: 63.3 rounded up); and the sweep: 64 frames of 512 x 8 K pixels at
segment_pixels 4096, so K segments a plane and 64 C K lane-form items, K growing from 1 (64 gray items, 192 RGB items).  The sweep
reports the smallest item count from which on the lane form beats the wave form by more than the margin at every count of the
sweep: what INDEX8_LANES_MIN_ITEMS(_RGB) in felics_kernels.h are set to (0xFFFFFFFF if there is none)."""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
SWITCH = "FELICS_TEST_INDEX_LANES"
SWEEP_K = (1, 2, 4, 8, 12, 16, 24, 32, 48, 64, 96, 128, 256)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--sweep-rounds", type=int, default=9)
    ap.add_argument("--part", default="frames,noise,rgb,sweep")
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

    say("indexed_lanes.py: source %s, device %s, %d rounds (sweep: %d) of wave / lane / wave"
        % (build.source_hash(), torch.cuda.get_device_name(0), a.rounds, a.sweep_rounds))
    say("thresholds in this build: gray %d, RGB %d lane-form items" % (api.index_lanes_min_items(0), api.index_lanes_min_items(1)))

    def make(kind, n, w, h, rgb):
        if kind == "noise":
            g = torch.Generator(device="cuda")
            g.manual_seed(1234 + n)
            return torch.randint(0, 256, (n, h, w, 3) if rgb else (n, h, w), dtype=torch.uint8, device="cuda", generator=g)
        return torch.stack([synth_torch.rgb8(w, h, f) if rgb else synth_torch.gray8(w, h, f, "S1") for f in range(n)]).cuda()

    def leg(frames, n, w, h, rgb, seg, rounds):
        """-> (wave median, lane median, margin, K), all in ms"""
        cap = n * ((frames[0].numel() * 5 // 4 + 64 + 15) // 16 * 16)
        d_out = torch.empty(cap, dtype=torch.uint8, device="cuda")
        d_px = torch.zeros_like(frames)
        isize = api.index_size(w, h, rgb, 0, seg)
        d_idx = torch.empty(n * isize, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        offs, lens = enc.compress_batch_device_indexed(frames.data_ptr(), n, w, h, rgb, 0, d_out.data_ptr(), cap, seg, d_idx.data_ptr(), n * isize)

        def call(form):
            os.environ[SWITCH] = str(form)
            d_px.zero_()
            before = enc.decode_stats()
            t = timed(lambda: enc.decompress_batch_device_indexed(d_out.data_ptr(), offs, lens, d_idx.data_ptr(), isize, d_px.data_ptr(), d_px.numel()))
            after = enc.decode_stats()
            assert torch.equal(d_px, frames)
            assert (after["lane_segments8"] > before["lane_segments8"]) == bool(form)
            return t

        call(0)
        call(1)
        seat_a, seat_b, seat_c = [], [], []
        for _ in range(rounds):
            seat_a.append(call(0))
            seat_b.append(call(1))
            seat_c.append(call(0))
        del os.environ[SWITCH]
        wave = statistics.median(seat_a + seat_c)
        margin = abs(statistics.median(seat_a) - statistics.median(seat_c))
        del d_out, d_px, d_idx
        torch.cuda.empty_cache()
        return wave, statistics.median(seat_b), margin, (w * h + seg - 1) // seg

    def report(label, n, w, h, res):
        wave, lane, margin, k = res
        mpix = n * w * h / 1e3
        say("  %-34s: wave %9.2f ms %7.1f MPix/s | lane %9.2f ms %7.1f MPix/s | margin %6.3f ms | lane form %5.2fx %s"
            % (label, wave, mpix / wave, lane, mpix / lane, margin, wave / lane, "FASTER" if wave - lane > margin else "not faster"))

    W, H = 3840, 2160
    for kind in ("frames", "noise"):
        if kind not in a.part:
            continue
        for n in (64, 256):
            frames = make("S1" if kind == "frames" else "noise", n, W, H, 0)
            say("%d gray8 %d x %d %s frames (%.1f MPix)" % (n, W, H, "S1" if kind == "frames" else "noise", n * W * H / 1e6))
            for seg in (4096 * 32, 4096 * 8, 4096):
                res = leg(frames, n, W, H, 0, seg, a.rounds)
                report("K = %4d (%d items)" % (res[3], n * res[3]), n, W, H, res)
            del frames
            torch.cuda.empty_cache()
    if "rgb" in a.part:
        n, w, h = 64, 1920, 1080
        frames = make("S1", n, w, h, 1)
        say("%d RGB8 %d x %d frames (%.1f MPix)" % (n, w, h, n * w * h / 1e6))
        res = leg(frames, n, w, h, 1, 32768, a.rounds)
        report("K = %4d (%d items)" % (res[3], n * 3 * res[3]), n, w, h, res)
        del frames
        torch.cuda.empty_cache()
    if "sweep" in a.part:
        for rgb in (0, 1):
            say("sweep, 64 %s frames of 512 x 8 K at segment_pixels 4096 (S1 content): 64 C K lane-form items" % ("RGB8" if rgb else "gray8"))
            wins = []
            for k in SWEEP_K:
                w, h, n = 512, 8 * k, 64
                frames = make("S1", n, w, h, rgb)
                res = leg(frames, n, w, h, rgb, 4096, a.sweep_rounds)
                items = n * (3 if rgb else 1) * k
                report("%6d items (K = %3d)" % (items, k), n, w, h, res)
                wins.append((items, res[0] - res[1] > res[2]))
                del frames
            first = None
            for items, won in reversed(wins):
                if not won:
                    break
                first = items
            say("  => %s: the lane form beats the wave form by more than the margin from %s"
                % ("RGB" if rgb else "gray", "%d items on" % first if first is not None else "no count of the sweep on (0xFFFFFFFF)"))
    enc.close()


if __name__ == "__main__":
    main()
