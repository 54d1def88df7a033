"""Mixed-shape batches on one GPU: (a) one felics_compress_images_device call against (b) one felics_compress_batch_device call
per distinct shape and (c) a same-shape batch of the same total pixels at the median shape.  (a) is byte-checked against (b).

    python profiles/tools/mixed_batch.py [--images 256] [--min 256] [--max 1024] [--reps 10] [--out FILE]

Content: synthetic S1 gray8 frames (felics_amd.synth), every image its own shape.  Times are wall-clock medians of --reps calls
after two warm-up calls, each call synchronous; then one call of (a) with profiling on reports the library's per-stage sums and
span (felics_get_stage_ms / felics_get_span_ms) of the last sub-batch collected."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=256)
    ap.add_argument("--min", type=int, default=256)
    ap.add_argument("--max", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import numpy as np
    import torch

    import felics_amd
    from felics_amd import build, synth

    rng = np.random.default_rng(1)
    shapes = set()
    while len(shapes) < a.images:
        shapes.add((int(rng.integers(a.min, a.max + 1)), int(rng.integers(a.min, a.max + 1))))
    shapes = sorted(shapes, key=lambda s: rng.random())
    frames = [torch.from_numpy(synth.gray8(w, h, i, "S1")).cuda() for i, (w, h) in enumerate(shapes)]
    total_pix = sum(w * h for w, h in shapes)
    mw, mh = sorted(shapes, key=lambda s: s[0] * s[1])[len(shapes) // 2]
    nc = max(1, round(total_pix / (mw * mh)))
    med = torch.from_numpy(np.stack([synth.gray8(mw, mh, i, "S1") for i in range(nc)])).cuda()
    cap = sum(w * h + w * h // 4 + 80 for w, h in shapes) + (1 << 20)
    out_a = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    out_b = torch.zeros(cap, dtype=torch.uint8, device="cuda")
    cap_c = nc * (mw * mh + mw * mh // 4 + 80) + (1 << 20)
    out_c = torch.zeros(cap_c, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    enc = felics_amd.Encoder(0)
    descs = [(f.data_ptr(), w, h, 0, 0) for f, (w, h) in zip(frames, shapes)]

    def run_a():
        return enc.compress_images_device(descs, out_a.data_ptr(), cap)

    def run_b():
        res, at = [], 0
        for f, (w, h) in zip(frames, shapes):
            slot = (w * h + w * h // 4 + 64 + 15) // 16 * 16
            offs, lens = enc.compress_batch_device(f.data_ptr(), 1, w, h, 0, 0, out_b.data_ptr() + at, slot)
            res.append((at + int(offs[0]), int(lens[0])))
            at += slot
        return res

    def run_c():
        return enc.compress_batch_device(med.data_ptr(), nc, mw, mh, 0, 0, out_c.data_ptr(), cap_c)

    def timed(fn):
        for _ in range(2):
            fn()
        ts = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(ts), min(ts), max(ts)

    sub0 = enc.stats()["submissions"]
    offs, lens = run_a()
    subs_a = enc.stats()["submissions"] - sub0
    got_a = out_a.cpu().numpy()
    rb = run_b()
    got_b = out_b.cpu().numpy()
    same = all(got_a[int(o):int(o) + int(n)].tobytes() == got_b[ob:ob + nb].tobytes() for o, n, (ob, nb) in zip(offs, lens, rb))
    ta, tb, tc = timed(run_a), timed(run_b), timed(run_c)
    enc.set_profiling(True)
    run_a()
    stages = {k: v for k, v in enc.stage_ms().items() if v}
    span = enc.span_ms()
    enc.set_profiling(False)
    bytes_a = int(sum(int(n) for n in lens))
    lines = [
        "mixed_batch.py: %d gray8 S1 images, each its own shape in [%d, %d]^2, %.1f MPix in all; source %s"
        % (a.images, a.min, a.max, total_pix / 1e6, build.source_hash()),
        "device %s, lanes %d" % (torch.cuda.get_device_name(0), enc.lane_count()),
        "(a) one felics_compress_images_device call: median %.2f ms (min %.2f, max %.2f), %d submissions, %.1f GPix/s"
        % (ta[0], ta[1], ta[2], subs_a, total_pix / ta[0] / 1e6),
        "(b) one felics_compress_batch_device call per shape (%d calls): median %.2f ms (min %.2f, max %.2f)" % (a.images, tb[0], tb[1], tb[2]),
        "(c) one same-shape batch of %d x %dx%d (median shape, %.1f MPix): median %.2f ms (min %.2f, max %.2f)"
        % (nc, mw, mh, nc * mw * mh / 1e6, tc[0], tc[1], tc[2]),
        "(b) / (a) = %.2f x   (a) / (c) = %.2f" % (tb[0] / ta[0], ta[0] / tc[0]),
        "(a) streams byte-identical to (b): %s (%d bytes)" % (same, bytes_a),
        "(a) profiled, last sub-batch collected: span %.3f ms; stage sums (ms) %s"
        % (span, ", ".join("%s %.3f" % kv for kv in sorted(stages.items()))),
    ]
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    enc.close()
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
