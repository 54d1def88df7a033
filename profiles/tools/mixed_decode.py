"""Mixed-shape decoding on one GPU: one felics_decompress_images_device call against one felics_decompress_batch_device call per
distinct shape and against the host decoder on 16 threads.  Every leg's pixels are checked against the frames.

    python profiles/tools/mixed_decode.py [--reps 5] [--shape-reps 1] [--out FILE]

Cases: (a) 256 gray8 S1 streams of distinct shapes in [256, 1024]^2; (b) 4 096 gray8 streams of distinct shapes in [64, 256]^2;
(c) 4 096 streams of 16 shapes, 256 each (mixed call with the library's choice and with both forms forced, and the per-shape calls).
Times are synchronised wall-clock medians of --reps calls after one warm-up call (--shape-reps for the per-shape legs of (a) and
(b): hundreds of calls of one stream each, each as long as its stream)."""
import argparse
import concurrent.futures as cf
import ctypes as C
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shape-reps", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import numpy as np
    import torch

    import felics_amd
    from felics_amd import api, build, synth

    enc = felics_amd.Encoder(0)
    L = api.lib()
    lines = ["mixed_decode.py: source %s, device %s" % (build.source_hash(), torch.cuda.get_device_name(0))]
    ok_all = True

    def timed(fn, reps, warm=1):
        for _ in range(warm):
            fn()
        ts = []
        for _ in range(reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(ts), min(ts), max(ts), len(ts)

    def case(name, shapes, forced_legs=False, per_shape_reps=None):
        nonlocal ok_all
        rng = np.random.default_rng(7)
        cache = {}
        frames = []
        for i, (w, h) in enumerate(shapes):
            if (w, h) not in cache or len(cache) < 64:
                cache[(w, h)] = synth.gray8(w, h, i % 97, "S1")
            frames.append(cache[(w, h)])
        d_fr = [torch.from_numpy(f).cuda() for f in frames]
        cap = sum(f.size * 2 + 96 for f in frames) + (1 << 20)
        d_out = torch.zeros(cap, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        offs, lens = enc.compress_images_device([(t.data_ptr(), f.shape[1], f.shape[0], 0, 0) for t, f in zip(d_fr, frames)], d_out.data_ptr(), cap)
        npx = sum(f.size for f in frames)
        need = sum((f.size + 15) // 16 * 16 for f in frames)
        d_px = torch.zeros(need + 64, dtype=torch.uint8, device="cuda")

        def check_mixed(po):
            host = d_px.cpu().numpy()
            return all((host[int(o): int(o) + f.size].reshape(f.shape) == f).all() for o, f in zip(po, frames))

        res = {}

        def mixed():
            res["po"] = enc.decompress_images_device(d_out.data_ptr(), offs, lens, d_px.data_ptr(), need)[0]

        legs = [("one mixed call", None)] + ([("mixed call, lane form forced", "1"), ("mixed call, wave form forced", "0")] if forced_legs else [])
        out = []
        for label, env in legs:
            if env is not None:
                os.environ["FELICS_TEST_DECODE_LANES"] = env
            try:
                t = timed(mixed, a.reps)
            finally:
                os.environ.pop("FELICS_TEST_DECODE_LANES", None)
            good = check_mixed(res["po"])
            ok_all &= good
            out.append("  %s: median %.2f ms (min %.2f, max %.2f, %d runs), %.3f GPix/s, pixels exact: %s" % (label, t[0], t[1], t[2], t[3], npx / t[0] / 1e6, good))
        # one same-shape call per distinct shape
        groups = {}
        for i, f in enumerate(frames):
            groups.setdefault(f.shape, []).append(i)
        gbuf = {s: torch.zeros(len(ix) * s[0] * s[1] + 16, dtype=torch.uint8, device="cuda") for s, ix in groups.items()}

        def per_shape():
            for s, ix in groups.items():
                enc.decompress_batch_device(d_out.data_ptr(), offs[ix], lens[ix], gbuf[s].data_ptr(), len(ix) * s[0] * s[1])

        t = timed(per_shape, per_shape_reps or a.reps, warm=1 if per_shape_reps is None else 0)
        good = all((gbuf[s].cpu().numpy()[k * s[0] * s[1]:(k + 1) * s[0] * s[1]].reshape(s) == frames[i]).all()
                   for s, ix in groups.items() for k, i in enumerate(ix))
        ok_all &= good
        out.append("  one felics_decompress_batch_device call per shape (%d calls): median %.2f ms (min %.2f, max %.2f, %d runs), pixels exact: %s"
                   % (len(groups), t[0], t[1], t[2], t[3], good))
        # the host decoder on 16 threads
        host_streams = d_out.cpu().numpy()
        blobs = [np.ascontiguousarray(host_streams[int(o): int(o + n)]) for o, n in zip(offs, lens)]
        outs = [np.zeros(f.shape, np.uint8) for f in frames]

        def one(k):
            return L.felics_decompress(blobs[k].ctypes.data, blobs[k].size, outs[k].ctypes.data, outs[k].nbytes, None)

        pool = cf.ThreadPoolExecutor(16)

        def host():
            assert all(rc == 0 for rc in pool.map(one, range(len(frames))))

        t = timed(host, a.reps)
        good = all((o == f).all() for o, f in zip(outs, frames))
        ok_all &= good
        out.append("  host decoder, 16 threads: median %.2f ms (min %.2f, max %.2f, %d runs), pixels exact: %s" % (t[0], t[1], t[2], t[3], good))
        pool.shutdown()
        lines.append("%s: %d gray8 S1 streams, %d shapes, %.1f MPix" % (name, len(frames), len(groups), npx / 1e6))
        lines.extend(out)

    rng = np.random.default_rng(1)

    def distinct(n, lo, hi):
        s = set()
        while len(s) < n:
            s.add((int(rng.integers(lo, hi + 1)), int(rng.integers(lo, hi + 1))))
        return sorted(s, key=lambda x: rng.random())

    case("(a)", distinct(256, 256, 1024), per_shape_reps=a.shape_reps)
    case("(b)", distinct(4096, 64, 256), per_shape_reps=a.shape_reps)
    sh16 = distinct(16, 64, 256)
    case("(c)", [sh16[i % 16] for i in range(4096)], forced_legs=True)
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    enc.close()
    return 0 if ok_all else 1


if __name__ == "__main__":
    sys.exit(main())
