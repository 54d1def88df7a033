"""Mixed-shape 16-bit batches on one GPU: this build against another build of the library (the parent commit's), call by call.

    python profiles/tools/mixed_batch16.py --parent-lib PARENT/libfelics.so [--reps 15] [--out FILE]

Workload: 256 gray16 synth.gray16 images of distinct shapes in [256, 1024]^2, and 128 RGB16 ones (three synth.gray16 frames per
image) in [128, 512]^2.  Per leg (gray16, RGB16):
  (a) one felics_compress_images_device call with this build;
  (b) the same call with the other build's library;
  (c) one same-shape batch (felics_compress_batch_device, this build) of the same pixel count at the median shape;
  control: one felics_compress_images_device call whose images all share the median shape, both builds (the path is unchanged).
Each library is loaded in a child process of its own (FELICS_LIB_PATH); the parent process never opens the GPU and asks the two
children for one call at a time, (a) then (b), leg after leg, --reps rounds after two warm-up rounds.  Times are wall-clock
milliseconds of the synchronous call; medians with min / max, the spread (max - min) / median of every form, the submission counts
(felics_stats) and whether the streams of (a) and (b) are byte-identical (sha256 over all streams in image order)."""
import argparse
import hashlib
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
LEGS = ("gray16", "rgb16")
FORMS = ("mixed", "same", "control")


def child():
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch

    import felics_amd
    from felics_amd import build, synth

    rng = np.random.default_rng(16)
    enc = felics_amd.Encoder(0)
    work = {}
    for leg, n, lo, hi in (("gray16", 256, 256, 1024), ("rgb16", 128, 128, 512)):
        rgb = leg == "rgb16"
        shapes = set()
        while len(shapes) < n:
            shapes.add((int(rng.integers(lo, hi + 1)), int(rng.integers(lo, hi + 1))))
        shapes = sorted(shapes, key=lambda s: rng.random())

        def frame(w, h, i):
            if rgb:
                return np.ascontiguousarray(np.stack([synth.gray16(w, h, 3 * i + c) for c in range(3)], axis=-1))
            return synth.gray16(w, h, i)

        frames = [torch.from_numpy(frame(w, h, i)).cuda() for i, (w, h) in enumerate(shapes)]
        total_pix = sum(w * h for w, h in shapes)
        mw, mh = sorted(shapes, key=lambda s: s[0] * s[1])[len(shapes) // 2]
        nc = max(1, round(total_pix / (mw * mh)))
        med = torch.from_numpy(np.stack([frame(mw, mh, i) for i in range(nc)])).cuda()
        ch = 3 if rgb else 1
        cap = sum(w * h * ch * 2 * 5 // 4 + 96 for w, h in shapes) + (1 << 20)
        cap_c = nc * (mw * mh * ch * 2 * 5 // 4 + 96) + (1 << 20)
        work[leg] = dict(
            descs=[(f.data_ptr(), w, h, int(rgb), 1) for f, (w, h) in zip(frames, shapes)], frames=frames, med=med, nc=nc, mw=mw, mh=mh,
            total_pix=total_pix, out=torch.zeros(cap, dtype=torch.uint8, device="cuda"), cap=cap,
            out_c=torch.zeros(cap_c, dtype=torch.uint8, device="cuda"), cap_c=cap_c, rgb=int(rgb),
            ctl=[(med.data_ptr() + i * mw * mh * ch * 2, mw, mh, int(rgb), 1) for i in range(nc)])
    torch.cuda.synchronize()

    def call(leg, form):
        w = work[leg]
        if form == "mixed":
            return enc.compress_images_device(w["descs"], w["out"].data_ptr(), w["cap"])
        if form == "same":
            return enc.compress_batch_device(w["med"].data_ptr(), w["nc"], w["mw"], w["mh"], w["rgb"], 1, w["out_c"].data_ptr(), w["cap_c"])
        return enc.compress_images_device(w["ctl"], w["out_c"].data_ptr(), w["cap_c"])

    for leg in LEGS:  # submissions and a digest of every form's streams, once
        w = work[leg]
        for form in FORMS:
            before = enc.stats()["submissions"]
            offs, lens = call(leg, form)
            subs = enc.stats()["submissions"] - before
            host = (w["out"] if form == "mixed" else w["out_c"]).cpu().numpy()
            h = hashlib.sha256()
            for o, n in zip(offs, lens):
                h.update(host[int(o):int(o) + int(n)].tobytes())
            print("INFO %s %s subs=%d bytes=%d sha=%s pix=%d nc=%d mw=%d mh=%d" % (leg, form, subs, int(sum(int(n) for n in lens)), h.hexdigest(),
                                                                                   w["total_pix"], w["nc"], w["mw"], w["mh"]), flush=True)
    print("READY %s %s" % (torch.cuda.get_device_name(0).replace(" ", "_"), build.source_hash()), flush=True)
    for line in sys.stdin:
        cmd = line.split()
        if not cmd or cmd[0] == "quit":
            break
        t0 = time.perf_counter()
        call(cmd[0], cmd[1])
        print("MS %.4f" % ((time.perf_counter() - t0) * 1e3), flush=True)
    enc.close()


class Child:
    def __init__(self, lib):
        env = dict(os.environ)
        if lib:
            env["FELICS_LIB_PATH"] = os.path.abspath(lib)
        self.p = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--child"], stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True,
                                  env=env, cwd=ROOT)
        self.info = {}
        self.ready = None
        for line in self.p.stdout:
            f = line.split()
            if f and f[0] == "INFO":
                self.info[(f[1], f[2])] = dict(kv.split("=") for kv in f[3:])
            elif f and f[0] == "READY":
                self.ready = f[1:]
                break
        if self.ready is None:
            raise RuntimeError("child for %s did not come up (exit %s)" % (lib or "this build", self.p.wait()))

    def ms(self, leg, form):
        self.p.stdin.write("%s %s\n" % (leg, form))
        self.p.stdin.flush()
        f = self.p.stdout.readline().split()
        if len(f) != 2 or f[0] != "MS":
            raise RuntimeError("child died (exit %s)" % self.p.wait())
        return float(f[1])

    def close(self):
        try:
            self.p.stdin.write("quit\n")
            self.p.stdin.flush()
        except OSError:
            pass
        self.p.wait(timeout=120)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.child:
        return child()
    if not a.parent_lib:
        ap.error("--parent-lib is needed")
    here, parent = Child(None), Child(a.parent_lib)
    try:
        plan = [(leg, "mixed", who) for leg in LEGS for who in ("a", "b")] + [(leg, "same", "a") for leg in LEGS] + \
               [(leg, "control", who) for leg in LEGS for who in ("a", "b")]
        ts = {k: [] for k in plan}
        for r in range(a.reps + 2):
            for k in plan:
                t = (here if k[2] == "a" else parent).ms(k[0], k[1])
                if r >= 2:
                    ts[k].append(t)
    finally:
        here.close()
        parent.close()

    def stat(k):
        v = ts[k]
        m = statistics.median(v)
        return m, min(v), max(v), (max(v) - min(v)) / m

    lines = ["mixed_batch16.py: this build (source %s) against the library given as --parent-lib (the parent commit's, built out of tree)" % here.ready[1],
             "device %s; a child process per library, forms alternating call by call, medians of %d after 2 warm-up rounds" % (here.ready[0], a.reps)]
    ok = True
    for leg in LEGS:
        ia, ib, ic = here.info[(leg, "mixed")], parent.info[(leg, "mixed")], here.info[(leg, "same")]
        A, B, Cc = stat((leg, "mixed", "a")), stat((leg, "mixed", "b")), stat((leg, "same", "a"))
        ca, cb = stat((leg, "control", "a")), stat((leg, "control", "b"))
        same = ia["sha"] == ib["sha"] and ia["bytes"] == ib["bytes"]
        ok = ok and same
        mpix = int(ia["pix"]) / 1e6
        lines += [
            "%s: %d images of distinct shapes, %.1f MPix" % (leg, 256 if leg == "gray16" else 128, mpix),
            "  (a) one felics_compress_images_device call, this build: median %.2f ms (min %.2f, max %.2f, spread %.0f %%), %s submissions, %.2f GPix/s"
            % (A[0], A[1], A[2], 100 * A[3], ia["subs"], mpix / A[0]),
            "  (b) the same call, parent's library: median %.2f ms (min %.2f, max %.2f, spread %.0f %%), %s submissions" % (B[0], B[1], B[2], 100 * B[3], ib["subs"]),
            "  (c) one same-shape batch of %s x %sx%s (median shape), this build: median %.2f ms (min %.2f, max %.2f), %s submissions"
            % (ic["nc"], ic["mw"], ic["mh"], Cc[0], Cc[1], Cc[2], ic["subs"]),
            "  (b) / (a) = %.2f x   (a) / (c) = %.2f   (a) faster than (b) by more than (b)'s spread: %s" % (B[0] / A[0], A[0] / Cc[0], (B[0] - A[0]) / B[0] > B[3]),
            "  streams of (a) and (b) byte-identical: %s (%s bytes)" % (same, ia["bytes"]),
            "  control, %s images of one shape through felics_compress_images_device: this build %.2f ms (min %.2f, max %.2f), parent %.2f ms (min %.2f, max %.2f),"
            " ratio %.2f, submissions %s / %s, streams identical: %s"
            % (ic["nc"], ca[0], ca[1], ca[2], cb[0], cb[1], cb[2], ca[0] / cb[0], here.info[(leg, "control")]["subs"], parent.info[(leg, "control")]["subs"],
               here.info[(leg, "control")]["sha"] == parent.info[(leg, "control")]["sha"]),
        ]
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
