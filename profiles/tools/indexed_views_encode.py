"""Indexed encode of views and mixed shapes on one GPU: this build against another build of the library (the parent commit's).

    python profiles/tools/indexed_views_encode.py --parent-lib PARENT/libfelics.so [--reps 15] [--bench-runs 3] [--out FILE]

Legs (all gray8):
  A  sixteen synth S1 frames of four shapes between 1080p and 4K, each a window of a pitched surface, about 64 segments per plane;
  B  64 noise-free synth S1 frames of distinct shapes in [500, 600]^2, dense, segment_pixels = 16384.
Forms per leg:
  views     one felics_compress_views_device_indexed call (this build only: the parent has no such call);
  by_shape  the only GPU route the parent has: a strided device copy of every view to dense frames, grouped by shape, then one
            felics_compress_batch_device_indexed call per shape -- copies, the wait for them and the calls all timed; run with this
            build's library and with the parent's;
  plain     felics_compress_views_device on the same views, this build (leg C: what the indexes cost).
Leg D: plain `python bench.py --gpus 1`, the parent's library (FELICS_LIB_PATH) and this build's alternating (the order swaps every
round), --bench-runs each.

Each library is loaded in a child process of its own; the parent process never opens the GPU and asks the children for one call at
a time, form after form, --reps rounds after two warm-up rounds.  Times are wall-clock milliseconds of the synchronous route;
medians with min / max and the spread (max - min) / median of every form.  Before anything is timed every stream of `views` is
decoded on the host and compared with its frame, compared with the stream `by_shape` gives, and every index compared with
felics_index_build of its stream."""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
LEGS = ("A", "B")


def child():
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch

    import felics_amd
    from felics_amd import api, build, synth

    new = hasattr(api.lib(), "felics_compress_views_device_indexed")
    rng = np.random.default_rng(64)
    enc = felics_amd.Encoder(0)
    work = {}

    def leg(name, shapes, seg_of, pitched):
        frames, surfaces, views = [], [], []
        for i, (w, h) in enumerate(shapes):
            f = synth.gray8(w, h, i, "S1")
            frames.append(f)
            if pitched:
                pitch = (w + 64 + 255) // 256 * 256
                s = torch.zeros((h + 4, pitch), dtype=torch.uint8, device="cuda")
                s[2:2 + h, 32:32 + w] = torch.from_numpy(f).cuda()
                surfaces.append(s)
                views.append((s.data_ptr() + 2 * pitch + 32, w, h, 0, 0, pitch, 1, 0))
            else:
                s = torch.from_numpy(f).cuda()
                surfaces.append(s)
                views.append((s.data_ptr(), w, h, 0, 0, w, 1, 0))
        segs = [seg_of(w, h) for w, h in shapes]
        groups = {}
        for i, sh in enumerate(shapes):
            groups.setdefault(sh, []).append(i)
        dense = {sh: torch.zeros((len(ix), sh[1], sh[0]), dtype=torch.uint8, device="cuda") for sh, ix in groups.items()}
        isize = [api.index_size(w, h, 0, 0, s) for (w, h), s in zip(shapes, segs)]
        ioffs = np.concatenate([[0], np.cumsum(isize)[:-1]]).astype(np.uint64)
        cap = sum(w * h * 5 // 4 + 96 for w, h in shapes) + (1 << 20)
        work[name] = dict(shapes=shapes, frames=frames, surfaces=surfaces, views=views, segs=segs, groups=groups, dense=dense, isize=isize, ioffs=ioffs,
                          cap=cap, out=torch.zeros(cap, dtype=torch.uint8, device="cuda"), out2=torch.zeros(cap, dtype=torch.uint8, device="cuda"),
                          idx=torch.zeros(int(sum(isize)) + 64, dtype=torch.uint8, device="cuda"),
                          idx2=torch.zeros(int(sum(isize)) + 64, dtype=torch.uint8, device="cuda"), pitched=pitched)

    def seg64(w, h):  # about 64 segments per plane
        return max(1, -(-w * h // 64) // 4096) * 4096

    leg("A", [s for s in ((1920, 1080), (2560, 1440), (3200, 1800), (3840, 2160)) for _ in range(4)], seg64, True)
    shapes = set()
    while len(shapes) < 64:
        shapes.add((int(rng.integers(500, 601)), int(rng.integers(500, 601))))
    leg("B", sorted(shapes, key=lambda s: rng.random()), lambda w, h: 16384, False)
    torch.cuda.synchronize()

    def call(name, form):
        """-> per view (offset, length) in out / out2, index offset"""
        w = work[name]
        if form == "views":
            offs, lens, _, _ = enc.compress_views_device_indexed(w["views"], w["segs"], w["out"].data_ptr(), w["cap"], w["idx"].data_ptr(),
                                                                 w["idx"].numel(), idx_offsets=w["ioffs"])
            return offs, lens
        if form == "plain":
            return enc.compress_views_device(w["views"], w["out"].data_ptr(), w["cap"])
        # by_shape: copy every view to its shape's dense batch, wait, one indexed call per shape
        for sh, ix in w["groups"].items():
            for k, i in enumerate(ix):
                s = w["surfaces"][i]
                w["dense"][sh][k].copy_(s[2:2 + sh[1], 32:32 + sh[0]] if w["pitched"] else s)
        torch.cuda.synchronize()
        offs, lens, at = np.zeros(len(w["views"]), np.uint64), np.zeros(len(w["views"]), np.uint64), 0
        for sh, ix in w["groups"].items():
            n = len(ix)
            room = n * (sh[0] * sh[1] * 5 // 4 + 96)
            o, ln = enc.compress_batch_device_indexed(w["dense"][sh].data_ptr(), n, sh[0], sh[1], 0, 0, w["out2"].data_ptr() + at, room, w["segs"][ix[0]],
                                                      w["idx2"].data_ptr() + int(w["ioffs"][ix[0]]), n * w["isize"][ix[0]])
            for k, i in enumerate(ix):
                offs[i], lens[i] = at + int(o[k]), ln[k]
            at += (room + 15) // 16 * 16
        return offs, lens

    for name in LEGS:  # what every form writes, checked once
        w = work[name]
        forms = ("views", "plain", "by_shape") if new else ("by_shape",)
        for form in forms:
            before = enc.stats()["submissions"]
            offs, lens = call(name, form)
            subs = enc.stats()["submissions"] - before
            host = (w["out2"] if form == "by_shape" else w["out"]).cpu().numpy()
            ihost = (w["idx2"] if form == "by_shape" else w["idx"]).cpu().numpy()
            hs, hi, ok = hashlib.sha256(), hashlib.sha256(), True
            for i, (o, n) in enumerate(zip(offs, lens)):
                stream = host[int(o):int(o) + int(n)].tobytes()
                hs.update(stream)
                if form != "views":
                    continue
                index = ihost[int(w["ioffs"][i]):int(w["ioffs"][i]) + w["isize"][i]].tobytes()
                hi.update(index)
                ok = ok and (api.decompress_bytes(stream) == w["frames"][i]).all() and index == api.index_build(stream, w["segs"][i])
            if form == "by_shape":  # its indexes lie group by group: index k of a group behind the group's first
                hi = hashlib.sha256()
                for i in range(len(w["views"])):
                    sh = w["shapes"][i]
                    ix = w["groups"][sh]
                    at = int(w["ioffs"][ix[0]]) + ix.index(i) * w["isize"][i]
                    index = ihost[at:at + w["isize"][i]].tobytes()
                    hi.update(index)
                    stream = host[int(offs[i]):int(offs[i]) + int(lens[i])].tobytes()
                    ok = ok and index == api.index_build(stream, w["segs"][i])
            print("INFO %s %s subs=%d bytes=%d sha=%s isha=%s ok=%d pix=%d n=%d shapes=%d ibytes=%d" % (
                name, form, subs, int(sum(int(n) for n in lens)), hs.hexdigest(), hi.hexdigest(), int(ok), sum(a * b for a, b in w["shapes"]),
                len(w["views"]), len(w["groups"]), int(sum(w["isize"]))), flush=True)
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


def bench(lib):
    env = dict(os.environ)
    if lib:
        env["FELICS_LIB_PATH"] = os.path.abspath(lib)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"], capture_output=True, text=True, env=env, cwd=ROOT, timeout=600)
    for line in reversed(out.stdout.splitlines()):
        if line.startswith("{"):
            return float(json.loads(line)["value"])
    raise RuntimeError("bench.py printed no result line (exit %d): %s" % (out.returncode, out.stderr[-400:]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--bench-runs", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.child:
        return child()
    if not a.parent_lib:
        ap.error("--parent-lib is needed")
    here, parent = Child(None), Child(a.parent_lib)
    try:
        plan = [(leg, form, who) for leg in LEGS for form, who in (("views", "a"), ("by_shape", "b"), ("by_shape", "a"), ("plain", "a"))]
        ts = {k: [] for k in plan}
        for r in range(a.reps + 2):
            for k in plan:
                t = (here if k[2] == "a" else parent).ms(k[0], k[1])
                if r >= 2:
                    ts[k].append(t)
    finally:
        here.close()
        parent.close()
    runs = {"parent": [], "this": []}
    for r in range(a.bench_runs):  # (the order swaps every round: P T T P P T ..., so that neither build always follows the other)
        for who in (("parent", "this") if r % 2 == 0 else ("this", "parent")):
            runs[who].append(bench(a.parent_lib if who == "parent" else None))

    def stat(k):
        v = ts[k]
        m = statistics.median(v)
        return m, min(v), max(v), (max(v) - min(v)) / m

    def fmt(s):
        return "median %.2f ms (min %.2f, max %.2f, spread %.0f %%)" % (s[0], s[1], s[2], 100 * s[3])

    lines = ["indexed_views_encode.py: this build (source %s) against the library given as --parent-lib (the parent commit's, built out of tree)" % here.ready[1],
             "device %s; a child process per library, forms alternating call by call, medians of %d after 2 warm-up rounds" % (here.ready[0], a.reps)]
    ok = True
    for leg in LEGS:
        iv, ip, ib, ic = here.info[(leg, "views")], parent.info[(leg, "by_shape")], here.info[(leg, "by_shape")], here.info[(leg, "plain")]
        V, P, B, C = stat((leg, "views", "a")), stat((leg, "by_shape", "b")), stat((leg, "by_shape", "a")), stat((leg, "plain", "a"))
        same = iv["sha"] == ip["sha"] == ib["sha"] == ic["sha"] and iv["isha"] == ip["isha"] == ib["isha"]
        checked = iv["ok"] == "1" and ip["ok"] == "1" and ib["ok"] == "1"
        ok = ok and same and checked
        mpix = int(iv["pix"]) / 1e6
        what = "windows of pitched surfaces, about 64 segments per plane" if leg == "A" else "dense, distinct shapes in [500, 600]^2, 16384 pixels per segment"
        lines += [
            "leg %s: %s gray8 S1 frames of %s shapes, %.1f MPix, %s; %.1f MB of indexes" % (leg, iv["n"], iv["shapes"], mpix, what, int(iv["ibytes"]) / 1e6),
            "  views, this build     : %s, %s submissions, %.2f GPix/s" % (fmt(V), iv["subs"], mpix / V[0]),
            "  by_shape, parent's lib: %s, %s submissions" % (fmt(P), ip["subs"]),
            "  by_shape, this build  : %s, %s submissions" % (fmt(B), ib["subs"]),
            "  by_shape (parent) / views = %.2f x   views faster by more than by_shape's spread: %s" % (P[0] / V[0], (P[0] - V[0]) / P[0] > P[3]),
            "  leg C, plain felics_compress_views_device, this build: %s, %s submissions; views / plain = %.2f (the indexes: +%.2f ms)"
            % (fmt(C), ic["subs"], V[0] / C[0], V[0] - C[0]),
            "  streams of all forms byte-identical, indexes of views and by_shape (both builds) byte-identical: %s; every stream of views decodes to its frame"
            " and every index equals felics_index_build of its stream: %s" % (same, checked),
        ]
    if a.bench_runs:
        P, T = runs["parent"], runs["this"]
        lines += ["leg D: python bench.py --gpus 1, alternating, MPix/s: parent %s, this build %s; medians %.1f / %.1f, ratio %.3f; ranges %s" % (
            " ".join("%.1f" % v for v in P), " ".join("%.1f" % v for v in T), statistics.median(P), statistics.median(T),
            statistics.median(T) / statistics.median(P), "overlap" if min(T) <= max(P) and min(P) <= max(T) else "DO NOT overlap")]
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
