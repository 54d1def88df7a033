"""Surface batches on one GPU: the queued surfaces call against the parent build's blocking views call and against dense frames
through the submission queue, form by form.

    python profiles/tools/surfaces_bench.py --leg a|b|c --parent-lib PARENT/libfelics.so [--reps 15] [--out FILE]

Legs:
  a  64 S1 gray8 windows of 3840 x 2160 in 4096 x 2304 surfaces
  b  64 RGBA surfaces of 1920 x 1080 read as RGB
  c  16 gray16 windows of 3840 x 2160 in 4096 x 2304 surfaces, FELICS_LANES=4
Forms, per leg:
  surfaces  felics_submit_surfaces_device, this build, two submissions in flight (leg c: the blocking felics_compress_surfaces_device)
  views     the parent build's blocking felics_compress_views_device on the same surfaces
  dense     the same pixels as dense frames through felics_submit_batch_device, this build, two in flight (leg c: one at a time)
Each library is loaded in a child process of its own (FELICS_LIB_PATH); the parent process never opens the GPU and asks the
children for one measurement at a time, the forms alternating, --reps rounds after two warm-up rounds.  A measurement of a queued
form is STEPS = 4 steps with the next submission made before the last one is waited for, reported per step; of a blocking form one
call.  Wall-clock milliseconds; medians with min / max and the spread (max - min) / median.  The frames of a leg repeat four distinct
ones; every form's streams are checked once: the distinct ones against the CPU oracle, the rest against those."""
import argparse
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
STEPS = 4
LEGS = {"a": dict(n=64, w=3840, h=2160, sw=4096, sh=2304, what="64 S1 gray8 windows of 3840 x 2160 in 4096 x 2304 surfaces"),
        "b": dict(n=64, w=1920, h=1080, sw=1920, sh=1080, what="64 RGBA 1920 x 1080 surfaces read as RGB"),
        "c": dict(n=16, w=3840, h=2160, sw=4096, sh=2304, what="16 gray16 windows of 3840 x 2160 in 4096 x 2304 surfaces, FELICS_LANES=4")}


def child(leg):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch

    import felics_amd
    from felics_amd import api, build, synth, synth_torch
    from tests import oracle_lib

    L = LEGS[leg]
    n, w, h, sw, sh = L["n"], L["w"], L["h"], L["sw"], L["sh"]
    dev = torch.device("cuda:0")
    enc = felics_amd.Encoder(0)
    y0, x0 = 64, 128
    if leg == "a":
        base = [synth_torch.gray8(w, h, f, "S1", device=dev) for f in range(4)]
        surf = torch.zeros((n, sh, sw), dtype=torch.uint8, device=dev)
        for i in range(n):
            surf[i, y0:y0 + h, x0:x0 + w] = base[i % 4]
        win = surf[:, y0:y0 + h, x0:x0 + w]
        color, depth, size = 0, 0, 1
        view = (win.data_ptr(), w, h, 0, 0, sw, 1, 0)
        fstride = sh * sw
    elif leg == "b":
        base = [synth_torch.rgb8(w, h, f, device=dev) for f in range(4)]
        surf = torch.full((n, h, w, 4), 255, dtype=torch.uint8, device=dev)
        for i in range(n):
            surf[i, :, :, :3] = base[i % 4]
        win = surf[..., :3]
        color, depth, size = 1, 0, 1
        view = (surf.data_ptr(), w, h, 1, 0, 4 * w, 4, 1)
        fstride = 4 * w * h
    else:
        base = [torch.from_numpy(synth.gray16(w, h, f).view(np.int16)).to(dev) for f in range(4)]  # (int16 storage of the u16 samples)
        surf = torch.zeros((n, sh, sw), dtype=torch.int16, device=dev)
        for i in range(n):
            surf[i, y0:y0 + h, x0:x0 + w] = base[i % 4]
        win = surf[:, y0:y0 + h, x0:x0 + w]
        color, depth, size = 0, 1, 2
        view = (win.data_ptr(), w, h, 0, 1, 2 * sw, 2, 0)
        fstride = 2 * sh * sw
    dense = win.contiguous()
    frame_bytes = w * h * (3 if color else 1) * size
    slot = (frame_bytes + frame_bytes // 4 + 64 + 15) & ~15
    cap = n * slot
    outs = [torch.zeros(cap, dtype=torch.uint8, device=dev) for _ in range(2)]
    views = [(view[0] + i * fstride,) + view[1:] for i in range(n)]
    have_surfaces = hasattr(api.lib(), "felics_submit_surfaces_device")
    torch.cuda.synchronize()
    queued = leg != "c"

    def submit(form, k):
        o = outs[k % 2]
        if form == "surfaces":
            return enc.submit_surfaces_device((view, fstride, n), o.data_ptr(), cap)
        return enc.submit_batch_device(dense.data_ptr(), n, w, h, color, depth, o.data_ptr(), cap)

    def measure(form):
        """One measurement; returns (offsets, lens) of the last step (in outs[(steps - 1) % 2])."""
        if form == "views":
            return enc.compress_views_device(views, outs[0].data_ptr(), cap), 1, 0
        if not queued:
            if form == "surfaces":
                return enc.compress_surfaces_device((view, fstride, n), outs[0].data_ptr(), cap), 1, 0
            return enc.compress_batch_device(dense.data_ptr(), n, w, h, color, depth, outs[0].data_ptr(), cap), 1, 0
        sub = submit(form, 0)
        for k in range(1, STEPS):
            nxt = submit(form, k)
            res = enc.wait_batch(sub)
            sub = nxt
        res = enc.wait_batch(sub)
        return res, STEPS, (STEPS - 1) % 2

    forms = ["views"] if not have_surfaces else ["surfaces", "dense", "views"]
    oracle = oracle_lib.load()
    want = [oracle.compress(np.ascontiguousarray(dense[i].cpu().numpy()).view(np.uint16 if depth else np.uint8)) for i in range(4)]
    for form in forms:  # every stream of every form, once
        (offs, lens), _, k = measure(form)
        host = outs[k].cpu().numpy()
        ok = all(host[int(o):int(o) + int(m)].tobytes() == want[i % 4] for i, (o, m) in enumerate(zip(offs, lens)))
        print("INFO %s ok=%d bytes=%d" % (form, ok, int(sum(int(m) for m in lens))), flush=True)
    if have_surfaces:
        print("STATS %s" % " ".join("%s=%d" % kv for kv in enc.surface_stats().items()), flush=True)
    print("READY %s %s" % (torch.cuda.get_device_name(0).replace(" ", "_"), build.source_hash()), flush=True)
    for line in sys.stdin:
        cmd = line.split()
        if not cmd or cmd[0] == "quit":
            break
        t0 = time.perf_counter()
        _, steps, _ = measure(cmd[0])
        print("MS %.4f" % ((time.perf_counter() - t0) * 1e3 / steps), flush=True)
    enc.close()


class Child:
    def __init__(self, lib, leg):
        env = dict(os.environ)
        if lib:
            env["FELICS_LIB_PATH"] = os.path.abspath(lib)
        if leg == "c":
            env["FELICS_LANES"] = "4"
        self.p = subprocess.Popen([sys.executable, os.path.abspath(__file__), "--child", "--leg", leg], stdin=subprocess.PIPE, stdout=subprocess.PIPE,
                                  text=True, env=env, cwd=ROOT)
        self.info, self.stats, self.ready = {}, "", None
        for line in self.p.stdout:
            f = line.split()
            if f and f[0] == "INFO":
                self.info[f[1]] = dict(kv.split("=") for kv in f[2:])
            elif f and f[0] == "STATS":
                self.stats = " ".join(f[1:])
            elif f and f[0] == "READY":
                self.ready = f[1:]
                break
        if self.ready is None:
            raise RuntimeError("child for %s did not come up (exit %s)" % (lib or "this build", self.p.wait()))

    def ms(self, form):
        self.p.stdin.write(form + "\n")
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
    ap.add_argument("--leg", choices=sorted(LEGS), required=True)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.child:
        return child(a.leg)
    if not a.parent_lib:
        ap.error("--parent-lib is needed")
    here, parent = Child(None, a.leg), Child(a.parent_lib, a.leg)
    plan = [("surfaces", here), ("views", parent), ("dense", here), ("views-this", here)]
    ts = {k: [] for k, _ in plan}
    try:
        for r in range(a.reps + 2):
            for k, who in plan:
                t = who.ms(k.split("-")[0])
                if r >= 2:
                    ts[k].append(t)
    finally:
        here.close()
        parent.close()
    L = LEGS[a.leg]
    mpix = L["n"] * L["w"] * L["h"] / 1e6
    lines = ["surfaces_bench.py leg %s: %s (%.0f MPix per step)" % (a.leg, L["what"], mpix),
             "this build (source %s) and the parent's library (--parent-lib), a child process each on %s; forms alternating, medians of %d after 2 warm-up rounds"
             % (here.ready[1], here.ready[0], a.reps)]
    names = {"surfaces": "surfaces call, this build" + (", two in flight" if a.leg != "c" else ", blocking, read in place"),
             "views": "blocking views call, parent's library", "dense": "dense frames, felics_submit_batch_device, this build" + (", two in flight" if a.leg != "c" else ", blocking"),
             "views-this": "blocking views call, this build"}
    med = {}
    for k, _ in plan:
        v = ts[k]
        med[k] = statistics.median(v)
        lines.append("  %-62s median %.3f ms per step (min %.3f, max %.3f, spread %.0f %%), %.2f GPix/s"
                     % (names[k] + ":", med[k], min(v), max(v), 100 * (max(v) - min(v)) / med[k], mpix / med[k] / 1e3))
    lines.append("  views (parent) / surfaces = %.2f x    surfaces / dense = %.2f" % (med["views"] / med["surfaces"], med["surfaces"] / med["dense"]))
    ok = all(i["ok"] == "1" for i in here.info.values()) and all(i["ok"] == "1" for i in parent.info.values())
    lines.append("  every stream of every form equal to the oracle's: %s   surface stats after the checks: %s" % (ok, here.stats))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "a") as f:
            f.write(text)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
