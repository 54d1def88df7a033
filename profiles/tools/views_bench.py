"""Views against the parent commit's way of doing the same job: re-layout to dense frames, synchronise, felics_compress_images_device.

    python profiles/tools/views_bench.py [--reps 15] [--parent-bench PATH] [--bench-runs 3] [--out profiles/views.txt]

Legs (every stream of every leg is digest-checked against the CPU oracle of the dense copy first):
  (a) 64 S1 gray8 windows of 3840 x 2160 inside 4096 x 2304 surfaces: the view call | .contiguous() + synchronise + the dense
      call, all timed | the dense frames alone
  (b) 64 RGBA 1920 x 1080 surfaces read as RGB: the view call | [..., :3].contiguous() + synchronise + the dense call
  (c) the same frames planar (C x H x W): the view call | permute(1, 2, 0).contiguous() + synchronise + the dense call
  (d) 64 gray8 windows of 1919 x 1081 at pitch 2048 (every row has a 16-pixel group that straddles its end) | their dense copies
  Every leg also times the dense frames through the VIEW call (class dense): the same entry point and Python marshalling as the
  view call, so that ratio compares the kernels alone.
  (e) plain `python bench.py` of a built checkout of the parent commit (--parent-bench: its bench.py) and of this one
Forms of a leg ALTERNATE call by call on one box (a comparison across boxes or runs measures the box); a time is the
wall-clock median of --reps blocking calls after two warm-up calls each, the spread is (max - min) / median of a form.
Also reported: how long the producer of tests/test_views.py::test_ready_event keeps its event pending."""
import argparse
import hashlib
import json
import os
import statistics
import subprocess
import sys
import time
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--parent-bench", default=None, help="bench.py of a built checkout of the parent commit: leg (e)")
    ap.add_argument("--bench-runs", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import numpy as np
    import torch

    import felics_amd
    from felics_amd import build, synth_torch
    from tests import oracle_lib

    oracle = oracle_lib.load()
    enc = felics_amd.Encoder(0)
    N = a.frames
    lines = ["views_bench.py: %d frames per leg, %d alternating reps; source %s" % (N, a.reps, build.source_hash()),
             "device %s, lanes %d, host %s" % (torch.cuda.get_device_name(0), enc.lane_count(), os.uname().nodename)]

    def say(s):
        lines.append(s)
        print(s, flush=True)

    for s in lines:
        print(s, flush=True)

    def digests(out, offs, lens):
        host = out.cpu().numpy()
        return [hashlib.sha256(host[int(o):int(o) + int(n)].tobytes()).hexdigest() for o, n in zip(offs, lens)]

    def oracle_digests(dense_tensors):
        imgs = [t.cpu().numpy() for t in dense_tensors]
        with ThreadPoolExecutor(16) as pool:
            return list(pool.map(lambda im: hashlib.sha256(oracle.compress(np.ascontiguousarray(im))).hexdigest(), imgs))

    def alternate(forms):
        """forms = [(name, fn)]: two warm-up rounds, then --reps rounds of every form in turn; (median, min, max) ms per form."""
        for _ in range(2):
            for _, fn in forms:
                fn()
        ts = {name: [] for name, _ in forms}
        for _ in range(a.reps):
            for name, fn in forms:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                ts[name].append((time.perf_counter() - t0) * 1e3)
        return {k: (statistics.median(v), min(v), max(v)) for k, v in ts.items()}

    def report(leg, what, res, base):
        for name, (med, lo, hi) in res.items():
            say("(%s) %-46s median %7.3f ms (min %.3f, max %.3f, spread %.1f %%)" % (leg, name, med, lo, hi, (hi - lo) / med * 100))
        for name, (med, _, _) in res.items():
            if name != base:
                say("(%s) %s: %s / %s = %.3f" % (leg, what, base, name, res[base][0] / med))

    def leg(tag, what, views_of, surfaces, relayout, color):
        """views_of(surface) -> the torch view to encode; relayout(view) -> a dense tensor (the parent's way)."""
        tviews = [views_of(s) for s in surfaces]
        dense = [relayout(v) for v in tviews]
        torch.cuda.synchronize()
        h, w = dense[0].shape[:2]
        cap = sum(d.numel() * 5 // 4 + 96 for d in dense) + 4096
        out_v = torch.zeros(cap, dtype=torch.uint8, device="cuda")
        out_d = torch.zeros(cap, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        vt = [felics_amd.api.view_of_array(v) for v in tviews]

        def run_view():
            return enc.compress_views_device(vt, out_v.data_ptr(), cap)

        def run_relayout():
            d = [relayout(v) for v in tviews]
            torch.cuda.synchronize()
            return enc.compress_images_device([(t.data_ptr(), w, h, color, 0) for t in d], out_d.data_ptr(), cap)

        def run_dense():
            return enc.compress_images_device([(t.data_ptr(), w, h, color, 0) for t in dense], out_d.data_ptr(), cap)

        dt = [felics_amd.api.view_of_array(t) for t in dense]

        def run_dense_views():  # (the same entry point and argument marshalling as the view call, the dense class's kernels)
            return enc.compress_views_device(dt, out_d.data_ptr(), cap)

        want = oracle_digests(dense)
        st0 = enc.view_stats()
        ok_v = digests(out_v, *run_view()) == want
        st1 = enc.view_stats()
        ok_r = digests(out_d, *run_relayout()) == want
        ok_d = digests(out_d, *run_dense()) == want
        say("(%s) %s: %d x %dx%d; streams equal the oracle's: view call %s, re-layout %s, dense %s; views in place %d, gathered %d, bytes staged %d"
            % (tag, what, len(dense), w, h, ok_v, ok_r, ok_d, st1["in_place"] - st0["in_place"], st1["gathered"] - st0["gathered"],
               st1["bytes_staged"] - st0["bytes_staged"]))
        res = alternate([("view call", run_view), ("re-layout + sync + dense call (the parent)", run_relayout), ("dense frames alone", run_dense),
                         ("dense frames alone, through the view call", run_dense_views)])
        report(tag, "ratios", res, "view call")
        return ok_v and ok_r and ok_d

    ok = True
    # (a) pitched 4K windows
    surf = [torch.zeros((2304, 4096), dtype=torch.uint8, device="cuda") for _ in range(N)]
    for f, s in enumerate(surf):
        s[100:2260, 128:3968] = synth_torch.gray8(3840, 2160, f, "S1")
    ok &= leg("a", "gray8 S1 windows of 4096 x 2304 surfaces", lambda s: s[100:2260, 128:3968], surf, lambda v: v.contiguous(), 0)
    del surf
    # (b) RGBA -> RGB, (c) planar
    rgb = [synth_torch.rgb8(1920, 1080, f) for f in range(N)]
    rgba = [torch.cat([t, torch.full((1080, 1920, 1), 255, dtype=torch.uint8, device="cuda")], dim=2).contiguous() for t in rgb]
    ok &= leg("b", "RGBA surfaces read as RGB", lambda s: s[..., :3], rgba, lambda v: v.contiguous(), 1)
    del rgba
    chw = [t.permute(2, 0, 1).contiguous() for t in rgb]
    ok &= leg("c", "planar C x H x W frames", lambda s: s.permute(1, 2, 0), chw, lambda v: v.contiguous(), 1)
    del chw, rgb
    # (d) every row has a straddling group
    surf = [torch.zeros((1081, 2048), dtype=torch.uint8, device="cuda") for _ in range(N)]
    for f, s in enumerate(surf):
        s[:, 64:1983] = synth_torch.gray8(1919, 1081, f, "S1")
    ok &= leg("d", "gray8 S1 windows of 1919 x 1081 at pitch 2048", lambda s: s[:, 64:1983], surf, lambda v: v.contiguous(), 0)
    del surf
    torch.cuda.empty_cache()

    # the producer of test_ready_event: how long its event stays pending
    side = torch.cuda.Stream()
    big = torch.zeros(1 << 26, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    with torch.cuda.stream(side):
        for _ in range(600):
            big.add_(1.0)
        ev = torch.cuda.Event()
        ev.record(side)
    t1 = time.perf_counter()
    ev.synchronize()
    say("ready-event producer (600 passes over 256 MB): enqueued in %.1f ms, its event fired %.1f ms after the first launch"
        % ((t1 - t0) * 1e3, (time.perf_counter() - t0) * 1e3))
    del big
    enc.close()

    # (e) the plain bench, parent's library and this one alternating (a process each)
    if a.parent_bench:
        res = {"parent": [], "this": []}
        for _ in range(a.bench_runs):
            for name in ("parent", "this"):
                script = os.path.abspath(a.parent_bench) if name == "parent" else os.path.join(ROOT, "bench.py")
                p = subprocess.run([sys.executable, script], cwd=os.path.dirname(script), capture_output=True, text=True, timeout=300)
                if p.returncode != 0:
                    say("(e) bench.py of the %s commit failed: %s" % (name, p.stderr[-300:]))
                    return 1
                res[name].append(json.loads(p.stdout.strip().splitlines()[-1])["ms_per_step"])
        for name in ("parent", "this"):
            v = res[name]
            say("(e) python bench.py, %-6s commit: ms_per_step %s  median %.3f" % (name, " ".join("%.3f" % x for x in v), statistics.median(v)))
        say("(e) this / parent = %.3f" % (statistics.median(res["this"]) / statistics.median(res["parent"])))
    else:
        say("(e) not measured: no --parent-bench")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
