"""Decoding into views against the parent commit's way of doing the same job: felics_decompress_images_device into a dense buffer, a
device re-layout copy into the surface, synchronise.

    python profiles/tools/decode_views_bench.py [--reps 15] [--scale 1] [--parent-bench PATH] [--bench-runs 3] [--out FILE]

Legs (64 x 64 streams; the pixels of every call of every form are compared with the source images):
  (a) 4 096 gray8 streams into the cells of a 4096 x 4096 mosaic                    (in place, lane form)
  (b) 4 096 RGB8 streams into an N x 3 x 64 x 64 tensor                             (in place: the conversion kernel writes the planes)
  (c) 2 048 RGB8 streams into RGBA surfaces                                         (in place; alpha keeps its value)
  (d) 16 384 gray16 streams into the cells of a pitched 8192-wide surface           (in place, lane form)
  (e) 4 096 gray8 streams into the cells of the mosaic of (a), bottom-up            (scattered: staged, then k_scatter_view)
Forms of a leg: the view call | the dense decode, then one torch copy that re-lays the frames out into the surface, then the
synchronise (the parent), all timed | the dense decode of the same streams alone.
  (f) plain `python bench.py` of a built checkout of the parent commit (--parent-bench: its bench.py) and of this one, alternating
Forms ALTERNATE call by call in one process; a time is the wall-clock median of --reps blocking calls after two warm-up
calls each, the spread is (max - min) / median of a form.  --scale k divides the stream counts by k (a short look)."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--scale", type=int, default=1)
    ap.add_argument("--parent-bench", default=None, help="bench.py of a built checkout of the parent commit: leg (f)")
    ap.add_argument("--bench-runs", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import numpy as np
    import torch

    import felics_amd
    from felics_amd import build, synth

    enc = felics_amd.Encoder(0)
    lines = ["decode_views_bench.py: %d alternating reps, scale 1/%d; source %s" % (a.reps, a.scale, build.source_hash()),
             "device %s, host %s" % (torch.cuda.get_device_name(0), os.uname().nodename)]

    def say(s):
        lines.append(s)
        print(s, flush=True)

    for s in lines:
        print(s, flush=True)

    def alternate(forms):
        for _ in range(2):
            for _, fn, _ in forms:
                fn()
        ts = {name: [] for name, _, _ in forms}
        good = {name: True for name, _, _ in forms}
        for _ in range(a.reps):
            for name, fn, check in forms:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                ts[name].append((time.perf_counter() - t0) * 1e3)
                good[name] = good[name] and check()
        return {k: (statistics.median(v), min(v), max(v)) for k, v in ts.items()}, good

    S = 64
    ok = True

    def leg(tag, what, n, distinct, make_surface, cell_views, relayout, expect):
        """distinct: numpy source images, cycled over n streams.  make_surface() -> torch surface; cell_views(surface) -> n torch
        view tuples; relayout(surface, dense N x 64 x 64 [x 3] tensor) writes the frames into the surface; expect(surface, src) -> bool."""
        nonlocal ok
        streams = enc.compress_images(distinct)
        blob, offs, lens = bytearray(), [], []
        for i in range(n):
            s = streams[i % len(distinct)]
            offs.append(len(blob))
            lens.append(len(s))
            blob += s + bytes(-len(s) % 4)
        d = torch.from_numpy(np.frombuffer(bytes(blob) + bytes(16), np.uint8).copy()).cuda()
        offs, lens = np.asarray(offs, np.uint64), np.asarray(lens, np.uint64)
        src = torch.from_numpy(np.stack([distinct[i % len(distinct)] for i in range(n)])).cuda()
        frame = distinct[0].nbytes
        dense = torch.zeros(n * frame, dtype=torch.uint8, device="cuda")
        wide = distinct[0].dtype == np.uint16  # (16-bit samples live in int16 tensors: the bits are compared)
        src_t = src.view(torch.int16) if wide else src
        dense_t = (dense.view(torch.int16) if wide else dense).view(src.shape)
        surf_v, surf_p = make_surface(), make_surface()
        views = cell_views(surf_v)
        torch.cuda.synchronize()

        def run_view():
            enc.decompress_views_device(d.data_ptr(), offs, lens, views)

        def run_parent():
            enc.decompress_images_device(d.data_ptr(), offs, lens, dense.data_ptr(), dense.numel())
            relayout(surf_p, dense_t)
            torch.cuda.synchronize()

        def run_dense():
            enc.decompress_images_device(d.data_ptr(), offs, lens, dense.data_ptr(), dense.numel())

        def check_view():
            r = expect(surf_v, src_t)
            surf_v.fill_(0x5A5A if wide else 0x5A)
            return r

        def check_parent():
            r = expect(surf_p, src_t)
            surf_p.fill_(0x5A5A if wide else 0x5A)
            return r

        def check_dense():
            r = bool(torch.equal(dense_t, src_t))
            dense.zero_()
            return r

        v0, s0 = enc.decode_view_stats(), enc.decode_stats()
        run_view()
        v1, s1 = enc.decode_view_stats(), enc.decode_stats()
        say("(%s) %s: %d streams; classes %s; forms %s" % (tag, what, n, {k: v1[k] - v0[k] for k in v1},
                                                          {k: s1[k] - s0[k] for k in ("wave8", "lanes8", "wave16", "lanes16", "host")}))
        res, good = alternate([("view call", run_view, check_view), ("dense decode + re-layout copy + sync (the parent)", run_parent, check_parent),
                               ("dense decode alone", run_dense, check_dense)])
        for name, (med, lo, hi) in res.items():
            say("(%s) %-50s median %8.3f ms (min %.3f, max %.3f, spread %.1f %%)  pixels %s"
                % (tag, name, med, lo, hi, (hi - lo) / med * 100, "exact in every call" if good[name] else "WRONG"))
        base = res["view call"][0]
        say("(%s) view call / parent's way = %.3f; view call / dense decode alone = %.3f"
            % (tag, base / res["dense decode + re-layout copy + sync (the parent)"][0], base / res["dense decode alone"][0]))
        ok = ok and all(good.values())
        del d, dense, surf_v, surf_p, src
        torch.cuda.empty_cache()

    def view_of(t, flip=False):
        """the view tuple of a torch tensor (H x W or H x W x 3, one or two bytes a sample); flip: bottom-up"""
        e = t.element_size()
        v = (t.data_ptr(), t.shape[1], t.shape[0], int(t.dim() == 3), int(e == 2), t.stride(0) * e, t.stride(1) * e, t.stride(2) * e if t.dim() == 3 else 0)
        return v if not flip else (v[0] + (v[2] - 1) * v[5],) + v[1:5] + (-v[5],) + v[6:]

    def cells(m, side, flip=False):
        """the S x S cells of a mosaic of side x side cells, in row-major order"""
        return [view_of(m[(c // side) * S:(c // side + 1) * S, (c % side) * S:(c % side + 1) * S], flip) for c in range(side * side)]

    def mosaic_of(m, side, dense_t, flip=False):
        t = dense_t.view(side, side, S, S).permute(0, 2, 1, 3)
        m[:, :side * S].unflatten(0, (side, S)).unflatten(2, (side, S)).copy_(t.flip(1) if flip else t)

    def mosaic_ok(m, side, src_t, flip=False):
        t = src_t.view(side, side, S, S).permute(0, 2, 1, 3)
        return bool(torch.equal(m[:, :side * S].unflatten(0, (side, S)).unflatten(2, (side, S)), t.flip(1) if flip else t))

    g8 = [synth.gray8(S, S, f, "S1") for f in range(64)]
    c8 = [synth.rgb8(S, S, f) for f in range(64)]
    g16 = [synth.gray16(S, S, f) for f in range(64)]
    side8 = max(1, 64 // a.scale)
    n8 = side8 * side8
    leg("a", "gray8 into the cells of a %d x %d mosaic" % (side8 * S, side8 * S), n8, g8,
        lambda: torch.full((side8 * S, side8 * S), 0x5A, dtype=torch.uint8, device="cuda"),
        lambda m: cells(m, side8), lambda m, t: mosaic_of(m, side8, t), lambda m, s: mosaic_ok(m, side8, s))
    nb = max(64, 4096 // a.scale)
    leg("b", "RGB8 into an N x 3 x 64 x 64 tensor", nb, c8,
        lambda: torch.full((nb, 3, S, S), 0x5A, dtype=torch.uint8, device="cuda"),
        lambda m: [view_of(m[i].permute(1, 2, 0)) for i in range(nb)], lambda m, t: m.copy_(t.permute(0, 3, 1, 2)),
        lambda m, s: bool(torch.equal(m, s.permute(0, 3, 1, 2))))
    nc = max(64, 2048 // a.scale)
    leg("c", "RGB8 into RGBA surfaces", nc, c8,
        lambda: torch.full((nc, S, S, 4), 0x5A, dtype=torch.uint8, device="cuda"),
        lambda m: [view_of(m[i][..., :3]) for i in range(nc)], lambda m, t: m[..., :3].copy_(t),
        lambda m, s: bool(torch.equal(m[..., :3], s)) and bool((m[..., 3] == 0x5A).all()))
    side16 = max(1, 128 // a.scale)
    leg("d", "gray16 into the cells of a surface of pitch %d samples" % (side16 * S + 32), side16 * side16, g16,
        lambda: torch.full((side16 * S, side16 * S + 32), 0x5A5A, dtype=torch.int16, device="cuda"),
        lambda m: cells(m, side16), lambda m, t: mosaic_of(m, side16, t),
        lambda m, s: mosaic_ok(m, side16, s) and bool((m[:, side16 * S:] == 0x5A5A).all()))
    leg("e", "gray8 into the cells of the mosaic, bottom-up (scattered)", n8, g8,
        lambda: torch.full((side8 * S, side8 * S), 0x5A, dtype=torch.uint8, device="cuda"),
        lambda m: cells(m, side8, flip=True), lambda m, t: mosaic_of(m, side8, t, flip=True), lambda m, s: mosaic_ok(m, side8, s, flip=True))
    enc.close()

    if a.parent_bench:
        res = {"parent": [], "this": []}
        for _ in range(a.bench_runs):
            for name in ("parent", "this"):
                script = os.path.abspath(a.parent_bench) if name == "parent" else os.path.join(ROOT, "bench.py")
                p = subprocess.run([sys.executable, script], cwd=os.path.dirname(script), capture_output=True, text=True, timeout=300)
                if p.returncode != 0:
                    say("(f) bench.py of the %s commit failed: %s" % (name, p.stderr[-300:]))
                    return 1
                res[name].append(json.loads(p.stdout.strip().splitlines()[-1])["ms_per_step"])
        for name in ("parent", "this"):
            v = res[name]
            say("(f) python bench.py, %-6s commit: ms_per_step %s  median %.3f" % (name, " ".join("%.3f" % x for x in v), statistics.median(v)))
        say("(f) this / parent = %.3f" % (statistics.median(res["this"]) / statistics.median(res["parent"])))
    else:
        say("(f) not measured: no --parent-bench")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
