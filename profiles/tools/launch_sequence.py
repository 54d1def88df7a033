"""Same launches: the kernels this build queues for a fixed small workload against another build of the library (the parent commit's).

    python profiles/tools/launch_sequence.py --parent-lib PARENT/libfelics.so [--out FILE]

Runs ON THE GPU BOX.  Workload, in a child process per library (FELICS_LIB_PATH names the other build) under
`rocprofv3 --kernel-trace` (no counters; the program after `--`):
  encode: the three smoke() images through compress; a 3-frame gray8 submit / wait; one compress_images_device call over two gray8
          shapes, one RGB8, two gray16 shapes and one RGB16; one compress_views_device call with a pitched gray8 view and an RGBA view;
  decode: one decompress_images_device call over the mixed call's streams and one decompress_batch_device call over the submit's.
Run 1, default settings, encode + decode: the multiset of (kernel, grid, workgroup) must be equal for the two libraries.
Run 2, FELICS_SERIAL=1 FELICS_LANES=1 (one lane, one stream: start order = launch order), encode only: the ordered sequence must be
equal as well.  This process never opens the GPU; every traced run has a time limit, and nothing is started after one that failed.
Exit status 0 when both comparisons hold."""
import argparse
import collections
import csv
import difflib
import glob
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def child(part):
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch

    import felics_amd
    from felics_amd import api, synth

    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a)).cuda()

    def rgb16(w, h, f):
        return np.stack([synth.gray16(w, h, 3 * f + c) for c in range(3)], axis=-1)

    cap = 64 << 20
    with felics_amd.Encoder(0) as enc:
        for img in (synth.gray8(640, 360, 0, "S1"), synth.rgb8(320, 180, 0), synth.gray16(320, 180, 0)):
            enc.compress(img)
        frames = dev(np.stack([synth.gray8(640, 360, f, "S1") for f in range(3)]))
        out_b = torch.zeros(cap, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        offs_b, lens_b = enc.wait_batch(enc.submit_batch_device(frames.data_ptr(), 3, 640, 360, 0, 0, out_b.data_ptr(), cap))
        mixed = [dev(synth.gray8(640, 360, 1, "S1")), dev(synth.gray8(600, 350, 2, "S1")), dev(synth.rgb8(320, 180, 1)),
                 dev(synth.gray16(320, 180, 1)), dev(synth.gray16(300, 170, 2)), dev(rgb16(160, 90, 0))]
        descs = [(t.data_ptr(), t.shape[1], t.shape[0], int(t.dim() == 3), int(t.dtype != torch.uint8)) for t in mixed]
        out_m = torch.zeros(cap, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        offs_m, lens_m = enc.compress_images_device(descs, out_m.data_ptr(), cap)
        wide = dev(synth.gray8(800, 360, 3, "S1"))
        rgba = dev(np.concatenate([synth.rgb8(320, 180, 2), np.full((180, 320, 1), 255, np.uint8)], axis=-1))
        out_v = torch.zeros(cap, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        enc.compress_views_device([api.view_of_array(wide[:, 80:720]), api.view_of_array(rgba[..., :3])], out_v.data_ptr(), cap)
        if part == "all":
            px = torch.zeros(cap, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            enc.decompress_images_device(out_m.data_ptr(), offs_m, lens_m, px.data_ptr(), cap)
            enc.decompress_batch_device(out_b.data_ptr(), offs_b, lens_b, px.data_ptr(), cap)
        torch.cuda.synchronize()
    print("workload done")


def trace(lib, part, serial, limit):
    """[(kernel, grid, workgroup)] of the library's kernels in start order"""
    env = dict(os.environ)
    if lib:
        env["FELICS_LIB_PATH"] = os.path.abspath(lib)
    if serial:
        env.update(FELICS_SERIAL="1", FELICS_LANES="1")
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__), "--child", part]
        p = subprocess.run(cmd, env=env, cwd=d, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=limit)
        if p.returncode != 0 or "workload done" not in p.stdout:
            sys.stdout.write(p.stdout[-3000:])
            raise SystemExit("the traced run of %s failed (exit %d): nothing more is started" % (lib or "this build", p.returncode))
        files = glob.glob(d + "/**/*kernel_trace.csv", recursive=True)
        if not files:
            raise SystemExit("no kernel trace was written")
        rows = [r for f in files for r in csv.DictReader(open(f)) if "felics" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    return [(r["Kernel_Name"], "x".join(r["Grid_Size_" + a] for a in "XYZ"), "x".join(r["Workgroup_Size_" + a] for a in "XYZ")) for r in rows]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", default=None)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--limit", type=int, default=240, help="seconds per traced run")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.child:
        return child(a.child)
    if not a.parent_lib:
        ap.error("--parent-lib is needed")
    lines = ["launch_sequence.py: this build against the library given as --parent-lib, kernels of the library only (rocprofv3 --kernel-trace)"]
    ok = True
    here, parent = trace(None, "all", False, a.limit), trace(a.parent_lib, "all", False, a.limit)
    ca, cb = collections.Counter(here), collections.Counter(parent)
    same = ca == cb
    ok = ok and same
    lines.append("run 1, default settings, encode + decode: %d / %d launches, %d distinct (kernel, grid, workgroup); multisets equal: %s"
                 % (len(here), len(parent), len(ca), same))
    for k in sorted(set(ca) | set(cb)):
        if ca[k] != cb[k]:
            lines.append("  this build %d, parent %d: %s grid %s workgroup %s" % (ca[k], cb[k], k[0], k[1], k[2]))
    here, parent = trace(None, "encode", True, a.limit), trace(a.parent_lib, "encode", True, a.limit)
    same = here == parent
    ok = ok and same
    lines.append("run 2, FELICS_SERIAL=1 FELICS_LANES=1, encode calls: %d / %d launches; ordered sequences equal: %s" % (len(here), len(parent), same))
    fmt = ["%s grid %s workgroup %s" % k for k in here], ["%s grid %s workgroup %s" % k for k in parent]
    lines += ["  " + l for l in difflib.unified_diff(fmt[1], fmt[0], "parent", "this build", lineterm="", n=1)] or ["  (diff of the two sequences: empty)"]
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
