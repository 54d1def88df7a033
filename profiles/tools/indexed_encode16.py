"""Restart index for 16-bit streams on one GPU: what writing it costs the encoder.

    python profiles/tools/indexed_encode16.py [--rounds 5] [--parent-lib LIB] [--trace] [--out FILE]

Workloads: 16 synthetic 3840 x 2160 gray16 frames (synth.gray16) and 4 RGB16 frames (the same with two chroma offsets), at
segment_pixels = 4096 x {127, 32, 8} (K = 16, 64, 254).  felics_compress_batch_device with depth 16 (blocking, unindexed) against
felics_compress_batch_device_indexed16 into a buffer of idx_total bytes.  One untimed call of every form first; then --rounds rounds of
one unindexed call followed by one indexed call per K, so the forms alternate in one process.  A time is what two device events
around the blocking call measure, reported as median (min .. max).  After EVERY indexed call the streams are compared with the unindexed
call's and the indexes with felics_index16_build's of those streams (built once, on sixteen host threads; one build is timed alone,
for scale), on the device.
--parent-lib LIB: the unindexed call of this build against the same call of LIB (the parent commit's libfelics.so), in child processes
of one library each that alternate, --ab-pairs pairs of them.
--trace: per workload one child under `rocprofv3 --kernel-trace` (every K, four calls each): the time of the index kernels per call.
--trace-only: nothing but that."""
import argparse
import collections
import concurrent.futures
import csv
import glob
import os
import re
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
W, H = 3840, 2160
SEGS = (4096 * 127, 4096 * 32, 4096 * 8)
WORKLOADS = (("16 gray16 4K frames", 16, 0), ("4 RGB16 4K frames", 4, 1))


def frame_of(f, rgb):
    import numpy as np

    from felics_amd import synth

    g = synth.gray16(W, H, f)
    if not rgb:
        return g
    r = np.clip(g.astype(np.int64) + (g & 3) * 16 - 24, 0, 65535)
    b = np.clip(g.astype(np.int64) - ((g >> 2) & 3) * 16 + 24, 0, 65535)
    return np.stack([r, g, b], -1).astype(np.uint16)


def timed(fn):
    import torch

    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0.record()
    fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1)


def fmt(ts):
    return "%8.3f ms (%.3f .. %.3f, %d calls)" % (statistics.median(ts), min(ts), max(ts), len(ts))


def device_frames(n, rgb):
    import numpy as np
    import torch

    frames = torch.from_numpy(np.stack([frame_of(f, rgb) for f in range(n)]).view(np.int16)).cuda()
    cap = n * ((frames[0].numel() * 2 * 5 // 4 + 64 + 15) // 16 * 16)
    return frames, torch.empty(cap, dtype=torch.uint8, device="cuda"), cap


def ab_child(calls):
    """the unindexed call of whichever library FELICS_LIB_PATH names: its median over `calls` calls, one line"""
    import torch

    import felics_amd

    enc = felics_amd.Encoder(0)
    frames, d_out, cap = device_frames(16, 0)
    torch.cuda.synchronize()
    call = lambda: enc.compress_batch_device(frames.data_ptr(), 16, W, H, 0, 1, d_out.data_ptr(), cap)
    call()
    ts = [timed(call) for _ in range(calls)]
    print("AB %.4f %.4f %.4f" % (statistics.median(ts), min(ts), max(ts)))


def trace_child(n, rgb):
    import torch

    import felics_amd

    enc = felics_amd.Encoder(0)
    frames, d_out, cap = device_frames(n, rgb)
    d_idx = torch.empty(64, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    for seg in SEGS:
        for _ in range(5):  # (the first call learns idx_total and is not counted: four full calls per K)
            rc, _, _, _, _, total = enc.compress_batch_device_indexed16_raw(frames.data_ptr(), n, W, H, rgb, d_out.data_ptr(), cap, seg, d_idx.data_ptr(),
                                                                           d_idx.numel())
            if rc == -8 and total:
                d_idx = torch.empty(total, dtype=torch.uint8, device="cuda")
                torch.cuda.synchronize()
            elif rc:
                raise SystemExit("the call failed: %d" % rc)
    print("workload done")


def trace(limit, n, rgb):
    """per K the index kernels' times per call, from the kernel trace of trace_child"""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__), "--trace-child",
               "%d,%d" % (n, rgb)]
        p = subprocess.run(cmd, cwd=d, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=limit)
        if p.returncode != 0 or "workload done" not in p.stdout:
            sys.stdout.write(p.stdout[-3000:])
            raise SystemExit("the traced run failed (exit %d): nothing more is started" % p.returncode)
        rows = [r for f in glob.glob(d + "/**/*kernel_trace.csv", recursive=True) for r in csv.DictReader(open(f)) if "felics" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    # a call's first kernel is k_wide_count (gray16) or k_rgb16_to_planes; five calls per K, the first of them the short one
    out = []
    for r in rows:
        if ("k_rgb16_to_planes" if rgb else "k_wide_count") in r["Kernel_Name"]:
            out.append([])
        if out:
            out[-1].append(r)
    lines = []
    if len(out) != 5 * len(SEGS):
        return ["  (%d calls in the trace, %d expected: not evaluated)" % (len(out), 5 * len(SEGS))]
    for i, seg in enumerate(SEGS):
        calls = out[5 * i + 1:5 * i + 5]
        sums = collections.Counter()
        for c in calls:
            for r in c:
                name = re.search(r"k_[a-z0-9_]+", r["Kernel_Name"]).group(0)
                sums[name if name.startswith("k_wide_index") else "the unindexed call's kernels"] += (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e6
        k = (W * H + seg - 1) // seg
        lines.append("  K = %3d, %d calls, kernel time per call: %s" % (k, len(calls), ", ".join("%s %.3f ms" % (n, v / len(calls)) for n, v in sorted(sums.items()))))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--ab-pairs", type=int, default=4)
    ap.add_argument("--ab-calls", type=int, default=12)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--limit", type=int, default=300, help="seconds per child process")
    ap.add_argument("--ab-child", action="store_true")
    ap.add_argument("--trace-child", default=None)
    ap.add_argument("--trace-only", action="store_true", help="skip the timed part and the comparison with the parent")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.ab_child:
        return ab_child(a.ab_calls)
    if a.trace_child:
        return trace_child(*(int(v) for v in a.trace_child.split(",")))

    import numpy as np
    import torch

    import felics_amd
    from felics_amd import api, build

    enc = felics_amd.Encoder(0)
    lines = []

    def say(s):
        lines.append(s)
        print(s, flush=True)

    say("indexed_encode16.py: source %s, device %s, %d rounds (one unindexed call, one indexed call per K)"
        % (build.source_hash(), torch.cuda.get_device_name(0), a.rounds))
    pool = concurrent.futures.ThreadPoolExecutor(16)
    for name, n, rgb in () if a.trace_only else WORKLOADS:
        frames, d_out, cap = device_frames(n, rgb)
        d_ref = torch.empty_like(d_out)
        torch.cuda.synchronize()
        offs, lens = enc.compress_batch_device(frames.data_ptr(), n, W, H, rgb, 1, d_ref.data_ptr(), cap)
        host = d_ref.cpu().numpy()
        streams = [host[int(o):int(o) + int(l)].tobytes() for o, l in zip(offs, lens)]
        t0 = time.perf_counter()
        one = api.index16_build(streams[0], SEGS[1])
        host_build_ms = (time.perf_counter() - t0) * 1e3
        want = {}
        for seg in SEGS:
            indexes = list(pool.map(lambda s: api.index16_build(s, seg), streams))
            want[seg] = (torch.from_numpy(np.frombuffer(b"".join(indexes), np.uint8).copy()).cuda(), [len(x) for x in indexes])
        assert want[SEGS[1]][1][0] == len(one)
        bits = 8.0 * float(sum(int(x) for x in lens)) / frames.numel()
        say("%s (%.1f MPix, %.2f bits per sample)" % (name, n * W * H / 1e6, bits))
        d_idx = {seg: torch.empty(sum(want[seg][1]), dtype=torch.uint8, device="cuda") for seg in SEGS}
        torch.cuda.synchronize()

        def plain():
            enc.compress_batch_device(frames.data_ptr(), n, W, H, rgb, 1, d_out.data_ptr(), cap)

        def indexed(seg):
            d_out.zero_()
            d_idx[seg].fill_(0x5A)
            res = []
            t = timed(lambda: res.append(enc.compress_batch_device_indexed16_raw(frames.data_ptr(), n, W, H, rgb, d_out.data_ptr(), cap, seg,
                                                                                 d_idx[seg].data_ptr(), d_idx[seg].numel())))
            rc, o2, l2, ioffs, ilens, total = res[0]
            assert rc == 0 and total == d_idx[seg].numel() and [int(x) for x in ilens] == want[seg][1], (rc, total)
            assert (o2 == offs).all() and (l2 == lens).all()
            for o, l in zip(offs, lens):
                assert torch.equal(d_out[int(o):int(o) + int(l)], d_ref[int(o):int(o) + int(l)])
            assert torch.equal(d_idx[seg], want[seg][0])  # (the indexes are multiples of 64 long: back to back on both sides)
            return t

        timed(plain)
        rows = {}
        for seg in SEGS:
            before = enc.index16_emit_stats()
            indexed(seg)
            rows[seg] = enc.index16_emit_stats()["rows_written"] - before["rows_written"]
        t_plain, t_idx = [], {seg: [] for seg in SEGS}
        for _ in range(a.rounds):
            t_plain.append(timed(plain))
            for seg in SEGS:
                t_idx[seg].append(indexed(seg))
        base = statistics.median(t_plain)
        say("  unindexed, blocking                      : %s" % fmt(t_plain))
        for seg in SEGS:
            m = statistics.median(t_idx[seg])
            k = (W * H + seg - 1) // seg
            say("  indexed, segment %6d px (K = %3d)     : %s  + %.3f ms (%+.0f %%)" % (seg, k, fmt(t_idx[seg]), m - base, 100 * (m - base) / base))
            say("      indexes %d bytes in all (largest %d; felics_index16_size_max %d), %d rows" % (sum(want[seg][1]), max(want[seg][1]),
                                                                                                    api.index16_size_max(W, H, rgb, seg), rows[seg]))
        m = statistics.median(t_idx[SEGS[1]])
        say("  felics_index16_build of ONE of these streams on the host (K = 64): %.0f ms; of all %d, one after the other: %.0f ms = %.0fx the whole "
            "indexed call, %.0fx what the index adds to it" % (host_build_ms, n, host_build_ms * n, host_build_ms * n / m, host_build_ms * n / max(m - base, 1e-3)))
        del frames, d_out, d_ref, d_idx, want
        torch.cuda.empty_cache()
    enc.close()
    if a.parent_lib and not a.trace_only:
        say("the unindexed call (16 gray16 4K frames), this build against the parent's library, child processes alternating, %d calls each:" % a.ab_calls)
        res = {"parent": [], "this build": []}
        for _ in range(a.ab_pairs):
            for who in ("parent", "this build"):
                env = dict(os.environ)
                if who == "parent":
                    env["FELICS_LIB_PATH"] = os.path.abspath(a.parent_lib)
                p = subprocess.run([sys.executable, os.path.abspath(__file__), "--ab-child", "--ab-calls", str(a.ab_calls)], env=env, stdout=subprocess.PIPE,
                                   stderr=subprocess.STDOUT, text=True, timeout=a.limit)
                got = [ln for ln in p.stdout.splitlines() if ln.startswith("AB ")]
                if p.returncode != 0 or not got:
                    sys.stdout.write(p.stdout[-3000:])
                    raise SystemExit("a child of the comparison failed (exit %d): nothing more is started" % p.returncode)
                res[who].append(float(got[0].split()[1]))
        for who in res:
            say("  %-10s: medians of the processes %s ms -> %.3f ms" % (who, " ".join("%.3f" % v for v in res[who]), statistics.median(res[who])))
        d = statistics.median(res["this build"]) / statistics.median(res["parent"]) - 1
        say("  this build / parent - 1 = %+.1f %% (the project quotes +- 4 %% from box to box) -- %s" % (100 * d, "within" if abs(d) <= 0.04 else "OUTSIDE"))
    if a.trace:
        for name, n, rgb in WORKLOADS:
            say("index kernels under rocprofv3 --kernel-trace (%s):" % name)
            for ln in trace(a.limit, n, rgb):
                say(ln)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
