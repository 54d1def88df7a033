"""Regions into views, mixed shapes in one call, against today's route on one GPU: a window of every frame of a mixed-shape set
into the slices of one N x C x h x w tensor.

    python profiles/tools/region_views.py [--reps 5] [--out FILE]             the measurement (needs the GPU)
    python profiles/tools/region_views.py --figures PARENT_LIB [--out FILE]  appends the kernel figures to FILE (needs no GPU;
                                                                             default profiles/region_views.txt)

Workload: 16 frames, four each of 3840 x 2160, 4096 x 2160, 3840 x 2048 and 3584 x 2160, as gray8, RGB8, gray16 and RGB16 (felics_amd.synth;
RGB16 as region_decode16.py makes it), each set at segment_pixels = 4096 and at the multiple of 4096 that gives a frame K = 64 segments
(63 where the division is exact below it).  Streams and indexes are written by the encoder's indexed batch calls, a call per shape.
The window is 256 x 256 or 1024 x 1024 in the middle of every frame; the targets are the slices t[i] of one 16 x C x h x w tensor
(gray: t[i, 0]; RGB: t[i].permute(1, 2, 0), planar memory).
Routes, alternating in one process, --reps rounds of
    today (seat A) | new | today (seat B)
after one untimed call of each.  `new` is ONE felics_decompress_region_views_device_indexed (16-bit: _indexed16) call on all 16 streams.
`today` is what a caller had before that call existed: the streams grouped by shape, one felics_decompress_regions_device_indexed
(_indexed16) call per shape into a staging buffer of dense crops, and one device copy per crop into its slice of the tensor.  The
dense region calls are untouched by the change that added the new call, so `today` is also the parent commit's behaviour, measured in
the same run.  It sits in two seats of the round: the difference of their medians is the run's own spread, and the margin the new
call is judged by, against the faster of the two seats.  A time is what two device events around the route measure, reported as
median (min .. max).  The tensor is compared with the frames' windows after every route."""
import argparse
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
SHAPES = ((3840, 2160), (4096, 2160), (3840, 2048), (3584, 2160))
PER_SHAPE = 4
WINDOWS = (256, 1024)
KERNELS = ("k_decode8_region", "k_decode16_region", "k_decode8_seg", "k_decode16_seg", "k_seg_status", "k_ycocg8_to_rgb", "k_ycocg16_to_rgb",
           "k_read_headers", "k_read_index_headers")


def figures(parent_lib, out):
    lib = os.path.join(ROOT, "felics_amd", "_build", "libfelics.so")
    tools = os.path.join(ROOT, "profiles", "tools")
    meta = subprocess.run([sys.executable, os.path.join(tools, "kernel_meta.py"), parent_lib, lib], capture_output=True, text=True, check=True).stdout
    keep = [ln[:190] for ln in meta.splitlines() if ln.startswith("#") or ln.startswith("new") or ln.startswith("differs") or ln.startswith("gone")
            or any("felics::%s" % k in ln for k in KERNELS)]
    totals = subprocess.run([sys.executable, os.path.join(tools, "opcodes.py"), "--totals", parent_lib, lib, *KERNELS], capture_output=True, text=True,
                            check=True).stdout
    with open(out, "a") as f:
        f.write("\nKernel figures (profiles/tools/kernel_meta.py PARENT_LIB LIB: vgpr sgpr lds scratch vgpr-spills sgpr-spills; no GPU needed)\n")
        f.write("\n".join(keep) + "\n")
        f.write("\n(profiles/tools/opcodes.py --totals PARENT_LIB LIB, the walks from a checkpoint, their finish and the header kernels)\n")
        f.write(totals)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    ap.add_argument("--figures", default=None, metavar="PARENT_LIB")
    a = ap.parse_args()
    if a.figures:
        return figures(a.figures, a.out or os.path.join(ROOT, "profiles", "region_views.txt"))

    import numpy as np
    import torch

    import felics_amd
    from felics_amd import api, build, synth

    enc = felics_amd.Encoder(0)
    lines = []

    def say(s):
        lines.append(s)
        print(s, flush=True)

    def timed(fn):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0.record()
        fn()
        t1.record()
        torch.cuda.synchronize()
        return t0.elapsed_time(t1)

    def fmt(ts):
        return "%9.2f ms (%.2f .. %.2f, %d calls)" % (statistics.median(ts), min(ts), max(ts), len(ts))

    def frame_of(w, h, f, rgb, wide):
        if not wide:
            return synth.rgb8(w, h, f) if rgb else synth.gray8(w, h, f, "S1")
        g = synth.gray16(w, h, f)
        if not rgb:
            return g
        r = np.clip(g.astype(np.int64) + (g & 3) * 16 - 24, 0, 65535)
        b = np.clip(g.astype(np.int64) - ((g >> 2) & 3) * 16 + 24, 0, 65535)
        return np.stack([r, g, b], -1).astype(np.uint16)

    say("region_views.py: source %s, device %s, %d rounds" % (build.source_hash(), torch.cuda.get_device_name(0), a.reps))
    worst, headline = None, None
    for name, rgb, wide in (("gray8", 0, 0), ("RGB8", 1, 0), ("gray16", 0, 1), ("RGB16", 1, 1)):
        planes, sample = (3 if rgb else 1), (2 if wide else 1)
        tdt = torch.int16 if wide else torch.uint8  # (torch compares int16; the bits are the samples')
        frames = []  # per shape: PER_SHAPE frames on the device
        for w, h in SHAPES:
            fr = np.stack([frame_of(w, h, f, rgb, wide) for f in range(PER_SHAPE)])
            frames.append(torch.from_numpy(fr.view(np.int16) if wide else fr).cuda())
        for k64 in (False, True):
            groups = []  # per shape: (w, h, seg, d_out, offs, lens, d_idx, ioffs, ilens)
            for (w, h), fr in zip(SHAPES, frames):
                seg = ((w * h + 63) // 64 + 4095) // 4096 * 4096 if k64 else 4096
                cap = PER_SHAPE * ((fr[0].numel() * sample * 5 // 4 + 64 + 15) // 16 * 16)
                d_out = torch.empty(cap, dtype=torch.uint8, device="cuda")
                if wide:
                    icap = 64
                    for _ in range(2):  # the two-call pattern: the second call has idx_total bytes
                        d_idx = torch.empty(icap, dtype=torch.uint8, device="cuda")
                        torch.cuda.synchronize()
                        rc, offs, lens, ioffs, ilens, icap = enc.compress_batch_device_indexed16_raw(fr.data_ptr(), PER_SHAPE, w, h, rgb, d_out.data_ptr(),
                                                                                                     cap, seg, d_idx.data_ptr(), icap)
                        if rc == 0:
                            break
                    assert rc == 0, rc
                else:
                    isize = api.index_size(w, h, rgb, 0, seg)
                    d_idx = torch.empty(PER_SHAPE * isize, dtype=torch.uint8, device="cuda")
                    torch.cuda.synchronize()
                    offs, lens = enc.compress_batch_device_indexed(fr.data_ptr(), PER_SHAPE, w, h, rgb, 0, d_out.data_ptr(), cap, seg, d_idx.data_ptr(),
                                                                   PER_SHAPE * isize)
                    ioffs = np.arange(PER_SHAPE, dtype=np.uint64) * np.uint64(isize)
                    ilens = np.full(PER_SHAPE, isize, np.uint64)
                assert d_idx.data_ptr() % 64 == 0
                groups.append((w, h, seg, d_out, offs, lens, d_idx, ioffs, ilens))
            # the mixed call's arrays: one base per kind, every stream and index by its distance from it
            base_s, base_i = min(g[3].data_ptr() for g in groups), min(g[6].data_ptr() for g in groups)
            m_offs = np.concatenate([np.asarray(g[4], np.uint64) + np.uint64(g[3].data_ptr() - base_s) for g in groups])
            m_lens = np.concatenate([np.asarray(g[5], np.uint64) for g in groups])
            m_ioffs = np.concatenate([np.asarray(g[7], np.uint64) + np.uint64(g[6].data_ptr() - base_i) for g in groups])
            m_ilens = np.concatenate([np.asarray(g[8], np.uint64) for g in groups])
            n = len(m_offs)
            say("16 %s frames of four shapes, %s, indexes %.1f MB" % (name, "K = 64 (segments of %s px)" % ", ".join(str(g[2]) for g in groups)
                                                                      if k64 else "segment 4096 px", float(m_ilens.sum()) / 1e6))
            for side in WINDOWS:
                target = torch.zeros((n, planes, side, side), dtype=tdt, device="cuda")
                staging = torch.zeros((PER_SHAPE, side, side, planes), dtype=tdt, device="cuda")
                wins = [((w - side) // 2, (h - side) // 2) for w, h in SHAPES for _ in range(PER_SHAPE)]
                want = torch.stack([frames[i // PER_SHAPE][i % PER_SHAPE][y:y + side, x:x + side].reshape(side, side, planes).permute(2, 0, 1)
                                    for i, (x, y) in enumerate(wins)])

                class U16:  # (uint16 samples in an int16 tensor: not every torch build has a uint16 dtype on the device)
                    def __init__(self, t):
                        self.__cuda_array_interface__ = {"shape": tuple(t.shape), "typestr": "<u2", "data": (t.data_ptr(), False), "version": 2,
                                                         "strides": tuple(2 * v for v in t.stride())}

                def slice_of(i):
                    t = target[i].permute(1, 2, 0) if rgb else target[i, 0]
                    return U16(t) if wide else t

                arrays = [slice_of(i) for i in range(n)]
                regions = [(i, x, y, side, side) for i, (x, y) in enumerate(wins)]

                def new():
                    target.zero_()
                    call = enc.decompress_region_arrays_device_indexed16 if wide else enc.decompress_region_arrays_device_indexed
                    t = timed(lambda: call(base_s, m_offs, m_lens, base_i, m_ioffs, m_ilens, regions, arrays))
                    assert torch.equal(target, want)
                    return t

                def today():
                    target.zero_()

                    def route():
                        for gi, (w, h, seg, d_out, offs, lens, d_idx, ioffs, ilens) in enumerate(groups):
                            x, y = (w - side) // 2, (h - side) // 2
                            reqs = [(i, x, y, side, side) for i in range(PER_SHAPE)]
                            if wide:
                                enc.decompress_regions_device_indexed16(d_out.data_ptr(), offs, lens, d_idx.data_ptr(), ioffs, ilens, reqs,
                                                                        staging.data_ptr(), staging.numel() * 2)
                            else:
                                enc.decompress_regions_device_indexed(d_out.data_ptr(), offs, lens, d_idx.data_ptr(), int(ilens[0]), reqs,
                                                                      staging.data_ptr(), staging.numel())
                            for i in range(PER_SHAPE):  # one device copy per crop into its place
                                target[gi * PER_SHAPE + i].copy_(staging[i].permute(2, 0, 1))

                    t = timed(route)
                    assert torch.equal(target, want)
                    return t

                today()
                new()
                ts = {"A": [], "B": [], "new": []}
                stats_name = "region16_view_stats" if wide else "region_view_stats"
                for _ in range(a.reps):
                    ts["A"].append(today())
                    before = getattr(enc, stats_name)()
                    ts["new"].append(new())
                    after = getattr(enc, stats_name)()
                    ts["B"].append(today())
                cnt = {key: after[key] - before[key] for key in after if key not in ("plane_bytes", "table_bytes")}
                ma, mb, m = statistics.median(ts["A"]), statistics.median(ts["B"]), statistics.median(ts["new"])
                spread = abs(ma - mb)
                over = m - (min(ma, mb) + spread)  # against the FASTER seat: not slower than today's route by more than the spread
                say("  %4d x %4d window per frame" % (side, side))
                say("    today: a region call per shape + a copy per crop, seat A : %s" % fmt(ts["A"]))
                say("    today: a region call per shape + a copy per crop, seat B : %s   spread of the two medians %.3f ms (%.2f %%)"
                    % (fmt(ts["B"]), spread, 100 * spread / min(ma, mb)))
                say("    new: one call into the tensor's slices                  : %s   %.3f of today's route   %s"
                    % (fmt(ts["new"]), m / min(ma, mb), "within the margin" if over <= 0 else "SLOWER than today + spread by %.3f ms" % over))
                say("      counters of one call: %s, plane_bytes %d" % (cnt, after["plane_bytes"]))
                if worst is None or over > worst[0]:
                    worst = (over, name, "K = 64" if k64 else "segment 4096", side)
                if (name, k64, side) == ("gray16", False, 256):
                    headline = (m, min(ma, mb))
                del target, staging, want
            del groups
            torch.cuda.empty_cache()
        del frames
        torch.cuda.empty_cache()
    say("acceptance (the new call not slower than today's route by more than the spread, in any case): %s"
        % ("met" if worst[0] <= 0 else "MISSED: %s, %s, %d x %d window, by %.3f ms" % (worst[1], worst[2], worst[3], worst[3], worst[0])))
    say("headline (16 gray16 frames, segment 4096, 256 x 256 windows): %.2f ms in one call against %.2f ms today" % headline)
    enc.close()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
