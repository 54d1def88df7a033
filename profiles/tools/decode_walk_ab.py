"""The GPU decoders of this build, wave per stream and lane per stream, against another build of the library (the parent commit's), call by call.

    python profiles/tools/decode_walk_ab.py --parent-lib PARENT/libfelics.so [--parent-source HASH] [--reps 15] [--out FILE]

Workloads, each one blocking decode call of well under a second, in the wave form (FELICS_TEST_DECODE_LANES=0 and
FELICS_TEST_DECODE16_LANES=0 around the call):
  gray8     64 gray8 S1 streams of 512 x 512, felics_decompress_batch_device          k_decode8<DecUniform>
  rgb8      64 RGB8 streams of 512 x 512                                               k_decode8<DecUniform>, three planes
  gray16    64 gray16 streams of 512 x 512                                             k_decode16<DecUniform>
  rgb16     64 RGB16 streams of 256 x 256                                              k_decode16<DecUniform>, three planes
  pitched8  the gray8 streams into 512 x 512 views of pitch 576, felics_decompress_views_device   k_decode8<DecPitched>
  mixed8    the gray8 streams through felics_decompress_images_device                  k_decode8<DecMixed>
  mixed16   the gray16 streams through felics_decompress_images_device                 k_decode16<DecMixed>
  indexed   one 2048 x 2048 gray8 S1 stream, indexed at segment 32 768                 k_decode8_seg
  indexed_rgb  one 1024 x 1024 RGB8 stream, indexed at segment 32 768                  k_decode8_seg, three planes
  regions   64 windows of 256 x 256 at seeded positions over the `indexed` stream, felics_decompress_regions_device_indexed   k_decode8_region
  indexed_views  the `indexed` stream into a 2048 x 2048 view of pitch 2 112, felics_decompress_views_device_indexed   k_decode8_seg_views
  indexed16      one 1024 x 1024 gray16 stream, its index built on the host at segment 32 768, felics_decompress_batch_device_indexed_wide   k_decode16_seg
  indexed16_rgb  one 512 x 512 RGB16 stream, indexed at segment 8 192                  k_decode16_seg, three planes
  regions16      64 windows of 256 x 256 at seeded positions over the `indexed16` stream, felics_decompress_regions_device_indexed_wide   k_decode16_region
  indexed_views16  the `indexed16` stream into a 1024 x 1024 view of pitch 1 088 samples, felics_decompress_views_device_indexed_wide   k_decode16_seg_views
and in the lane form (FELICS_TEST_DECODE_LANES=1, FELICS_TEST_DECODE16_LANES=1 or FELICS_TEST_INDEX_LANES=1 around the call) -- to a
change of one form the other form's workloads are the control, code it leaves alone:
  lanes8    4 096 gray8 streams of 64 x 64                                             k_decode8_lanes<false, LaneUniform>
  lanes8_rgb   1 024 RGB8 streams of 64 x 64                                           k_decode8_lanes<true, LaneUniform>
  lanes16   1 024 gray16 streams of 64 x 64                                            k_decode16_lanes<false, LaneUniform>
  lanes16_rgb  512 RGB16 streams of 64 x 64                                            k_decode16_lanes<true, LaneUniform>
  lanes8_pitched  the lanes8 streams into 64 x 64 views of pitch 80                    k_decode8_lanes<false, LanePitched>
  lanes8_mixed    the lanes8 streams through felics_decompress_images_device           k_decode8_lanes<false, LaneMixed>
  indexed_lanes      128 gray8 streams of 256 x 256, indexed at segment 4 096          k_decode8_seg_lanes<false>
  indexed_lanes_rgb  128 RGB8 streams of 256 x 256, indexed at segment 4 096           k_decode8_seg_lanes<true>
Each library is loaded in a child process of its own (FELICS_LIB_PATH); the parent process never opens the GPU and asks the two
children for one call at a time, seat a then seat b, workload after workload, --reps rounds after two warm-up rounds.  A time is
what two device events around the blocking call measure, in milliseconds; medians with min .. max.  Every child compares what its
first call of a workload decoded with the frames and prints a digest of it.

The protocol runs twice.  First with the parent's library in BOTH seats: the relative difference of the two seats' medians is the
workload's margin -- what the protocol itself cannot tell apart.  Then the parent's library against this build: no workload's median
may exceed the parent's by more than its margin (exit status 1 otherwise).

That margin comes from one pair of seats and is smaller than what two invocations differ by on code that did not change
(profiles/lane_fold.txt).  --first FILE names the --out file of an earlier invocation; this one then adds, per workload: the noise =
(max - min) / min over the parent's six medians (both seats of run 1 and seat a of run 2, of both invocations), and SLOWER only if this
build's median exceeds the parent's seat-a median of the same run 2 by more than that noise in BOTH invocations; the exit status is
then this rule's (1: a workload is slower, or pixels differ)."""
import argparse
import hashlib
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
WORKLOADS = ("gray8", "rgb8", "gray16", "rgb16", "pitched8", "mixed8", "mixed16", "indexed", "indexed_rgb", "regions", "indexed_views", "indexed16",
             "indexed16_rgb", "regions16", "indexed_views16", "lanes8", "lanes8_rgb", "lanes16",
             "lanes16_rgb", "lanes8_pitched", "lanes8_mixed", "indexed_lanes", "indexed_lanes_rgb")
SEGMENT = 32768
PITCH = 576
LANE_SEGMENT = 4096
VIEW_PITCH = 2112
VIEW16_PITCH = 1088  # samples
SEGMENT16_RGB = 8192
LANE_PITCH = 80


def child():
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch

    import felics_amd
    from felics_amd import api, build, synth

    enc = felics_amd.Encoder(0)

    def encode(frames, w, h, color, depth, seg=0):
        """frames: a numpy array (n, h, w[, 3]); -> (device frames, device streams, offsets, lens[, device index, index size])"""
        d = torch.from_numpy(np.ascontiguousarray(frames)).cuda()
        n = frames.shape[0]
        # (twice the frame: the worst-case bound of a 16-bit frame is 49 KB per pixel, 320 GB for these sets; a stream that does not fit is
        # the encoder's FELICS_E_BUFFER_TOO_SMALL)
        per = frames[0].nbytes * 2 + 96
        cap = n * ((per + 15) // 16 * 16)
        out = torch.empty(cap, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        if seg:
            isize = api.index_size(w, h, color, depth, seg)
            idx = torch.empty(n * isize, dtype=torch.uint8, device="cuda")
            offs, lens = enc.compress_batch_device_indexed(d.data_ptr(), n, w, h, color, depth, out.data_ptr(), cap, seg, idx.data_ptr(), n * isize)
            return d, out, offs, lens, idx, isize
        offs, lens = enc.compress_batch_device(d.data_ptr(), n, w, h, color, depth, out.data_ptr(), cap)
        return d, out, offs, lens

    def encode16_indexed(frames, w, h, color, seg):
        """a 16-bit set whose version-2 indexes are built on the host from the streams: -> (..., device indexes, their offsets, lengths)"""
        d, out, offs, lens = encode(frames, w, h, color, 1)
        host = out.cpu().numpy()
        blob, ioffs, ilens = bytearray(), [], []
        for o, l in zip(offs, lens):
            ix = api.index16_build(host[int(o):int(o) + int(l)].tobytes(), seg)
            ioffs.append(len(blob))
            ilens.append(len(ix))
            blob += ix + bytes((-len(ix)) % 64)
        return d, out, offs, lens, torch.from_numpy(np.frombuffer(bytes(blob), np.uint8).copy()).cuda(), ioffs, ilens

    g8 = np.stack([synth.gray8(512, 512, f, "S1") for f in range(64)])
    c8 = np.stack([synth.rgb8(512, 512, f) for f in range(64)])
    g16 = np.stack([synth.gray16(512, 512, f) for f in range(64)])
    c16 = np.stack([np.stack([synth.gray16(256, 256, 3 * f + c) for c in range(3)], axis=-1) for f in range(64)])
    big = synth.gray8(2048, 2048, 0, "S1")[None]
    bigc = synth.rgb8(1024, 1024, 0)[None]
    rng = np.random.default_rng(0)
    windows = [(0, int(x), int(y), 256, 256) for x, y in rng.integers(0, 2048 - 256 + 1, size=(64, 2))]
    big16 = synth.gray16(1024, 1024, 0)[None]
    windows16 = [(0, int(x), int(y), 256, 256) for x, y in rng.integers(0, 1024 - 256 + 1, size=(64, 2))]
    small = np.stack([synth.gray8(64, 64, f, "S1") for f in range(4096)])
    sets = {"gray8": encode(g8, 512, 512, 0, 0), "rgb8": encode(c8, 512, 512, 1, 0), "gray16": encode(g16, 512, 512, 0, 1),
            "rgb16": encode(c16, 256, 256, 1, 1), "indexed": encode(big, 2048, 2048, 0, 0, SEGMENT),
            "indexed_rgb": encode(bigc, 1024, 1024, 1, 0, SEGMENT),
            "indexed16": encode16_indexed(big16, 1024, 1024, 0, SEGMENT),
            "indexed16_rgb": encode16_indexed(np.stack([synth.gray16(512, 512, c) for c in range(3)], axis=-1)[None], 512, 512, 1, SEGMENT16_RGB),
            "lanes8": encode(small, 64, 64, 0, 0),
            "lanes8_rgb": encode(np.stack([synth.rgb8(64, 64, f) for f in range(1024)]), 64, 64, 1, 0),
            "lanes16": encode(np.stack([synth.gray16(64, 64, f) for f in range(1024)]), 64, 64, 0, 1),
            "lanes16_rgb": encode(np.stack([np.stack([synth.gray16(64, 64, 3 * f + c) for c in range(3)], axis=-1) for f in range(512)]), 64, 64, 1, 1),
            "indexed_lanes": encode(np.stack([synth.gray8(256, 256, f, "S1") for f in range(128)]), 256, 256, 0, 0, LANE_SEGMENT),
            "indexed_lanes_rgb": encode(np.stack([synth.rgb8(256, 256, f) for f in range(128)]), 256, 256, 1, 0, LANE_SEGMENT)}
    sets["pitched8"] = sets["mixed8"] = sets["gray8"]
    sets["mixed16"] = sets["gray16"]
    sets["lanes8_pitched"] = sets["lanes8_mixed"] = sets["lanes8"]
    sets["regions"] = sets["indexed_views"] = sets["indexed"]
    sets["regions16"] = sets["indexed_views16"] = sets["indexed16"]
    want = {k: v[0].cpu().numpy().view(np.uint8).reshape(-1) for k, v in sets.items()}
    want["regions"] = np.concatenate([big[0, y:y + h, x:x + w].reshape(-1) for _, x, y, w, h in windows])
    want["regions16"] = np.concatenate([big16[0, y:y + h, x:x + w].reshape(-1) for _, x, y, w, h in windows16]).view(np.uint8)
    mosaics = {"pitched8": torch.zeros((64, 512, PITCH), dtype=torch.uint8, device="cuda"),
               "lanes8_pitched": torch.zeros((4096, 64, LANE_PITCH), dtype=torch.uint8, device="cuda"),
               "indexed_views": torch.zeros((1, 2048, VIEW_PITCH), dtype=torch.uint8, device="cuda"),
               "indexed_views16": torch.zeros((1, 1024, VIEW16_PITCH), dtype=torch.int16, device="cuda")}  # (uint16 samples: the bytes are what counts)
    views = {"pitched8": [mosaics["pitched8"][i, :, :512] for i in range(64)],
             "lanes8_pitched": [mosaics["lanes8_pitched"][i, :, :64] for i in range(4096)],
             "indexed_views": [mosaics["indexed_views"][0, :, :2048]], "indexed_views16": [mosaics["indexed_views16"][0, :, :1024]]}
    view16 = [(mosaics["indexed_views16"].data_ptr(), 1024, 1024, 0, 1, 2 * VIEW16_PITCH, 2, 0)]
    dest = {k: torch.zeros(len(v), dtype=torch.uint8, device="cuda") for k, v in want.items() if k not in mosaics}

    def decoded(name):  # the bytes a call of `name` wrote, as the frames lie
        return mosaics[name][:, :, :views[name][0].shape[1]].contiguous().view(torch.uint8).view(-1) if name in mosaics else dest[name]

    def call(name):
        s = sets[name]
        os.environ["FELICS_TEST_DECODE_LANES"] = "1" if name.startswith("lanes8") else "0"  # (read per call)
        os.environ["FELICS_TEST_DECODE16_LANES"] = "1" if name.startswith("lanes16") else "0"
        os.environ["FELICS_TEST_INDEX_LANES"] = "1" if name.startswith("indexed_lanes") else "0"
        if name == "indexed_views":
            enc.decompress_arrays_device_indexed(s[1].data_ptr(), s[2], s[3], s[4].data_ptr(), [0], [s[5]], views[name])
        elif name == "indexed_views16":
            enc.decompress_views_device_indexed16(s[1].data_ptr(), s[2], s[3], s[4].data_ptr(), s[5], s[6], view16)
        elif name == "regions16":
            enc.decompress_regions_device_indexed16(s[1].data_ptr(), s[2], s[3], s[4].data_ptr(), s[5], s[6], windows16, dest[name].data_ptr(),
                                                    dest[name].numel())
        elif name.startswith("indexed16"):
            enc.decompress_batch_device_indexed16(s[1].data_ptr(), s[2], s[3], s[4].data_ptr(), s[5], s[6], dest[name].data_ptr(), dest[name].numel())
        elif name in mosaics:
            enc.decompress_arrays_device(s[1].data_ptr(), s[2], s[3], views[name])
        elif name in ("mixed8", "mixed16", "lanes8_mixed"):
            enc.decompress_images_device(s[1].data_ptr(), s[2], s[3], dest[name].data_ptr(), dest[name].numel())
        elif name == "regions":
            enc.decompress_regions_device_indexed(s[1].data_ptr(), s[2], s[3], s[4].data_ptr(), s[5], windows, dest[name].data_ptr(), dest[name].numel())
        elif name.startswith("indexed"):
            enc.decompress_batch_device_indexed(s[1].data_ptr(), s[2], s[3], s[4].data_ptr(), s[5], dest[name].data_ptr(), dest[name].numel())
        else:
            enc.decompress_batch_device(s[1].data_ptr(), s[2], s[3], dest[name].data_ptr(), dest[name].numel())

    for name in WORKLOADS:  # untimed: allocations, code objects; the pixels checked and their digest printed
        call(name)
        torch.cuda.synchronize()
        got = decoded(name).cpu().numpy()
        print("INFO %s ok=%d sha=%s" % (name, int(np.array_equal(got, want[name])), hashlib.sha256(got.tobytes()).hexdigest()[:16]), flush=True)
    lib_sha = hashlib.sha256(open(build.ensure_lib(), "rb").read()).hexdigest()[:16]
    print("READY %s %s" % (torch.cuda.get_device_name(0).replace(" ", "_"), lib_sha), flush=True)
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for line in sys.stdin:
        cmd = line.split()
        if not cmd or cmd[0] == "quit":
            break
        torch.cuda.synchronize()
        t0.record()
        call(cmd[0])
        t1.record()
        torch.cuda.synchronize()
        print("MS %.5f" % t0.elapsed_time(t1), flush=True)
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
                self.info[f[1]] = dict(kv.split("=") for kv in f[2:])
            elif f and f[0] == "READY":
                self.ready = f[1:]
                break
        if self.ready is None:
            raise RuntimeError("child for %s did not come up (exit %s)" % (lib or "this build", self.p.wait()))

    def ms(self, name):
        self.p.stdin.write(name + "\n")
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


def protocol(lib_a, lib_b, reps):
    """{workload: (times of seat a, times of seat b)}, the two children's READY and INFO lines"""
    a = Child(lib_a)
    try:
        b = Child(lib_b)  # (a child that does not come up must not leave the other one behind)
    except Exception:
        a.close()
        raise
    try:
        ts = {w: ([], []) for w in WORKLOADS}
        for r in range(reps + 2):
            for w in WORKLOADS:
                ta, tb = a.ms(w), b.ms(w)
                if r >= 2:
                    ts[w][0].append(ta)
                    ts[w][1].append(tb)
    finally:
        a.close()
        b.close()
    return ts, (a.ready, b.ready), (a.info, b.info)


def fmt(v):
    return "%10.4f ms (%.4f .. %.4f)" % (statistics.median(v), min(v), max(v))


def medians_of(path):
    """{workload: (run 1 seat a, run 1 seat b, run 2 parent, run 2 this build)} of an --out file's medians"""
    m = {}
    for line in open(path):
        f = line.split()
        if len(f) > 9 and f[0] in WORKLOADS and f[1] == "a":
            m[f[0]] = [float(f[2]), float(f[f.index("b") + 1])]
        elif len(f) > 9 and f[0] in WORKLOADS and f[1] == "parent":
            m[f[0]] += [float(f[2]), float(f[f.index("this") + 1])]
    return m


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--parent-source", default="not given", help="the parent build's source hash (felics_amd.build.source_hash() in its tree)")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--out", default=None)
    ap.add_argument("--first", default=None, help="the --out file of an earlier invocation: judge both by the parent's spread over the two")
    a = ap.parse_args()
    if a.child:
        return child()
    if not a.parent_lib:
        ap.error("--parent-lib is needed")
    sys.path.insert(0, ROOT)
    from felics_amd import build

    lines = []

    def say(s):
        lines.append(s)
        print(s, flush=True)

    ok = pixels = True
    same_ts, ready, info = protocol(a.parent_lib, a.parent_lib, a.reps)
    say("decode_walk_ab.py: device %s; a child process per library, seats alternating call by call, medians of %d after 2 warm-up rounds"
        % (ready[0][0], a.reps))
    say("parent: source %s, library sha256 %s...; this build: source %s" % (a.parent_source, ready[0][1], build.source_hash()))
    say("run 1, the parent's library in both seats (margin = |a - b| / min(a, b) of the medians):")
    margin = {}
    for w in WORKLOADS:
        ma, mb = statistics.median(same_ts[w][0]), statistics.median(same_ts[w][1])
        margin[w] = abs(ma - mb) / min(ma, mb)
        good = info[0][w]["ok"] == "1" and info[1][w]["ok"] == "1"
        ok, pixels = ok and good, pixels and good
        say("  %-17s a %s  b %s  margin %.4f %%  pixels %s" % (w, fmt(same_ts[w][0]), fmt(same_ts[w][1]), 100 * margin[w], "ok" if good else "WRONG"))
    ts, ready, info = protocol(a.parent_lib, None, a.reps)
    say("run 2, seat a = the parent's library, seat b = this build (library sha256 %s...):" % ready[1][1])
    for w in WORKLOADS:
        ma, mb = statistics.median(ts[w][0]), statistics.median(ts[w][1])
        good = info[1][w]["ok"] == "1" and info[0][w]["sha"] == info[1][w]["sha"]
        within = mb <= ma * (1 + margin[w])
        ok, pixels = ok and good and within, pixels and good
        say("  %-17s parent %s  this %s  this / parent - 1 = %+.4f %%  (margin %.4f %%): %s; pixels %s"
            % (w, fmt(ts[w][0]), fmt(ts[w][1]), 100 * (mb / ma - 1), 100 * margin[w], "within" if within else "EXCEEDS", "identical" if good else "DIFFER"))
    say("verdict: %s" % ("every workload within its margin, pixels identical" if ok else "MISSED (see above)"))
    if a.first:
        first = medians_of(a.first)
        say("both invocations (%s and this one): noise = (max - min) / min of the parent's six medians; this / parent - 1 of each run 2:" % a.first)
        slower = []
        for w in WORKLOADS:
            here = [statistics.median(same_ts[w][0]), statistics.median(same_ts[w][1]), statistics.median(ts[w][0]), statistics.median(ts[w][1])]
            par = first[w][:3] + here[:3]
            noise = (max(par) - min(par)) / min(par)
            d1, d2 = first[w][3] / first[w][2] - 1, here[3] / here[2] - 1
            if d1 > noise and d2 > noise:
                slower.append(w)
            say("  %-17s noise %.4f %%  first %+.4f %%  this %+.4f %%: %s" % (w, 100 * noise, 100 * d1, 100 * d2, "SLOWER" if d1 > noise and d2 > noise else "not slower"))
        say("by that rule: %s" % ("slower: " + ", ".join(slower) if slower else "no workload is slower"))
        ok = pixels and not slower  # (the exit status is this rule's then)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
