"""16-bit decoding on one GPU: the lane form (k_decode16_lanes, 64 streams per wave) against the wave form (k_decode16, a wave per
stream), both through felics_decompress_batch_device in the same process, forced with FELICS_TEST_DECODE16_LANES=1 / =0.

    python profiles/tools/decode16_lanes.py [--rounds 3] [--out FILE] [--sizes 64,256] [--counts 256,1024,4096,16384]

Per content (synth.gray16 crops, tiles cut from the golden 16-bit natural images, full-range noise), shape (64 x 64, 256 x 256) and
type (gray16, rgb16): n streams that reference 8 distinct ones n / 8 times each (as bench.py's decode leg does), every frame with a
buffer of its own.  One untimed call per form first (allocations, code objects), then --rounds rounds in alternating order; a time
is the synchronised wall clock of one call, reported as median (min .. max).  Pixels are compared with the sources after every
call.  A combination whose frames (and RGB planes) would take more than a quarter of the device's memory is skipped and named.
The lane form's tables are tagged with epochs and never zeroed per call, so there is no zeroing time to report."""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
VAR = "FELICS_TEST_DECODE16_LANES"
K = 8


def rows_of(npix):  # felics_lanetable.h, dec16l_rows
    need = 2 * min(max(npix - 2, 0), 131071)
    if need > 65536:
        return 131071
    rows = 64
    while rows < need:
        rows *= 2
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--sizes", default="64,256")
    ap.add_argument("--counts", default="256,1024,4096,16384")
    a = ap.parse_args()

    import numpy as np
    import torch
    from PIL import Image

    import felics_amd
    from felics_amd import build, synth
    from tests import oracle_lib

    oracle = oracle_lib.load()
    enc = felics_amd.Encoder(0)
    total_mem = torch.cuda.get_device_properties(0).total_memory
    lines = ["decode16_lanes.py: source %s, device %s, %d rounds per form in alternating order after one untimed call each"
             % (build.source_hash(), torch.cuda.get_device_name(0), a.rounds)]
    golden = os.path.join(ROOT, "tests", "golden")
    naturals = [np.array(Image.open(os.path.join(golden, f))) for f in sorted(os.listdir(golden)) if f.endswith(".tiff")]
    naturals = [im for im in naturals if im.dtype == np.uint16 and im.ndim == 2]
    rng = np.random.default_rng(3)

    def gray(content, s, i):
        if content == "synth":
            return synth.gray16(1024, 768, i)[37 * i % 300:37 * i % 300 + s, 53 * i % 500:53 * i % 500 + s].copy()
        if content == "natural":
            im = naturals[i % len(naturals)]
            y, x = (61 * i) % (im.shape[0] - s + 1), (97 * i) % (im.shape[1] - s + 1)
            return im[y:y + s, x:x + s].copy()
        return rng.integers(0, 65536, size=(s, s), dtype=np.uint16)

    def frame(content, s, rgb, i):
        g = gray(content, s, i)
        if not rgb:
            return g
        if content == "noise":
            return rng.integers(0, 65536, size=(s, s, 3), dtype=np.uint16)
        return np.stack([g, np.roll(g, 1, axis=0), np.roll(g, 1, axis=1)], -1).copy()  # three correlated channels

    ok_all = True
    wins = {}
    for rgb in (False, True):
        for s in [int(v) for v in a.sizes.split(",")]:
            for content in ("synth", "natural", "noise"):
                frames = [frame(content, s, rgb, i) for i in range(K)]
                streams = [oracle.compress(f) for f in frames]
                offs0, blob = [], bytearray()
                for st in streams:
                    offs0.append(len(blob))
                    blob += st + bytes((-len(st)) % 16)
                d_in = torch.from_numpy(np.frombuffer(bytes(blob) + bytes(16), dtype=np.uint8).copy()).cuda()
                ref = torch.from_numpy(np.stack(frames).astype(np.int32)).cuda().to(torch.int32).reshape(K, -1)
                fbytes = frames[0].nbytes
                np_ = 3 if rgb else 1
                tb1 = np_ * rows_of(s * s) * 64
                lines.append("%s %d x %d %s: %d distinct streams of %.0f bytes mean (%.2f bits per sample), lane table %d bytes per stream (wave form: %d)"
                             % ("rgb16" if rgb else "gray16", s, s, content, K, np.mean([len(x) for x in streams]),
                                8 * np.mean([len(x) for x in streams]) / frames[0].size, tb1, 131071 * 64))
                for n in [int(v) for v in a.counts.split(",")]:
                    need = n * fbytes + (n * s * s * 3 * 4 if rgb else 0)
                    if need > total_mem // 4:
                        lines.append("  n = %5d: skipped (frames%s of %.1f GB are more than a quarter of the device's memory)"
                                     % (n, " and planes" if rgb else "", need / 1e9))
                        continue
                    offs = np.array([offs0[i % K] for i in range(n)], dtype=np.uint64)
                    lens = np.array([len(streams[i % K]) for i in range(n)], dtype=np.uint64)
                    d_px = torch.zeros(n * fbytes, dtype=torch.uint8, device="cuda")
                    times = {"0": [], "1": []}
                    good = {"0": True, "1": True}
                    info = {}

                    def run(form, keep):
                        os.environ[VAR] = form
                        try:
                            d_px.zero_()
                            torch.cuda.synchronize()
                            t0 = time.perf_counter()
                            _, status = enc.decompress_batch_device(d_in.data_ptr(), offs, lens, d_px.data_ptr(), d_px.numel())
                            torch.cuda.synchronize()
                            dt = (time.perf_counter() - t0) * 1e3
                        finally:
                            os.environ.pop(VAR, None)
                        got = d_px.view(torch.int16).to(torch.int32).bitwise_and(0xFFFF).reshape(n // K, K, -1)
                        good[form] &= bool((status == 0).all()) and bool((got == ref[None]).all().item())
                        if keep:
                            times[form].append(dt)
                        if form == "1":
                            info["tb"] = enc.decode_stats()["lanes16_table_bytes"]

                    run("0", False)
                    run("1", False)
                    for r in range(a.rounds):
                        for form in (("0", "1") if r % 2 == 0 else ("1", "0")):
                            run(form, True)
                    del d_px
                    torch.cuda.empty_cache()
                    mpix = n * s * s / 1e6
                    med = {f: statistics.median(times[f]) for f in times}
                    per = max(1, info["tb"] // tb1)
                    ok_all &= good["0"] and good["1"]
                    wins.setdefault((rgb, s, n), []).append(med["1"] < med["0"])
                    lines.append("  n = %5d (%7.1f MPix): wave %8.2f ms (%.2f .. %.2f) %6.3f GPix/s | lanes %8.2f ms (%.2f .. %.2f) %6.3f GPix/s | lanes / wave %.2fx | "
                                 "lane tables %.1f MB in %d pass%s | pixels exact: wave %s, lanes %s"
                                 % (n, mpix, med["0"], min(times["0"]), max(times["0"]), mpix / med["0"], med["1"], min(times["1"]), max(times["1"]),
                                    mpix / med["1"], med["0"] / med["1"], info["tb"] / 1e6, -(-n // per), "" if n <= per else "es", good["0"], good["1"]))
                    sys.stdout.write(lines[-1] + "\n")
                    sys.stdout.flush()
    lines.append("lane form faster than the wave form on all three contents (median against median, same run):")
    for (rgb, s, n), w in sorted(wins.items()):
        lines.append("  %s %3d x %3d n = %5d: %s" % ("rgb16 " if rgb else "gray16", s, s, n, "yes" if all(w) and len(w) == 3 else "no (%d of %d)" % (sum(w), len(w))))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
    enc.close()
    return 0 if ok_all else 1


if __name__ == "__main__":
    sys.exit(main())
