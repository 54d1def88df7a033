"""Where a front workgroup's time goes, step by step (s_memtime stamps of wave 0, summed per tile; k_front, the FSTAMP indices as
felics_kernels.hip has them).  The wait in front of trip d ends once the trip's nine registers have arrived: the cycles between the
loads' issue and their first use that nothing hid.

Needs a library built with the stamps compiled in (they are not in the product build):
    profiles/tools/variant.sh fstamps -DFELICS_FRONT_STAMPS      # in the build container (add -DFELICS_FORMS=127 for the parent's order)
    python3 profiles/tools/front_stamps.py 64 [variant] [kind]   # on the GPU box, from the repository root
"""
import os, sys, ctypes, time
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
os.environ.setdefault("FELICS_LIB_PATH", os.path.join(ROOT, "felics_amd", "_variants", sys.argv[2] if len(sys.argv) > 2 else "fstamps", "libfelics.so"))
import numpy as np, torch
import felics_amd
from felics_amd import synth_torch
n = int(sys.argv[1]) if len(sys.argv) > 1 else 64
kind = sys.argv[3] if len(sys.argv) > 3 else "S1"
W, H = 3840, 2160
frames = torch.stack([synth_torch.gray8(W, H, f, kind) for f in range(n)])
d_out = torch.empty(int(n * W * H * 1.25) + (1 << 20), dtype=torch.uint8, device="cuda")
torch.cuda.synchronize()
enc = felics_amd.Encoder(0)
lib = ctypes.CDLL(os.environ["FELICS_LIB_PATH"])
buf = (ctypes.c_ulonglong * (256 * 16))()
for _ in range(3):
    enc.compress_batch_device(frames.data_ptr(), n, W, H, 0, 0, d_out.data_ptr(), d_out.numel())
lib.felics_debug_front_stamps(buf, 1)
t = time.time()
R = 5
for _ in range(R):
    enc.compress_batch_device(frames.data_ptr(), n, W, H, 0, 0, d_out.data_ptr(), d_out.numel())
dt = (time.time() - t) / R
lib.felics_debug_front_stamps(buf, 0)
v = list(np.array(list(buf), dtype=np.float64).reshape(256, 16).sum(0))
cnt = v[15]
rows = [(11, "addresses, the first trips issued"), (4, "the last trip in flight issued"), (0, "WAIT in front of trip 0"), (5, "trip 0 classified and ranked (+ next issue)"),
        (1, "WAIT in front of trip 1"), (6, "trip 1 classified and ranked (+ next issue)"), (2, "WAIT in front of trip 2"), (7, "trip 2 classified and ranked"),
        (3, "WAIT in front of trip 3"), (8, "trip 3 classified and ranked"), (9, "barrier behind the trips"), (12, "step 3: the tile's layout, run table (two barriers)"),
        (13, "step 4: place into the sorted order (+ barrier)"), (14, "step 5: out, order check")]
tot = sum(v[:15])
print("%s, %s: blocking call %.3f ms; %d tiles stamped; s_memtime ticks per tile (wave 0):" % (os.path.basename(os.path.dirname(os.environ["FELICS_LIB_PATH"])), kind, dt * 1e3, cnt))
for i, nm in rows:
    print("  %2d %-60s %9.0f  %5.1f %%" % (i, nm, v[i] / cnt, 100.0 * v[i] / tot))
print("  waits in front of the trips together %.0f; total %.0f ticks per tile" % (sum(v[:4]) / cnt, tot / cnt))
enc.close()
