"""Where a pack workgroup's time goes, phase by phase (s_memtime stamps of thread 0, summed per tile; k_pack_t, the PSTAMP indices
as felics_kernels.hip has them).  "Wait" phases end once the register the wait is for has arrived: the cycles between a load's issue
and its first use that nothing hid.

Needs a library built with the stamps compiled in (they are not in the product build):
    profiles/tools/variant.sh pstamps -DFELICS_PACK_STAMPS       # in the build container (add -DFELICS_FORMS=127 for the parent's order)
    python3 profiles/tools/pack_stamps.py 64 [variant] [kind]    # on the GPU box, from the repository root
"""
import os, sys, ctypes
ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
os.environ.setdefault("FELICS_LIB_PATH", os.path.join(ROOT, "felics_amd", "_variants", sys.argv[2] if len(sys.argv) > 2 else "pstamps", "libfelics.so"))
import numpy as np, torch
import felics_amd
from felics_amd import synth_torch, api
n = int(sys.argv[1]) if len(sys.argv) > 1 else 64
W, H = 3840, 2160
kind = sys.argv[3] if len(sys.argv) > 3 else "S1"
frames = torch.stack([synth_torch.gray8(W, H, f, kind) for f in range(n)])
d_out = torch.empty(int(n * W * H * 1.25) + (1 << 20), dtype=torch.uint8, device="cuda")
torch.cuda.synchronize()
enc = felics_amd.Encoder(0)
lib = ctypes.CDLL(os.environ["FELICS_LIB_PATH"])
buf = (ctypes.c_ulonglong * (256 * 16))()
import time
for _ in range(3):
    enc.compress_batch_device(frames.data_ptr(), n, W, H, 0, 0, d_out.data_ptr(), d_out.numel())
lib.felics_debug_pack_stamps(buf, 1)
t = time.time()
R = 5
for _ in range(R):
    enc.compress_batch_device(frames.data_ptr(), n, W, H, 0, 0, d_out.data_ptr(), d_out.numel())
dt = (time.time() - t) / R
lib.felics_debug_pack_stamps(buf, 0)
a = np.array(list(buf), dtype=np.float64).reshape(256, 16); v = list(a.sum(0))
cnt = v[15]
names = ["ticket (tile and plane of the workgroup)", "window out (shift, stores)", "gather: codes / k of the loaded slots into LDS",
         "wait for the other waves (barrier behind the gather)", "code phase: geometry of the group", "code phase: sixteen codes + scan",
         "sync (the waves' bit counts)", "look-back + sync", "codes into the window", "pixel loads issued, window (and words) cleared",
         "WAIT for the slot loads (kq, pix, ev)", "WAIT for tile_slots[pt] (early form: pixel and slot loads issued first)"]
print("%s, %s: blocking call %.3f ms; %d tiles stamped; s_memtime ticks per tile (thread 0):" % (os.path.basename(os.path.dirname(os.environ["FELICS_LIB_PATH"])), kind, dt * 1e3, cnt))
tot = sum(v[:12])
for i, nm in enumerate(names):
    if nm != "-":
        print("  %2d %-72s %9.0f  %5.1f %%" % (i, nm, v[i] / cnt, 100.0 * v[i] / tot))
print("  total %.0f ticks per tile" % (tot / cnt))
enc.close()
