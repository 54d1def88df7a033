#!/usr/bin/env python3
"""Code-object figures of every kernel in a built libfelics.so: VGPRs, SGPRs, LDS bytes, scratch bytes, spills.

    python profiles/tools/kernel_meta.py LIB                 one line per kernel symbol
    python profiles/tools/kernel_meta.py PARENT_LIB LIB      both builds side by side, per kernel symbol, and the kernels that differ

Needs no GPU: the figures are the AMDGPU metadata note of the gfx950 code objects bundled in the library (the kernel descriptors'
values as the compiler recorded them).  What DESIGN 3h's invariant is checked with: a change that adds a geometry policy must leave
the existing instantiations' figures as they were.
"""
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("ROCM_LLVM", "/opt/rocm/llvm/bin")
FIELDS = [("vgpr_count", "vgpr"), ("sgpr_count", "sgpr"), ("group_segment_fixed_size", "lds"), ("private_segment_fixed_size", "scratch"),
          ("vgpr_spill_count", "vspill"), ("sgpr_spill_count", "sspill")]
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def code_objects(lib):
    """The gfx950 code objects of every bundle in the library's .hip_fatbin section."""
    blob = open(lib, "rb").read()
    out = []
    at = blob.find(MAGIC)
    while at >= 0:
        n = int.from_bytes(blob[at + 24:at + 32], "little")
        p = at + 32
        for _ in range(n):
            off, size, tlen = (int.from_bytes(blob[p + 8 * i:p + 8 * i + 8], "little") for i in range(3))
            triple = blob[p + 24:p + 24 + tlen].decode()
            p += 24 + tlen
            if "gfx950" in triple and size:
                out.append(blob[at + off:at + off + size])
        at = blob.find(MAGIC, at + 1)
    return out


def kernels(lib):
    res = {}
    for co in code_objects(lib):
        with tempfile.NamedTemporaryFile(suffix=".co") as f:
            f.write(co)
            f.flush()
            notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", f.name], capture_output=True, text=True, check=True).stdout
        for block in re.split(r"\n\s*- \.agpr_count:", notes)[1:]:
            name = re.search(r"\.name:\s+(\S+)", block)
            if not name:
                continue
            vals = []
            for key, _ in FIELDS:
                m = re.search(r"\.%s:\s+(\d+)" % key, block)
                vals.append(int(m.group(1)) if m else -1)
            res[name.group(1)] = tuple(vals)
    return res


def demangle(names):
    import shutil

    tool = next((t for t in (os.path.join(LLVM, "llvm-cxxfilt"), shutil.which("c++filt")) if t and os.path.exists(t)), None)
    if not tool:
        return {n: n for n in names}
    out = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    return dict(zip(names, out))


def main(argv):
    if len(argv) == 2:
        k = kernels(argv[1])
        dm = demangle(sorted(k))
        print("# %s" % " ".join(short for _, short in FIELDS))
        for n in sorted(k):
            print("%s  %s" % (" ".join("%d" % v for v in k[n]), dm[n]))
        return 0
    a, b = kernels(argv[1]), kernels(argv[2])
    dm = demangle(sorted(set(a) | set(b)))
    differ = 0
    print("# per kernel symbol: %s  (parent | this build)" % " ".join(short for _, short in FIELDS))
    for n in sorted(set(a) | set(b)):
        fa = " ".join("%d" % v for v in a[n]) if n in a else "-"
        fb = " ".join("%d" % v for v in b[n]) if n in b else "-"
        mark = "new" if n not in a else "gone" if n not in b else "same" if a[n] == b[n] else "DIFFERS"
        differ += mark in ("gone", "DIFFERS")
        print("%-7s %-24s | %-24s %s" % (mark, fa, fb, dm[n]))
    print("# %d kernels in the parent, %d in this build, %d of the parent's differ or are gone" % (len(a), len(b), differ))
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
