"""The index rule of the 16-bit lane decoder's hashed estimator table (felics_amd/csrc/felics_lanetable.h), checked on the host by
lanetable_check: the program compiles the very functions the kernel does -- rows per pixel count, home row, probe step, search --
and inserts, for every table size from the smallest to the dense one, as many contexts as the rule admits in sets chosen to collide."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "felics_amd", "csrc")
EXE = os.path.join(ROOT, "felics_amd", "_build", "lanetable_check")


def test_lanetable_index_rule():
    subprocess.check_call(["make", "-C", CSRC, "../_build/lanetable_check"], stdout=subprocess.DEVNULL)
    r = subprocess.run([EXE], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:]
    assert "all checks held" in r.stdout
    # twelve sizes: 64 rows doubling to 65 536, then the dense table
    sizes = [int(line.split()[-2]) for line in r.stdout.splitlines() if line.startswith("from ")]
    assert sizes == [64 << i for i in range(11)] + [131071], sizes
    for kind in ("congruent", "consecutive", "top", "x4096"):
        assert sum(1 for line in r.stdout.splitlines() if line.startswith("rows ") and kind in line) == 12, kind
