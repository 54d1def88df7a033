"""The per-lane code of the lane decoders (felics_amd/csrc/felics_lanewalk.h: bit reader, pixel step, estimators, the walk over a plane
and the walk over a segment from its checkpoint), checked on the host by lanewalk_check: the program compiles the very functions
k_decode8_lanes, k_decode8_seg_lanes and k_decode16_lanes do and decodes the oracle's streams through them, one stream per call, into
buffers of exactly the size a walk may touch -- whole planes, pitched views whose gaps must keep their pattern, segments that must
stay inside their pixels, cut and flipped streams, and a 16-bit table whose rows another stream left in the same epoch (which must
be noticed: what the epoch rules of felics_epochs.h are there to prevent) -- also at the end of a whole cycle of 10 922 launches in
other epochs on a table that is never cleared, the schedule tests/test_gpu_epochs.py runs on the GPU.  Once as an ordinary build, once under AddressSanitizer, the same shapes."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "felics_amd", "csrc")


@pytest.mark.parametrize("target", ["../_build/lanewalk_check", "../_build/asan/lanewalk_check"])
def test_lane_walks_on_the_host(target):
    subprocess.check_call(["make", "-C", CSRC, target], stdout=subprocess.DEVNULL)
    r = subprocess.run([os.path.normpath(os.path.join(CSRC, target))], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:]
    lines = r.stdout.splitlines()
    assert lines[-1] == "all checks held", r.stdout[-4000:]
    # the rare paths were walked: contexts beyond the hot ones (their rows in the table) and Rice codes longer than the reader's window
    # (the long codes in the 8-bit step and in the 16-bit step, which have limits of their own)
    m = re.search(r"^whole planes: noise cold-context pixels (\d+) long-code pixels 8-bit (\d+) 16-bit (\d+)$", r.stdout, re.M)
    assert m and all(int(g) > 0 for g in m.groups()), r.stdout[-4000:]
    for case in ("whole planes:", "pitched:", "from a checkpoint:", "damage:", "stale table:", "whole cycle:"):
        assert any(line.startswith(case) for line in lines), case
