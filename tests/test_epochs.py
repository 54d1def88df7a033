"""The epoch rules of a long-lived context (felics_amd/csrc/felics_epochs.h: the look-back status words of k_pack_t, the estimator
tables of k_decode16 and of k_decode16_lanes, each kept valid between calls by a tag instead of a clear), checked on the host by
epoch_check: the program compiles the very functions run_lane and the decoders' hosts do and walks each over its whole period and
its wrap beside a model of the tagged buffer -- no tag handed out twice between two clears, tag 0 only behind a clear, a fresh
buffer's first epochs 1, 1 .. 3 and 1 .. 3 -- and it must report the reuse behind 0x03FFFFFF in the look-back rule as it stood before
the counter was left to run over.  Once as an ordinary build (2^32 sub-batches), once under AddressSanitizer (2^27 steps on either
side of each 32-bit wrap)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "felics_amd", "csrc")


@pytest.mark.parametrize("target", ["../_build/epoch_check", "../_build/asan/epoch_check"])
def test_epoch_rules_on_the_host(target):
    subprocess.check_call(["make", "-C", CSRC, target], stdout=subprocess.DEVNULL)
    r = subprocess.run([os.path.normpath(os.path.join(CSRC, target))], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:]
    lines = r.stdout.splitlines()
    assert lines[-1] == "all checks held", r.stdout[-4000:]
    assert "fresh buffers: first epochs 1, 1 .. 3, 1 .. 3" in lines
    # the walk notices what it is there for: the rule before the fix reuses epoch 1 without a clear
    assert any(re.fullmatch(r"look-back, the rule before the fix \(expected to fail\): step 67108863 epoch 0x1 masked 0x1 reused, "
                            r"first used at epoch 0x3fc0001, no clear between", line) for line in lines), r.stdout[-4000:]
    m = re.search(r"^look-back: (\d+) sub-batches walked, (\d+) clears", r.stdout, re.M)
    assert m and int(m.group(1)) >= (1 << 28) and int(m.group(2)) > 0
    if "asan" not in target:
        assert int(m.group(1)) > (1 << 32)  # the counter's whole period and the wrap behind it
    assert re.search(r"^lane form: first clear on launch 10923, one every 10922 launches", r.stdout, re.M)
    assert re.search(r"^wave form: \d+ passes walked, 1 clear", r.stdout, re.M)
