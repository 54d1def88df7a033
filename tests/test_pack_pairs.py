"""The pair builder of k_pack_t's 8-bit instantiations (felics_amd/csrc/felics_pairs.h: the classification and the phased-in code of two
pixels per instruction), checked on the host by pairs_check: the program compiles the header the kernels compile and compares it, for
every (pixel, left, above) in 256^3, in either half of a pair and beside two different partners, with the scalar formulas -- val, above
and in_range for every triple, code_in and len_in wherever the pixel is in range, a half never depending on the other -- and then the
byte selection of a 16-sample group: the left neighbour across a dword boundary and the sample in front of the group.  Once as an
ordinary build, once under AddressSanitizer and UBSan (a stand-alone host binary)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "felics_amd", "csrc")


@pytest.mark.parametrize("target", ["../_build/pairs_check", "../_build/asan/pairs_check"])
def test_pair_builder_on_the_host(target):
    subprocess.check_call(["make", "-C", CSRC, target], stdout=subprocess.DEVNULL)
    r = subprocess.run([os.path.normpath(os.path.join(CSRC, target))], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:]
    m = re.fullmatch(r"pairs_check: (\d+) triples in both halves with two partners each, (\d+) groups: ok", r.stdout.strip().splitlines()[-1])
    assert m, r.stdout[-4000:]
    assert int(m.group(1)) == 256 ** 3 and int(m.group(2)) > 200000
