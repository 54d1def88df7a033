"""The pure pieces of k_front's back half (felics_amd/csrc/felics_frontout.h: the output words of four consecutive slots, the padding
fix pix = 0xFFFF, the order predicate, the slot bases of step 3), checked on the host by frontout_check: the program compiles the
header the kernels compile and compares it with the scalar definitions -- every (context, value, offset, above) class in every position
beside every kind of partner, every ordered pair of key classes with padding on either side, and whole tiles whose runs of 0 .. 33
events lie at every distance from a pass boundary and from the end of the LDS image, sorted and with two neighbours exchanged.  Once as
an ordinary build, once under AddressSanitizer and UBSan (a stand-alone host binary)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "felics_amd", "csrc")


@pytest.mark.parametrize("target", ["../_build/frontout_check", "../_build/asan/frontout_check"])
def test_front_out_pieces_on_the_host(target):
    subprocess.check_call(["make", "-C", CSRC, target], stdout=subprocess.DEVNULL)
    r = subprocess.run([os.path.normpath(os.path.join(CSRC, target))], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:]
    m = re.fullmatch(r"frontout_check: (\d+) entry classes beside their partners, (\d+) ordered pairs, (\d+) tiles at the pass boundaries and the "
                     r"window's end \(and (\d+) larger\), (\d+) exchanges caught: ok", r.stdout.strip().splitlines()[-1])
    assert m, r.stdout[-4000:]
    classes, pairs, tiles, larger, exchanges = (int(g) for g in m.groups())
    assert classes == 512 * 512 * 11 * 2 * 5 and pairs > 200000 and tiles > 3000 and larger > 0 and exchanges > 100000
