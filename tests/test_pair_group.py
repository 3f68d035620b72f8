"""collide()'s grouped capsule bisection (csrc/allsteps_pair_group.h), checked on the host.

tests/pair_group_check.cpp is a stand-alone program (its own main) that emulates a group of 2^L lanes
serially, for L = 2, 3 and 4: every sub-lane's slope sign at its dyadic point, then the walk on the sign
bits, 12 / L rounds.  Against the 12-round one-lane loop over the same sd_box_slope it demands, in bits:
lo and hi after every group round, every t of the one-lane loop among the group's points of that round,
and the final t.  Cases: 1.2 million random segment / box draws (short and long segments, axis-parallel
ones, magnitudes up to the stones' 15 m range) and the adversarial ones -- parallel to a face, along an
edge, zero length, inside the box, minimum at t = 0 and at t = 1, through the centre planes.  Built once
plain and once with -fsanitize=address,undefined; both run directly."""

import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "pair_group_check.cpp")
CXX = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")

pytestmark = pytest.mark.skipif(CXX is None, reason="no host C++ compiler")


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]],
                         ids=["plain", "asan_ubsan"])
def test_pair_group_search(tmp_path, flags):
    exe = tmp_path / "pair_group_check"
    r = subprocess.run([CXX, "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Werror", *flags, "-o", str(exe), SRC],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    assert "1200030 cases, 0 mismatches" in r.stdout
