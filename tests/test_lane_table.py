"""k_step's per-lane constants table (csrc/allsteps_lane_table.h), checked on the host.

tests/lane_table_check.cpp is a stand-alone program (its own main) around the header's builder: it fills
as_model_t / as_task_t / the actuator with a pattern that gives every source entry its own value, at the
walker's shape (22 links, 21 hinges, 22 geoms, 27 dofs) and the quadruped's (13 links, 18 dofs), and
compares every field of all 32 rows with the entry the kernel read from the model tables before -- the
clamped lanes and the mirror / sign selection (a later match wins) included.  Built once plain and once
with -fsanitize=address,undefined; both run directly."""

import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "lane_table_check.cpp")
CXX = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")

pytestmark = pytest.mark.skipif(CXX is None, reason="no host C++ compiler")


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]],
                         ids=["plain", "asan_ubsan"])
def test_lane_table_rows(tmp_path, flags):
    exe = tmp_path / "lane_table_check"
    r = subprocess.run([CXX, "-std=c++17", "-O1", "-Wall", "-Werror", *flags, "-o", str(exe), SRC],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    assert "lane table: 0 mismatches" in r.stdout
