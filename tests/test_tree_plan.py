"""k_step's tree plan and the structural H^-1 sweep (csrc/allsteps_consts.h), checked on the host.

tests/tree_plan_check.cpp is a stand-alone program (its own main) around plan_tree and sweep_skip_mask.  It
gets the walker's and the quadruped's trees on the command line and adds a 17-link chain (max_path 16,
fk_rounds 4: the deepest accepted), a star and a two-level binary tree; for each it recomputes every plan
word (lpath, lsub, dsub, ancmask, ddesc, jump, root_kids, max_path, max_sub, fk_rounds) from its definition
by walking parent[] and compares it with plan_tree's.  The rejections are checked by their messages
(parent[0] != -1, parent[i] >= i, a negative parent, cfg_dof_link outside [1, num_links), an 18-link chain),
and the structural sweep must contain the compiled skips for the walker and the quadruped and be 0 for a
chain.  Built once plain and once with -fsanitize=address,undefined; both run directly."""

import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "tree_plan_check.cpp")
CXX = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")

pytestmark = pytest.mark.skipif(CXX is None, reason="no host C++ compiler")


def _tree_args():
    from allsteps_isaaclab_amd.model import ANYMAL_C_JSON, load_model

    args = []
    for name, m in (("walker", load_model()), ("quadruped", load_model(ANYMAL_C_JSON))):
        nl = int(m["num_links"])
        args += [name, str(nl), ",".join(str(int(x)) for x in m["parent"][:nl]),
                 ",".join(str(int(x)) for x in m["cfg_dof_link"][:nl - 1])]
    return args


@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]],
                         ids=["plain", "asan_ubsan"])
def test_tree_plan_words(tmp_path, flags):
    exe = tmp_path / "tree_plan_check"
    r = subprocess.run([CXX, "-std=c++17", "-O1", "-Wall", "-Werror", *flags, "-o", str(exe), SRC],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe), *_tree_args()], capture_output=True, text=True, timeout=60)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    assert "tree plan: 5 trees, 0 mismatches" in r.stdout
