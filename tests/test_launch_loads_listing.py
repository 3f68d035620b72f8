"""Guard the batching of k_step's and k_obs's per-launch global loads on the CPU box.

Outside the physics every wave of k_step only reads constants and per-env scalars that are known at
launch start; read one by one they were some 44 serialized memory round trips per wave per launch.
They are now issued together (the lane table, the two prologue batches, the parked
epilogue scalars; k_obs's loads ahead of its stores).  A source or compiler change that splits the
batches again would cost launch time without failing any result, so this test compiles
allsteps_kernels.hip with the package's own flags (_native.STEP_FLAGS), counts the vector global loads
and the load-then-wait groups of each kernel (scripts/vm_groups.py) and holds them to
tests/launch_loads_budget.json."""

import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")

BUDGET = {k: v for k, v in json.load(open(os.path.join(ROOT, "tests", "launch_loads_budget.json"))).items()
          if k != "_comment"}


@pytest.fixture(scope="module")
def listing(tmp_path_factory):
    from allsteps_isaaclab_amd import _native

    d = tmp_path_factory.mktemp("vmgroups")
    asm = d / "k.s"
    r = subprocess.run([HIPCC, *_native.STEP_FLAGS, "--cuda-device-only", "-S", "-o", str(asm),
                        os.path.join(_native.CSRC, "allsteps_kernels.hip")],
                       capture_output=True, text=True, timeout=600, cwd=str(d))
    assert r.returncode == 0, r.stderr[-3000:]
    return asm.read_text().split("\n")


@pytest.mark.parametrize("func", sorted(BUDGET))
def test_launch_load_groups(listing, func):
    import vm_groups

    b = BUDGET[func]
    loads, groups, marks = vm_groups.count(listing, func)
    print(f"{func}: {loads} vector global loads in {groups} groups {marks}")
    assert groups <= b["groups_max"], (groups, marks)
    assert loads <= b["loads_max"], loads
    # the cap itself guards the batching: it stays below what the kernel had before it
    assert b["groups_max"] < b["parent_groups"] and b["loads_max"] < b["parent_loads"]
