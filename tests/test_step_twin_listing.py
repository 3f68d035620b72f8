"""k_step and its diagnostic twin k_step_diag on the compiled listing.

The phase stamps of as_debug_stamps (csrc/step_lanes.h, Stamp<kOn>) are compiled into k_step_diag alone:
launch_step picks the twin exactly when a stamp buffer is set, and the production kernel carries no stamp
pointer, counter, branch, clock read or LDS accumulator.  This test compiles allsteps_kernels.hip once with the
package's own flags (_native.STEP_FLAGS) and checks, for the four instantiations (walker and quadruped, with
and without the sweep skips):

  * every k_step<...> and every k_step_diag<...> symbol is in the listing;
  * no production kernel reads a clock (s_memtime / s_memrealtime);
  * every twin does.
"""

import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")

# <NV, SKIP> as mangled: the walker and the quadruped, each with its sweep-skip mask and with the full sweep
# (the same instantiations tests/kernel_budget.json names)
INSTANCES = ("ILi27ELm207817167EEEvNS_8StepArgsE", "ILi27ELm0EEEvNS_8StepArgsE",
             "ILi18ELm3219EEEvNS_8StepArgsE", "ILi18ELm0EEEvNS_8StepArgsE")
PRODUCTION = tuple("_ZN2as6k_step" + i for i in INSTANCES)
TWINS = tuple("_ZN2as11k_step_diag" + i for i in INSTANCES)
CLOCK = re.compile(r"^\s*s_mem(real)?time\b")


@pytest.fixture(scope="module")
def bodies(tmp_path_factory):
    """{symbol: the instruction lines of its body} for every function of the listing."""
    from allsteps_isaaclab_amd import _native

    d = tmp_path_factory.mktemp("steptwin")
    asm = d / "k.s"
    r = subprocess.run([HIPCC, *_native.STEP_FLAGS, "--cuda-device-only", "-S", "-o", str(asm),
                        os.path.join(_native.CSRC, "allsteps_kernels.hip")],
                       capture_output=True, text=True, timeout=600, cwd=str(d))
    assert r.returncode == 0, r.stderr[-3000:]
    out, cur = {}, None
    for line in asm.read_text().split("\n"):
        m = re.match(r"^(_Z\w+):", line)
        if m:
            cur = out.setdefault(m.group(1), [])
        elif line.startswith(".Lfunc_end"):
            cur = None
        elif cur is not None:
            cur.append(line)
    return out


@pytest.mark.parametrize("func", PRODUCTION + TWINS)
def test_symbol_exists(bodies, func):
    assert func in bodies and len(bodies[func]) > 1000, sorted(k for k in bodies if "k_step" in k)


@pytest.mark.parametrize("func", PRODUCTION)
def test_production_kernel_reads_no_clock(bodies, func):
    hits = [l.strip() for l in bodies[func] if CLOCK.match(l)]
    print(f"{func}: {len(hits)} clock reads")
    assert not hits, hits[:5]


@pytest.mark.parametrize("func", TWINS)
def test_twin_reads_the_clock(bodies, func):
    hits = [l.strip() for l in bodies[func] if CLOCK.match(l)]
    print(f"{func}: {len(hits)} clock reads")
    assert hits
