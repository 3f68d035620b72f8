"""The contact timers' shared code (csrc/allsteps_contact_timers.h) on the host.

tests/contact_timers_check.cpp is a stand-alone program (its own main) around the header.  It must reproduce every
array of tests/golden/contact_timers.npz -- the reference's own SensorBase.update, ContactSensor._update_buffers_impl
and ContactSensor.reset run on recorded forces (tests/golden/gen_contact_timers.py) -- bit for bit: the four timers
and the timestamp after every recorded update.  It is fed the fixture's IMPULSES, not the forces: the header's
whole path runs, the division by dt included (the generator keeps impulses whose float32 quotient by dt is the force
the reference saw).  Built once plain and once with -fsanitize=address,undefined; both run directly.  The float32
numpy restatement the GPU tests compare with (_contact_timers_cases.host_update) must give the same bits."""

import os
import shutil
import struct
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "contact_timers_check.cpp")
CXX = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")

sys.path.insert(0, os.path.join(ROOT, "tests"))


def _write_cases(path):
    from _contact_timers_cases import load_cases

    cases = load_cases()
    f32 = lambda a: np.ascontiguousarray(a, np.float32).tobytes()  # noqa: E731
    with open(path, "wb") as f:
        f.write(struct.pack("i", len(cases)))
        for c in cases:
            f.write(struct.pack("4i2f", c["n"], c["bodies"], c["updates"], c["stride"], c["dt"], c["threshold"]))
            f.write(f32(c["impulses"]) + np.ascontiguousarray(c["resets"], np.int32).tobytes())
            f.write(f32(c["timers"]) + f32(c["timestamp"]))
    return cases


def test_fixture_has_the_cases_the_issue_names():
    from _contact_timers_cases import load_cases

    cases = {c["name"]: c for c in load_cases()}
    assert set(cases) == {"a", "b", "c0", "c1"}
    a, b = cases["a"], cases["b"]
    assert (a["n"], a["bodies"], a["updates"], a["stride"], a["threshold"]) == (70, 2, 240, 1, 1.0)
    assert a["dt"] == 1 / 240 and a["resets"].any() and not a["resets"].reshape(60, 4, 70)[:, :3].any()
    assert a["timers"].shape == (240, 4, 2, 70) and a["timestamp"].shape == (240, 70)
    assert (b["updates"], b["stride"]) == (3600, 4) and not b["resets"].any()
    # the drift: the timestamp's steps over an env step are not one value
    assert len(np.unique(np.diff(b["timestamp"][:, 0]))) > 1
    assert cases["c0"]["threshold"] == 1.0 and cases["c1"]["threshold"] == 2.0


@pytest.mark.skipif(CXX is None, reason="no host C++ compiler")
@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]],
                         ids=["plain", "asan_ubsan"])
def test_timers_header_reproduces_the_reference(tmp_path, flags):
    exe, path = tmp_path / "contact_timers_check", tmp_path / "cases.bin"
    cases = _write_cases(path)
    r = subprocess.run([CXX, "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror", *flags, "-o", str(exe),
                        SRC], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe), str(path)], capture_output=True, text=True, timeout=120)
    print(r.stdout[-3000:], r.stderr[-2000:])
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert f"contact timers fixture: {len(cases)} cases" in r.stdout
    assert ", 0 mismatches" in r.stdout.split("contact timers fixture:")[1]
    assert "layout and elapsed time: 0 mismatches" in r.stdout


def test_numpy_restatement_reproduces_the_reference():
    """host_update / host_reset on the fixture's impulses give the fixture's bits at every record."""
    from _contact_timers_cases import host_reset, host_update, load_cases

    for c in load_cases():
        timers = np.zeros((4, c["bodies"], c["n"]), np.float32)
        ts = np.zeros(c["n"], np.float32)
        for u in range(c["updates"]):
            host_update(timers, ts, np.ascontiguousarray(c["impulses"][u]), c["dt"], c["threshold"])
            host_reset(timers, ts, c["resets"][u])
            if (u + 1) % c["stride"] == 0:
                rec = (u + 1) // c["stride"] - 1
                assert np.array_equal(timers.view(np.uint32), c["timers"][rec].view(np.uint32)), (c["name"], u)
                assert np.array_equal(ts.view(np.uint32), c["timestamp"][rec].view(np.uint32)), (c["name"], u)
