"""The interval events' shared code (csrc/allsteps_events.h) on the host.

tests/events_check.cpp is a stand-alone program (its own main) around the header.  It must reproduce every array
of tests/golden/events.npz -- the reference's own EventManager.apply(mode="interval") and
push_by_setting_velocity run on recorded draws (tests/golden/gen_events.py) -- bit for bit: timers, fired masks
and velocities of every step, and the initial timers, from descriptors resolved by the env's host code
(envs/events.py: the interval width formed in double, the velocity width in float32).  Its Philox block for the
two event tags equals the oracle's or_philox_block.  Built once plain and once with
-fsanitize=address,undefined; both run directly."""

import ctypes as C
import os
import shutil
import struct
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "events_check.cpp")
CXX = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")

sys.path.insert(0, os.path.join(ROOT, "tests"))


def _philox_queries(orc):
    """Queries over the two event tags and the oracle's answers: (6 uint32, 4 float32) each."""
    from allsteps_isaaclab_amd import _native

    fn = orc.L.or_philox_block
    fn.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_float)]
    fn.restype = None
    rng = np.random.default_rng(6)
    out = []
    for tag in _native.EVENT_TAGS:
        for q in range(16):
            seed = int(rng.integers(0, 1 << 63)) if q else 42
            env, t, b = (int(rng.integers(0, 1 << 32)) if q > 1 else q for _ in range(3))
            buf = (C.c_float * 4)()
            fn(seed, env, t, b, tag, buf)
            out.append(((seed & 0xFFFFFFFF, seed >> 32, env, t, b, tag), tuple(buf)))
    return out


def _write_cases(path, orc):
    from _events_cases import N, load_cases

    cases = load_cases()
    f32 = lambda a: np.ascontiguousarray(a, np.float32).tobytes()  # noqa: E731
    with open(path, "wb") as f:
        queries = _philox_queries(orc)
        f.write(struct.pack("i", len(queries)))
        for words, floats in queries:
            f.write(struct.pack("6I4f", *words, *floats))
        f.write(struct.pack("i", len(cases)))
        for c in cases:
            f.write(struct.pack("4if", N, c["rows"].shape[0], c["steps"], int("init_draws" in c), c["dt"]))
            f.write(f32(c["rows"]) + f32(c["vel0"]) + f32(c["time_left0"]))
            if "init_draws" in c:
                f.write(f32(c["init_draws"]))
            for s in range(c["steps"]):
                f.write(f32(c["iv_draws"][s]) + f32(c["push_draws"][s]) + f32(c["time_left"][s]))
                f.write(np.ascontiguousarray(c["fired"][s], np.int32).tobytes())
                f.write(f32(c["vel"][s]))
    return len(cases)


@pytest.mark.skipif(CXX is None, reason="no host C++ compiler")
@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]],
                         ids=["plain", "asan_ubsan"])
def test_events_header_reproduces_the_reference(tmp_path, orc, flags):
    exe, cases = tmp_path / "events_check", tmp_path / "cases.bin"
    ncases = _write_cases(cases, orc)
    assert ncases == 3
    r = subprocess.run([CXX, "-std=c++17", "-O1", "-Wall", "-Werror", *flags, "-o", str(exe), SRC],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe), str(cases)], capture_output=True, text=True, timeout=60)
    print(r.stdout[-3000:], r.stderr[-2000:])
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert "philox: 32 queries, 0 mismatches" in r.stdout
    assert f"events fixture: {ncases} cases" in r.stdout and ", 0 mismatches" in r.stdout.split("events fixture:")[1]
    assert "stream layout and fire test: 0 mismatches" in r.stdout


def test_numpy_restatement_reproduces_the_reference():
    """The float32 numpy restatement the GPU tests compare the Philox path with (_events_cases.host_step) gives
    the fixture's bits from the fixture's draws."""
    from _events_cases import host_step, load_cases

    for c in load_cases():
        tl, vel = c["time_left0"], c["vel0"]
        for s in range(c["steps"]):
            tl, vel, fired = host_step(c["rows"], c["dt"], tl, vel, c["iv_draws"][s], c["push_draws"][s])
            for got, want in ((tl, c["time_left"][s]), (vel, c["vel"][s])):
                assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (c["name"], s)
            assert np.array_equal(fired, c["fired"][s]), (c["name"], s)
