"""The command manager's shared code (csrc/allsteps_commands.h) on the host.

tests/commands_check.cpp is a stand-alone program (its own main) around the header.  It must reproduce
tests/golden/commands.npz -- the reference's own CommandManager.reset / compute with UniformVelocityCommand and
NormalVelocityCommand terms run on recorded draws (tests/golden/gen_commands.py) -- from descriptors resolved by the
env's host code (envs/commands.py): bit for bit everything that is not downstream of atan2 (timers, counters, masks,
heading targets, sampled commands, the zeroing, error_vel_xy, the snapshot rows, who resamples in which phase, the
normal term entirely), and within the measured heading tolerance the yaw command of the heading envs and
error_vel_yaw.  Its Philox block for the two command tags equals the oracle's or_philox_block.  Built once plain
and once with -fsanitize=address,undefined; both run directly."""

import ctypes as C
import os
import re
import shutil
import struct
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "commands_check.cpp")
CXX = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")

sys.path.insert(0, os.path.join(ROOT, "tests"))


def _philox_queries(orc):
    """Queries over the two command tags and the oracle's answers: (6 uint32, 4 float32) each."""
    from allsteps_isaaclab_amd import _native

    fn = orc.L.or_philox_block
    fn.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_float)]
    fn.restype = None
    rng = np.random.default_rng(7)
    out = []
    for tag in _native.COMMAND_TAGS:
        for q in range(16):
            seed = int(rng.integers(0, 1 << 63)) if q else 42
            env, t, b = (int(rng.integers(0, 1 << 32)) if q > 1 else q for _ in range(3))
            buf = (C.c_float * 4)()
            fn(seed, env, t, b, tag, buf)
            out.append(((seed & 0xFFFFFFFF, seed >> 32, env, t, b, tag), tuple(buf)))
    return out


def write_cases(path, orc, cases=None) -> int:
    """cases.bin of commands_check.cpp from the fixture's cases (or the given ones)."""
    from _commands_cases import N, load_cases

    cases = load_cases() if cases is None else cases
    f32 = lambda a: np.ascontiguousarray(a, np.float32).tobytes()  # noqa: E731
    i32 = lambda a: np.ascontiguousarray(a, np.int32).tobytes()  # noqa: E731

    def state(c, s=None):
        g = (lambda k: c[k + "0"]) if s is None else (lambda k: c[k][s])
        return (f32(g("vel")) + f32(g("heading_target")) + i32(g("flags")) + f32(g("time_left")) + i32(g("counter"))
                + f32(g("metrics")))

    with open(path, "wb") as f:
        queries = _philox_queries(orc)
        f.write(struct.pack("i", len(queries)))
        for words, floats in queries:
            f.write(struct.pack("6I4f", *words, *floats))
        f.write(struct.pack("i", len(cases)))
        for c in cases:
            f.write(struct.pack("4if", N, c["rows"].shape[0], c["steps"], int(c["name"] != "c"), c["dt"]))
            f.write(f32(c["rows"]) + state(c) + f32(c["init_draws"]))
            for s in range(c["steps"]):
                f.write(f32(c["root_quat"][s]) + f32(c["root_lin"][s]) + f32(c["root_ang"][s]) + i32(c["reset"][s]))
                f.write(f32(c["draws"][s]) + state(c, s) + f32(c["last_metrics"][s]) + i32(c["resampled"][s]))
    return len(cases)


def build_check(tmp_path, flags=()):
    exe = tmp_path / "commands_check"
    r = subprocess.run([CXX, "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror", *flags, "-o", str(exe), SRC],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def read_dump(path, cases):
    """The header's state after every step of every case, as commands_check.cpp dumps it: per case a dict of
    (steps, ...) arrays in the kernel's layouts (flags and counter int32)."""
    from _commands_cases import N

    raw = np.fromfile(path, np.uint32)
    out, o = [], 0
    for c in cases:
        K = c["rows"].shape[0]
        shapes = (("vel", (K, 3, N), np.float32), ("heading_target", (K, N), np.float32), ("flags", (K, 5, N), np.int32),
                  ("time_left", (K, N), np.float32), ("counter", (K, N), np.int32), ("metrics", (K, 2, N), np.float32),
                  ("last_metrics", (K, 2, N), np.float32))
        d = {k: [] for k, _, _ in shapes}
        for _ in range(c["steps"]):
            for k, shape, dtype in shapes:
                size = int(np.prod(shape))
                d[k].append(raw[o:o + size].view(dtype).reshape(shape))
                o += size
        out.append({k: np.stack(v) for k, v in d.items()})
    assert o == raw.size
    return out


def _measures(stdout):
    m = re.search(r"max \|diff\| (\S+) rad/s, per unit stiffness (\S+) rad; error_vel_yaw max \|diff\| (\S+);", stdout)
    assert m, stdout
    return tuple(float(x) for x in m.groups())


@pytest.mark.skipif(CXX is None, reason="no host C++ compiler")
@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]],
                         ids=["plain", "asan_ubsan"])
def test_commands_header_reproduces_the_reference(tmp_path, orc, flags):
    from _commands_cases import HEADING_BOUND, MEASURED_ERR_YAW_DIFF, MEASURED_HEADING_DIFF

    cases = tmp_path / "cases.bin"
    ncases = write_cases(cases, orc)
    assert ncases == 4
    exe = build_check(tmp_path, flags)
    for args, carried in (([], False), ([str(tmp_path / "dump.bin")], True)):
        r = subprocess.run([str(exe), str(cases), *args], capture_output=True, text=True, timeout=120)
        print(r.stdout[-3000:], r.stderr[-2000:])
        assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
        assert "philox: 32 queries, 0 mismatches" in r.stdout
        tail = r.stdout.split("commands fixture:")[1]
        assert f" {ncases} cases" in tail and ", 0 mismatches" in tail
        assert " 0 double resamples" not in tail
        assert "stream layout, wrap and sample: 0 mismatches" in r.stdout
        yaw, per_stiffness, err_yaw = _measures(r.stdout)
        print(f"measured: yaw {yaw:.9g} rad/s, per unit stiffness {per_stiffness:.9g} rad, error_vel_yaw {err_yaw:.9g}")
        # the measured value may not exceed |stiffness| 8 2^-22 rad/s: anything larger is a bug, not rounding
        assert per_stiffness <= HEADING_BOUND
        assert per_stiffness <= MEASURED_HEADING_DIFF  # the value the tolerance of the GPU tests is made from
        if carried:  # the header's own yaw commands carried from step to step: error_vel_yaw sums their differences
            assert err_yaw <= MEASURED_ERR_YAW_DIFF
        else:  # the reference's yaw command taken over after every step: error_vel_yaw reads that one
            assert err_yaw == 0.0


def test_numpy_restatement_reproduces_the_header(tmp_path, orc):
    """The float32 numpy restatement the GPU tests compare the Philox path and the envs with
    (_commands_cases.host_step, atan2 from the oracle's as_atan2f) gives the host header's bits -- atan2 included --
    from the fixture's inputs and draws."""
    if CXX is None:
        pytest.skip("no host C++ compiler")
    from _commands_cases import STATE, host_step, load_cases, oracle_atan2

    cases = load_cases()
    write_cases(tmp_path / "cases.bin", orc, cases)
    exe = build_check(tmp_path)
    r = subprocess.run([str(exe), str(tmp_path / "cases.bin"), str(tmp_path / "dump.bin")], capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-3000:]
    atan2 = oracle_atan2(orc)
    for c, want in zip(cases, read_dump(tmp_path / "dump.bin", cases)):
        st = {k: c[k + "0"].copy() for k in STATE}
        st["last_metrics"] = np.zeros_like(st["metrics"])
        for s in range(c["steps"]):
            st, resampled = host_step(c["rows"], c["dt"], st, atan2, (c["root_quat"][s], c["root_lin"][s],
                                                                      c["root_ang"][s]), c["reset"][s], c["draws"][s])
            assert np.array_equal(resampled, c["resampled"][s].astype(bool)), (c["name"], s)
            for k in (*STATE, "last_metrics"):
                got = np.ascontiguousarray(st[k]).astype(want[k].dtype)
                assert np.array_equal(got.view(np.uint32), want[k][s].view(np.uint32)), (c["name"], s, k)
