"""The noise models' shared formulas (csrc/allsteps_noise.h) on the host.

tests/noise_check.cpp is a stand-alone program (its own main) around the header.  It must reproduce every
output of tests/golden/noise.npz -- the reference's own isaaclab/utils/noise/noise_model.py run on recorded
draws (tests/golden/gen_noise.py) -- bit for bit: every kind x operation, Python-float and per-column
parameters (resolved by the env's host code, envs/noise.py), bias models with a reset of all envs and of a
subset.  Its Philox block for the four noise tags equals the oracle's or_philox_block, and its Box-Muller is
within 1e-5 of a float64 one (r <= sqrt(48 ln 2) ~ 5.8; the f32 angle 2 pi u carries up to 2.4e-7; cos, sin
and log a few ulp: ~3.5e-6 worst case, x3 for another libm).  Built once plain and once with
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
SRC = os.path.join(ROOT, "tests", "noise_check.cpp")
CXX = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
REFERENCE = "/root/reference"

sys.path.insert(0, os.path.join(ROOT, "tests"))


def _philox_queries(orc):
    """Queries over the four noise tags and the oracle's answers: (6 uint32, 4 float32) each."""
    from allsteps_isaaclab_amd import _native

    fn = orc.L.or_philox_block
    fn.argtypes = [C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.POINTER(C.c_float)]
    fn.restype = None
    rng = np.random.default_rng(5)
    out = []
    for tag in _native.NOISE_TAGS:
        for q in range(16):
            seed = int(rng.integers(0, 1 << 63)) if q else 42
            env, t, b = (int(rng.integers(0, 1 << 32)) if q > 1 else q for _ in range(3))
            buf = (C.c_float * 4)()
            fn(seed, env, t, b, tag, buf)
            out.append(((seed & 0xFFFFFFFF, seed >> 32, env, t, b, tag), tuple(buf)))
    return out


def _write_cases(path, orc):
    from _noise_cases import N, load_cases

    cases = load_cases("cpu")
    with open(path, "wb") as f:
        queries = _philox_queries(orc)
        f.write(struct.pack("i", len(queries)))
        for words, floats in queries:
            f.write(struct.pack("6I4f", *words, *floats))
        f.write(struct.pack("i", len(cases)))
        for c in cases:
            d = c["state"].desc
            f.write(struct.pack("7i2f", N, c["cols"], d.kind, d.op, d.bias_kind, d.bias_op, len(c["steps"]),
                                d.bias_p0, d.bias_p1))
            for a in (c["state"].p0.numpy(), c["state"].p1.numpy(), c["x"], c["draws"]):
                f.write(np.ascontiguousarray(a, np.float32).tobytes())
            for mask, bdraw, bias, out in c["steps"]:
                f.write(np.ascontiguousarray(mask, np.int32).tobytes())
                for a in (bdraw, bias, out):
                    f.write(np.ascontiguousarray(a, np.float32).tobytes())
    return len(cases)


@pytest.mark.skipif(CXX is None, reason="no host C++ compiler")
@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]],
                         ids=["plain", "asan_ubsan"])
def test_noise_header_reproduces_the_reference(tmp_path, orc, flags):
    exe, cases = tmp_path / "noise_check", tmp_path / "cases.bin"
    ncases = _write_cases(cases, orc)
    assert ncases == 32
    r = subprocess.run([CXX, "-std=c++17", "-O1", "-Wall", "-Werror", *flags, "-o", str(exe), SRC],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe), str(cases)], capture_output=True, text=True, timeout=60)
    print(r.stdout[-3000:], r.stderr[-2000:])
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert "philox: 64 queries, 0 mismatches" in r.stdout
    assert f"noise fixture: {ncases} cases" in r.stdout and ", 0 mismatches" in r.stdout.split("noise fixture:")[1]
    assert "groups and bias draw: 0 mismatches" in r.stdout


@pytest.mark.skipif(not os.path.isdir(REFERENCE), reason="no reference checkout here")
def test_fixture_regenerates_byte_for_byte():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "golden", "gen_noise.py"), "--check",
                        "--reference", REFERENCE], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert "identical" in r.stdout
