"""The action manager's shared code (csrc/allsteps_actions.h) on the host.

tests/actions_check.cpp is a stand-alone program (its own main) around the header.  On tests/golden/actions.npz -- the
reference's own ActionManager.process_action / apply_action / reset(env_ids) with its four joint term classes on
recorded inputs (tests/golden/gen_actions.py) -- and the column tables the env's host code makes of the same cfgs
(envs/actions.py), the header reproduces bit for bit every array of every step of every case: action, prev_action,
the terms' raw_actions (the columns of action), processed_actions, the targets handed to the articulation (the
command buffer) and the EMA terms' prev_applied, after the step and after the reset that follows it.  No tolerance:
the operations are +, x, min and max in float32.  One thing is not a value and is not compared: which NaN a NaN is.
torch.clamp with tensor bounds returns the input's NaN from its scalar loop and an all-ones NaN (0xffffffff) from its
vector loop, so the reference's own payload depends on where in the tensor the element lies; a word that is a NaN on
both sides counts as equal, every other word is compared by its bits (signed zeros and infinities included).  The
header against its NumPy restatement is compared by bits throughout: the restatement of tests/_actions_cases.py, which
the GPU tests compare the kernels with at other sizes, equals the header in every word.

Built once plain and once with -fsanitize=address,undefined; both run directly."""

import os
import shutil
import struct
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "actions_check.cpp")
CXX = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
REFERENCE = os.environ.get("ALLSTEPS_REFERENCE", "")
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]

sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def reset_mask(case: dict, s: int) -> np.ndarray:
    m = np.zeros(case["n"], np.uint8)
    m[case["resets"].get(s, [])] = 1
    return m


def write_cases(path, cases) -> None:
    with open(path, "wb") as f:
        f.write(struct.pack("i", len(cases)))
        for c in cases:
            rows = np.ascontiguousarray(c["spec"].rows, np.float32)
            f.write(struct.pack("4i", c["n"], rows.shape[0], c["joints"], c["steps"]))
            f.write(rows.tobytes())
            for s in range(c["steps"]):
                f.write(np.ascontiguousarray(c["raw"][s], np.float32).tobytes())
                f.write(np.ascontiguousarray(c["joint_pos"][s].T, np.float32).tobytes())
                f.write(struct.pack("i", c.get("reset_mode", {}).get(s, 1 if s in c["resets"] else 0)))
                f.write(reset_mask(c, s).tobytes())


def read_dump(path, cases) -> list:
    raw = np.fromfile(path, np.float32)
    out, at = [], 0
    for c in cases:
        n, D, J = c["n"], c["spec"].total, c["joints"]
        steps = []
        for _ in range(c["steps"]):
            d = {}
            for key, cols in (("action", D), ("prev_action", D), ("processed", D), ("prev_applied", D), ("cmd", J),
                              ("post_action", D), ("post_prev_action", D), ("post_prev_applied", D)):
                d[key] = raw[at:at + n * cols].reshape(n, cols)
                at += n * cols
            steps.append(d)
        out.append(steps)
    assert at == raw.size
    return out


def build_check(tmp_path, flags=()):
    exe = tmp_path / "actions_check"
    r = subprocess.run([CXX, "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror", *flags, "-o", str(exe), SRC],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


@pytest.fixture(scope="module")
def cases():
    from _actions_cases import load_cases

    return load_cases()


def test_fixture_is_small_and_has_the_cases(cases):
    from _actions_cases import FIXTURE, KIND_EFFORT, KIND_EMA, KIND_POSITION, KIND_TO_LIMITS

    assert os.path.getsize(FIXTURE) <= 400 << 10
    assert [c["name"] for c in cases] == ["a", "b", "c", "d", "e", "f"]
    assert [c["joints"] for c in cases] == [12, 12, 12, 12, 21, 12]
    kinds = [sorted({t.kind for t in c["spec"].terms}) for c in cases]
    assert kinds == [[KIND_POSITION], [KIND_POSITION], [KIND_TO_LIMITS, KIND_EMA], [KIND_EMA], [KIND_EFFORT], [KIND_EMA]]
    a, b, c, d, e, f = cases
    for case in (a, b, e, f):
        assert case["resets"] == {1: [1, 4, 7, 12], 3: [1, 4, 7, 12]}
    assert c["resets"] == {} and d["resets"] == {}  # (the reference cannot reset an EMA term over a joint subset)
    assert len(c["spec"].terms) == 2 and len(d["spec"].terms) == 3 and len(e["spec"].terms) == 2
    assert b["meta"]["terms"][0]["fields"]["preserve_order"] is True
    assert b["spec"].column_joints != sorted(b["spec"].column_joints)  # the order of the expressions, not the joints'
    al = f["spec"].rows[:, 10]
    assert (al == 0).any() and (al == 1).any() and ((al > 0) & (al < 1)).any()
    assert {float(t.rows.view(np.float32)[0, 10]) for t in d["spec"].terms[:2]} == {0.0, 1.0}
    for case in cases:
        x = case["raw"]
        assert np.isnan(x).any() and np.isposinf(x).any() and np.isneginf(x).any()
        zero = x[x == 0]
        assert np.signbit(zero).any() and not np.signbit(zero).all()
        assert (np.abs(x[np.isfinite(x)]) > 1e30).any() and (np.abs(x[np.isfinite(x)]) > 1).any()
        # the reference's resolution: same term dimensions and joint order as this project's
        assert case["meta"]["dims"] == case["spec"].dims and case["meta"]["total"] == case["spec"].total
        names = case["spec"].ctx.joint_names
        assert case["meta"]["term_joints"] == [[names[j] for j in t.joint_ids] for t in case["spec"].terms]


@pytest.mark.skipif(CXX is None, reason="no host C++ compiler")
@pytest.mark.parametrize("flags", [[], SAN], ids=["plain", "asan_ubsan"])
def test_actions_header_reproduces_the_reference(tmp_path, cases, flags):
    from _actions_cases import host_process, host_reset, same_bits, same_bits_or_nan, zero_state

    # the fixture's cases, and case f once more with every env reset through a null mask
    run = list(cases) + [dict(cases[-1], name="f_all", reset_mode={1: 2, 3: 2})]
    write_cases(tmp_path / "cases.bin", run)
    exe = build_check(tmp_path, flags)
    r = subprocess.run([str(exe), str(tmp_path / "cases.bin"), str(tmp_path / "dump.bin")], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    print(r.stdout.strip())
    dump = read_dump(tmp_path / "dump.bin", run)
    for c, steps in zip(run, dump):
        spec, ref = c["spec"], c["ref"]
        st = zero_state(c["n"], spec.total, c["joints"])
        for s, d in enumerate(steps):
            where = (c["name"], s)
            # the NumPy restatement equals the header in every word
            host_process(spec.rows, c["raw"][s], st)
            for k in ("action", "prev_action", "processed", "prev_applied", "cmd"):
                assert same_bits(d[k], st[k]), (where, k)
            mode = c.get("reset_mode", {}).get(s, 1 if s in c["resets"] else 0)
            if mode:
                host_reset(spec.rows, st, c["joint_pos"][s].T, None if mode == 2 else reset_mask(c, s))
            for k in ("action", "prev_action", "prev_applied"):
                assert same_bits(d["post_" + k], st[k]), (where, "post_" + k)
            if c["name"] == "f_all":
                if mode:
                    assert not d["post_action"].any() and not d["post_prev_action"].any()
                    assert same_bits(d["post_prev_applied"], c["joint_pos"][s][:, spec.column_joints])
                continue
            # the header equals the reference bit for bit (a NaN for a NaN: see the module docstring)
            for k in ("action", "prev_action", "processed", "prev_applied"):
                assert same_bits_or_nan(d[k], ref[k][s]), (where, k)
            assert same_bits_or_nan(d["action"], ref["raw"][s]), where  # raw_actions: the columns of action
            assert same_bits_or_nan(d["cmd"], ref["targets"][s]), where
            for k in ("action", "prev_action", "prev_applied"):
                assert same_bits_or_nan(d["post_" + k], ref["post_" + k][s]), (where, "post_" + k)
            assert same_bits_or_nan(d["post_action"], ref["post_raw"][s]), where


@pytest.mark.skipif(not os.path.isdir(REFERENCE), reason="ALLSTEPS_REFERENCE does not name a reference checkout")
def test_fixture_regenerates_bit_for_bit():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "golden", "gen_actions.py"), "--reference",
                        REFERENCE, "--check"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
