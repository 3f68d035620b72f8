"""The reward manager's shared code (csrc/allsteps_rewards.h) on the host.

tests/rewards_check.cpp is a stand-alone program (its own main) around the header.  On tests/golden/rewards.npz -- the
reference's own RewardManager.compute / reset with its term functions on recorded inputs (tests/golden/gen_rewards.py)
-- and the device tables the env's host code makes of the same cfgs (envs/rewards.py):

  cases a, a0, c, c1 (inputs on a 2^-8 grid, every reduction exact): every word of every term but the exp terms is
      the reference's bit for bit -- the term values, the episodic sums, step_reward, last_episode_sums, and the
      totals of a0 and c1, which have no exp term; zero-weight terms are skipped;
  the exp terms: the argument is torch's bit for bit and the result within 3 ulp of torch's (as_expf's documented
      2 ulp, include/as_detmath.h, plus 1 ulp for torch's vectorised exp);
  case b (full-precision inputs): per term kind the header's max abs error against the float64 values is at most
      twice the reference float32's own (a different association of <= 21 rounded addends can at most double the
      error), exact where that is 0; the threshold terms agree exactly.

The NumPy restatement of tests/_rewards_cases.py (with the oracle's exp) equals the header bit for bit.  Built once
plain and once with -fsanitize=address,undefined; both run directly.

  track_lin_vel_xy_yaw_frame_exp, whose argument passes the library's atan2 / sincos: argument and value against
      float64 under _rewards_cases.yaw_frame_bounds, which the reference's own float32 value meets as well.

Measured (case a / c exp terms): at most 1 ulp from torch; the yaw-frame term uses at most 0.10 of its bound.  Case b
ratios header / reference of the max abs error against float64: between 0.53 and 1.00 per kind."""

import os
import shutil
import struct
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "rewards_check.cpp")
CXX = os.environ.get("CXX") or shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
REFERENCE = os.environ.get("ALLSTEPS_REFERENCE", "")

sys.path.insert(0, os.path.join(ROOT, "tests"))


def write_cases(path, cases) -> None:
    from _rewards_cases import SOURCES

    with open(path, "wb") as f:
        f.write(struct.pack("i", len(cases)))
        for c in cases:
            x = c["inputs"]
            f.write(struct.pack("10i2f", c["n"], len(c["names"]), c["steps"], x["actions"].shape[2], x["q"].shape[1],
                                x["net"].shape[1], x["net"].shape[2], x["timers"].shape[2], x["commands"].shape[1],
                                0, c["dt"], c["sim_dt"]))
            for s in range(c["steps"]):
                spec = c["specs"][s]
                f.write(np.ascontiguousarray(spec.rows, np.float32).tobytes())
                f.write(np.ascontiguousarray(spec.table, np.float32).tobytes())
                for k in SOURCES:
                    f.write(np.ascontiguousarray(x[k][s]).tobytes())
                f.write(np.ascontiguousarray(c["reset"][s], np.uint8).tobytes())


def read_dump(path, cases) -> list:
    raw = np.fromfile(path, np.float32)
    out, at = [], 0
    for c in cases:
        n, T, A = c["n"], len(c["names"]), c["inputs"]["actions"].shape[2]
        steps = []
        for _ in range(c["steps"]):
            d = {}
            for key, shape in (("f", (T, n)), ("reward", (n,)), ("sums", (T, n)), ("step", (T, n)), ("last", (T, n)),
                               ("prev", (n, A))):
                size = int(np.prod(shape))
                d[key] = raw[at:at + size].reshape(shape)
                at += size
            steps.append(d)
        out.append(steps)
    assert at == raw.size
    return out


def build_check(tmp_path, flags=()):
    exe = tmp_path / "rewards_check"
    r = subprocess.run([CXX, "-std=c++17", "-O1", "-ffp-contract=off", "-Wall", "-Werror", *flags, "-o", str(exe), SRC],
                       capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return exe


def same_bits(a, b) -> bool:
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    nan = np.isnan(b)
    return bool(np.array_equal(a.view(np.uint32)[~nan], b.view(np.uint32)[~nan]) and np.isnan(a[nan]).all())


@pytest.fixture(scope="module")
def cases():
    from _rewards_cases import load_cases

    return load_cases()


def test_fixture_is_within_the_committed_file_size_limit_and_has_the_cases(cases):
    from _rewards_cases import FIXTURE

    assert os.path.getsize(FIXTURE) <= 1 << 20
    assert [c["name"] for c in cases] == ["a", "a0", "b", "c", "c1"]
    a, a0, b, c, c1 = cases
    assert len(a["names"]) == 21 and len(a0["names"]) == 17 and len(c1["names"]) == 1 and a["n"] == 66
    assert a["steps"] == 12 and b["steps"] == 6
    assert a["reset"][3, 5] and a["reset"][4, 5]  # one env reset in two steps running
    k = a["names"].index("ang_vel_xy")
    assert [float(s.terms[k].weight) == 0.0 for s in a["specs"]] == [False] * 4 + [True] * 4 + [False] * 4
    qd = c["inputs"]["qd"]
    assert np.isnan(qd).any() and np.isposinf(qd).any() and np.isneginf(qd).any()
    assert not c["inputs"]["net"][:, :, :, :, 3].any()  # an all-zero history
    cc = c["inputs"]["timers"][:, 2]
    assert ((cc[:, :, 4] > 0).sum(1) == 1).all() and ((cc[:, :, 5] > 0).sum(1) == 2).all()
    ids = {t["name"]: t["params"].get("joint_ids") for t in c["terms"]}
    assert ids["jvel_l1"] == [3] and ids["jvel_l2"] is None


@pytest.mark.skipif(CXX is None, reason="no host C++ compiler")
@pytest.mark.parametrize("flags", [[], ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"]],
                         ids=["plain", "asan_ubsan"])
def test_rewards_header_reproduces_the_reference(tmp_path, orc, cases, flags):
    from _rewards_cases import (EXP_FUNCS, REDUCTIONS, YAW_FUNC, host_step, oracle_exp, step_inputs, term_values,
                                ulp_diff, yaw_frame_bounds, yaw_frame_f64, zero_state)

    write_cases(tmp_path / "cases.bin", cases)
    exe = build_check(tmp_path, flags)
    r = subprocess.run([str(exe), str(tmp_path / "cases.bin"), str(tmp_path / "dump.bin")], capture_output=True,
                       text=True, timeout=120)
    print(r.stdout[-3000:], r.stderr[-3000:])
    assert r.returncode == 0, (r.stdout[-3000:], r.stderr[-3000:])
    assert "rewards fixture: 5 cases" in r.stdout and " 0 skipped" not in r.stdout and " 0 done" not in r.stdout
    dump = read_dump(tmp_path / "dump.bin", cases)
    exp = oracle_exp(orc)
    worst_exp_ulp, worst_yaw = 0, 0.0
    for c, steps in zip(cases, dump):
        T, n, A = len(c["names"]), c["n"], c["inputs"]["actions"].shape[2]
        state = zero_state(T, n, A)
        err_h, err_r = {}, {}
        for s, got in enumerate(steps):
            spec = c["specs"][s]
            # the NumPy restatement equals the header, every word
            total, state, fv = host_step(spec, step_inputs(c, s), state, c["reset"][s], c["dt"], c["sim_dt"], exp)
            where = (c["name"], s)
            assert same_bits(fv, got["f"]), where
            assert same_bits(total, got["reward"]), where
            for key, name in (("sums", "episode_sums"), ("step", "step_reward"), ("last", "last_episode_sums"),
                              ("prev", "prev_actions")):
                assert same_bits(state[name], got[key]), (where, key)
            done = c["reset"][s].astype(bool)
            assert same_bits(got["prev"], np.where(done[:, None], np.float32(0), c["inputs"]["actions"][s]))
            for k, t in enumerate(c["terms"]):
                where = (c["name"], s, t["name"])
                if t["func"] == YAW_FUNC:
                    # the library's atan2 / sincos: argument and value against float64 under the derived bounds,
                    # which the reference's own float32 value must meet as well
                    x = step_inputs(c, s)
                    std, row = t["params"]["std"], spec.terms[k].cmd_row
                    arg64, val64 = yaw_frame_f64(x, row, std)
                    assert np.allclose(val64, c["f64"][s, k], rtol=1e-12, atol=0), where
                    darg, dval = yaw_frame_bounds(x, row, std)
                    args = {}
                    term_values(spec, x, state["prev_actions"], c["sim_dt"], exp, exp_args=args)
                    ea = np.abs(args[k].astype(np.float64) - arg64) / darg
                    ev = np.abs(got["f"][k].astype(np.float64) - val64) / dval
                    er = np.abs(c["f"][s, k].astype(np.float64) - val64) / dval
                    worst_yaw = max(worst_yaw, float(ea.max()), float(ev.max()))
                    assert ea.max() <= 1 and ev.max() <= 1 and er.max() <= 1, (where, ea.max(), ev.max(), er.max())
                    continue
                if t["func"] in EXP_FUNCS:
                    d = ulp_diff(got["f"][k], c["f"][s, k])
                    worst_exp_ulp = max(worst_exp_ulp, int(d.max()))
                    assert d.max() <= 3, (where, int(d.max()))
                    continue
                if c["name"] == "b":
                    kind = t["func"]
                    f64 = c["f64"][s, k]
                    err_h[kind] = max(err_h.get(kind, 0.0), float(np.abs(got["f"][k].astype(np.float64) - f64).max()))
                    err_r[kind] = max(err_r.get(kind, 0.0), float(np.abs(c["f"][s, k].astype(np.float64) - f64).max()))
                    if kind not in REDUCTIONS:
                        assert same_bits(got["f"][k], c["f"][s, k]), where
                    continue
                # grid cases: the reference's bits in every word of the term
                assert same_bits(got["f"][k], c["f"][s, k]), where
                assert same_bits(got["sums"][k], c["sums"][s, k]), where
                assert same_bits(got["step"][k], c["step"][s, k]), where
                assert same_bits(got["last"][k], c["last"][s, k]), where
            if c["name"] in ("a0", "c1"):  # no exp term: the total is the reference's
                assert same_bits(got["reward"], c["reward"][s]), where
            if c["name"] == "a" and 4 <= s < 8:  # the zero-weight term's rows stay as step 3 left them
                k = c["names"].index("ang_vel_xy")
                assert same_bits(got["step"][k], steps[3]["step"][k])
        for kind in err_h:
            print(f"case b {kind}: header {err_h[kind]:.3e} reference {err_r[kind]:.3e} "
                  f"ratio {err_h[kind] / err_r[kind] if err_r[kind] else 0.0:.2f}")
            assert err_h[kind] <= 2.0 * err_r[kind], (kind, err_h[kind], err_r[kind])
    print("exp terms: worst distance from torch", worst_exp_ulp, "ulp; yaw-frame term: worst fraction of its bound",
          round(worst_yaw, 3))


def test_exp_arguments_are_torchs_bit_for_bit(orc, cases):
    """The exp terms' arguments, restated by _rewards_cases.term_values as the header forms them, against the same
    expression in torch on the recorded rows; torch's exp of that argument is the fixture's value."""
    import torch

    from _rewards_cases import EXP_FUNCS, oracle_exp, step_inputs, term_values
    from allsteps_isaaclab_amd.envs.views import _RobotData

    exp = oracle_exp(orc)
    checked = 0
    for c in cases:
        if c["name"] == "b":
            continue
        for s in range(c["steps"]):
            x = step_inputs(c, s)
            args = {}
            term_values(c["specs"][s], x, np.zeros_like(x["actions"]), c["sim_dt"], exp, exp_args=args)
            t = lambda a: torch.from_numpy(np.ascontiguousarray(a.T))  # noqa: E731
            q, cmd = t(x["root_quat"]), t(x["commands"])
            lin_b = _RobotData._rotate_inverse(q, t(x["root_lin"]))
            ang_b = _RobotData._rotate_inverse(q, t(x["root_ang"]))
            for k, term in enumerate(c["terms"]):
                if term["func"] not in EXP_FUNCS:
                    continue
                std = term["params"]["std"]
                if term["func"] == "track_lin_vel_xy_exp":
                    want = -torch.sum(torch.square(cmd[:, :2] - lin_b[:, :2]), dim=1) / std**2
                elif term["func"] == "track_ang_vel_z_exp":
                    want = -torch.square(cmd[:, 2] - ang_b[:, 2]) / std**2
                else:
                    want = -torch.square(cmd[:, 2] - t(x["root_ang"])[:, 2]) / std**2
                assert same_bits(args[k], want.numpy()), (c["name"], s, term["name"])
                assert same_bits(torch.exp(want).numpy(), c["f"][s, k]), (c["name"], s, term["name"])
                checked += 1
    assert checked >= 3 * 12


@pytest.mark.skipif(not os.path.isdir(REFERENCE), reason="no reference checkout given (ALLSTEPS_REFERENCE)")
def test_fixture_regenerates_bit_for_bit():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "golden", "gen_rewards.py"), "--check",
                        "--reference", REFERENCE], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert "identical" in r.stdout
