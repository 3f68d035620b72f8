"""The IMU's shared code (csrc/allsteps_imu.h) on the host.

tests/imu_check.cpp is a stand-alone program (its own main) around the header.  Built once plain and once with
-fsanitize=address,undefined; both run directly.  Its outputs must be

  * within 2 x E_ref of the reference's own float64 outputs, per output field and per case of tests/golden/imu.npz
    (gen_imu.py: the reference's Imu, SensorBase and math code over a fake body view), E_ref being the reference's
    own float32-against-float64 difference on the same inputs.  2 x is the project's margin for arithmetic without
    transcendentals (test_ray_caster_host.py); the slack exists because torch.bmm fixes neither the dot product's
    association nor its use of FMA.  Measured: at most 1.09 x (case c, lin_acc_b), 1.00 x or less elsewhere;
  * the stated exact answers on the hand cases (_imu_cases.hand_cases: identity and 180 degree quaternions, the
    (4, 4, 8) then (0, 0, 8) acceleration, the per-env outdated rule);
  * equal, bit for bit, to the NumPy float32 restatement of _imu_cases on every case -- the restatement the GPU tests
    hold the kernel to."""

import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _imu_cases as ic  # noqa: E402

REFERENCE = os.environ.get("ALLSTEPS_REFERENCE", "")
needs_cxx = pytest.mark.skipif(ic.CXX is None, reason="no host C++ compiler")


@pytest.fixture(scope="module")
def program_outputs(tmp_path_factory):
    """The plain build's outputs on every case: (cases, outputs per case, stdout)."""
    tmp = tmp_path_factory.mktemp("imu_plain")
    exe = str(tmp / "imu_check")
    ic.build_program(exe)
    cases = ic.all_cases()
    stdout, outs = ic.run_program(exe, str(tmp), cases)
    return cases, outs, stdout


@pytest.fixture(scope="module")
def restated():
    return [ic.replay(c) for c in ic.all_cases()]


def _same_as_restatement(cases, outs, restated):
    for c, o, (d, p) in zip(cases, outs, restated):
        assert np.array_equal(o["data"].view(np.uint32), d.view(np.uint32)), c["name"]
        assert np.array_equal(o["prev"].view(np.uint32), p.view(np.uint32)), c["name"]


def test_fixture_has_the_cases_the_issue_names():
    cases = {c["name"]: c for c in ic.load_cases()}
    assert set(cases) == {"a", "b", "c"}
    a, b, c = cases["a"], cases["b"], cases["c"]
    for k in cases.values():
        assert k["dt"] == 1 / 240 and set(k["e_ref"]) == {f for f, _, _ in ic.FIELDS}
        assert k["data64"].dtype == np.float64 and k["data64"].shape == (len(k["stored"]), 19, k["n"])
        assert k["pose"].dtype == np.float32 and k["pose"].shape == (k["updates"], 7, k["n"])
        assert k["mask"].shape == (k["records"], k["n"]) and k["mask"][0].all()
        assert any(x != 0 for x in k["com"])
    assert (a["n"], a["updates"], a["records"]) == (67, 48, 48) and a["mask"].all()
    assert a["offset_pos"] == [0, 0, 0] and a["offset_rot"] == [1, 0, 0, 0]
    assert a["gravity_bias"] == [0, 0, float(np.float32(9.81))]
    q = a["pose"][:, 3:7].astype(np.float64)
    tilt = np.arccos(np.clip(1 - 2 * (q[:, 1] ** 2 + q[:, 2] ** 2), -1, 1))
    assert 0.5 < tilt.max() <= 0.6 + 1e-6 and 4 < np.linalg.norm(a["vel"][:, 3:6], axis=1).max() <= 6 + 1e-5
    # b: the same motion, a tilted offset, no bias, read every fourth update, then the reset envs read again
    assert b["motion"] == "a" and b["offset_pos"] == [float(np.float32(x)) for x in (0.1, -0.05, 0.2)]
    assert sum(x != 0 for x in b["offset_rot"]) == 4 and b["gravity_bias"] == [0, 0, 0]
    assert b["upd"].tolist() == [u for u in range(3, 48, 4) for _ in (0, 1)]
    assert b["mask"][0::2].all() and not b["mask"][1::2].all(1).any() and b["mask"][1::2].sum() >= b["n"]
    # c: masked resets in updates already read
    assert c["n"] == 3 and c["mask"].tolist() == [[1, 1, 1], [1, 1, 1], [0, 1, 0], [1, 1, 1], [1, 0, 1], [1, 1, 1]]
    assert c["upd"].tolist() == [0, 1, 1, 2, 2, 3]
    assert os.path.getsize(ic.GOLDEN) < 500_000


@needs_cxx
def test_plain_build_equals_the_restatement_bit_for_bit(program_outputs, restated):
    cases, outs, stdout = program_outputs
    print(stdout)
    assert f"imu: {len(cases)} cases" in stdout and "layout and rows: 0 mismatches" in stdout
    _same_as_restatement(cases, outs, restated)


@needs_cxx
def test_sanitized_build_runs_clean_and_equals_the_restatement(tmp_path, restated):
    exe = str(tmp_path / "imu_check_san")
    ic.build_program(exe, ic.SANITIZE)
    cases = ic.all_cases()
    stdout, outs = ic.run_program(exe, str(tmp_path), cases)
    assert "layout and rows: 0 mismatches" in stdout
    _same_as_restatement(cases, outs, restated)


@needs_cxx
def test_outputs_against_the_reference_in_float64(program_outputs):
    cases, outs, _ = program_outputs
    seen = 0
    for c, o in zip(cases, outs):
        if "e_ref" not in c:
            continue
        got = o["data"][c["stored"]].astype(np.float64)
        for field, lo, hi in ic.FIELDS:
            err, e_ref = np.abs(got[:, lo:hi] - c["data64"][:, lo:hi]).max(), c["e_ref"][field]
            print(f"case {c['name']} {field}: error {err:.3e}, E_ref {e_ref:.3e}, ratio "
                  f"{err / e_ref if e_ref else 0.0:.3f} (bound 2)")
            assert err <= 2.0 * e_ref, (c["name"], field, err, e_ref)
            seen += 1
    assert seen == 18


@needs_cxx
def test_hand_cases_give_their_exact_answers(program_outputs):
    cases, outs, _ = program_outputs
    seen = []
    for c, o in zip(cases, outs):
        if "expect" not in c:
            continue
        assert np.array_equal(o["data"], c["expect"]), (c["name"], o["data"][..., 0], c["expect"][..., 0])
        assert np.array_equal(o["prev"], c["expect_prev"]), (c["name"], o["prev"][..., 0])
        seen.append(c["name"])
    assert seen == ["h_identity", "h_com", "h_body_180z", "h_sensor_180x", "h_outdated"]
    ident = outs[cases.index(next(c for c in cases if c["name"] == "h_identity"))]["data"][:, :, 0]
    assert ident[0, 13:16].tolist() == [4, 4, 8] and ident[1, 13:16].tolist() == [0, 0, 8]


def test_restatement_answers_the_hand_cases_and_keeps_unflagged_envs():
    """No compiler needed: the NumPy restatement on the hand cases, and the per-env rule on the fixture -- an env
    outside a record's mask keeps data and prev bit for bit."""
    for c in ic.hand_cases():
        d, p = ic.replay(c)
        assert np.array_equal(d, c["expect"]) and np.array_equal(p, c["expect_prev"]), c["name"]
    for c in ic.load_cases():
        d, p = ic.replay(c)
        for r in range(1, len(c["upd"])):
            keep = c["mask"][r] == 0
            assert np.array_equal(d[r][:, keep].view(np.uint32), d[r - 1][:, keep].view(np.uint32))
            assert np.array_equal(p[r][:, keep].view(np.uint32), p[r - 1][:, keep].view(np.uint32))
            if c["name"] != "a" and not keep.all():
                assert not np.array_equal(d[r][13:16, ~keep], d[r - 1][13:16, ~keep])


@pytest.mark.skipif(not os.path.isdir(REFERENCE), reason="no reference checkout given (ALLSTEPS_REFERENCE)")
def test_fixture_regenerates_bit_for_bit():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "golden", "gen_imu.py"), "--check",
                        "--reference", REFERENCE], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert "identical" in r.stdout
