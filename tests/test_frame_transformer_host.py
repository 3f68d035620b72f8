"""The frame transformer's shared code (csrc/allsteps_frame_transformer.h) on the host.

tests/frame_transformer_check.cpp is a stand-alone program (its own main) around the header.  Built once plain and
once with -fsanitize=address,undefined; both run directly.  Its outputs must be

  * within 2 x E_ref of the reference's own float64 outputs, per output field and per case of
    tests/golden/frame_transformer.npz (gen_frame_transformer.py: the reference's FrameTransformer, SensorBase and
    math code over a fake stage and a fake PhysX view), E_ref being the reference's own float32-against-float64
    difference on the same inputs; a field whose E_ref is 0 (a pose handed through) must be exact.  2 x is the
    project's margin for arithmetic without transcendentals (test_imu_host.py); the slack exists because torch's
    norm and cross fix neither the summation order nor the use of FMA.  Measured: at most 1.14 x (case b,
    target_pos_source), 1.00 x or less elsewhere;
  * the stated exact answers on the hand cases (_frame_transformer_cases.hand_cases: identity, a body turned 180
    degrees about z, a source offset only, a target offset only, both, a stone target);
  * equal, bit for bit, to the NumPy float32 restatement of _frame_transformer_cases on every case -- the
    restatement the GPU tests hold the kernel to;
  * and the frame names of the package's host resolution (FrameTransformerSpec) must be the reference's, case by
    case."""

import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _frame_transformer_cases as fc  # noqa: E402

REFERENCE = os.environ.get("ALLSTEPS_REFERENCE", "")
needs_cxx = pytest.mark.skipif(fc.CXX is None, reason="no host C++ compiler")


@pytest.fixture(scope="module")
def program_outputs(tmp_path_factory):
    """The plain build's outputs on every case: (cases, outputs per case, stdout)."""
    tmp = tmp_path_factory.mktemp("frame_transformer_plain")
    exe = str(tmp / "frame_transformer_check")
    fc.build_program(exe)
    cases = fc.all_cases()
    stdout, outs = fc.run_program(exe, str(tmp), cases)
    return cases, outs, stdout


@pytest.fixture(scope="module")
def restated():
    return [fc.replay(c) for c in fc.all_cases()]


def _same_as_restatement(cases, outs, restated):
    for c, o, (s, t) in zip(cases, outs, restated):
        assert np.array_equal(o["source"].view(np.uint32), s.view(np.uint32)), c["name"]
        assert np.array_equal(o["target"].view(np.uint32), t.view(np.uint32)), c["name"]


def test_fixture_has_the_cases_the_issue_names_and_the_spec_gives_the_reference_frame_names():
    cases = {c["name"]: c for c in fc.load_cases()}
    assert set(cases) == {"a", "b", "c"}
    a, b, c = cases["a"], cases["b"], cases["c"]
    for k in cases.values():
        fields = {f for f, _, _ in fc.SOURCE_FIELDS + fc.TARGET_FIELDS}
        assert set(k["e_ref"]) == fields and len(k["upd"]) == k["records"]
        nf = len(k["target_frame_names"])
        assert k["source64"].dtype == np.float64 and k["source64"].shape == (len(k["stored"]), 7, k["n"])
        assert k["target64"].dtype == np.float64 and k["target64"].shape == (len(k["stored"]), 14, nf, k["n"])
        assert k["pose"].dtype == np.float32 and k["pose"].shape == (k["updates"], len(k["bodies"]), 7, k["n"])
        # the package's host resolution: the reference's names, order and switches
        assert k["frame_names"] == k["target_frame_names"], k["name"]
        assert (k["apply_source"], k["apply_target"]) == (k["apply_source_offset"], k["apply_target_offset"])
        assert len(set(b for b, _ in k["frames"])) == nf  # one frame per body in the fixture
    assert (a["n"], a["updates"], b["n"], b["motion"]) == (67, 24, 67, a["motion"])
    assert a["target_frame_names"] == ["left_foot", "right_foot"] and not a["apply_source"] and not a["apply_target"]
    assert all(a["e_ref"][f] == 0 for f in ("source_pos_w", "source_quat_w", "target_pos_w", "target_quat_w"))
    # b: a tilted, unnormalised source offset; one target with an offset, one without; cfg order right before left
    rot = np.asarray(b["cfg"]["source_frame_offset"]["rot"])
    assert (rot != 0).all() and abs(np.linalg.norm(rot) - 1) > 0.01
    assert b["target_frame_names"] == ["toe", "right_foot"] and b["apply_source"] and b["apply_target"]
    assert [t["prim_path"].split("/")[-1] for t in b["cfg"]["target_frames"]] == ["right_foot", "left_foot"]
    assert b["frames"][1][1].tolist() == [0, 0, 0, 1, 0, 0, 0] and all(v > 0 for v in b["e_ref"].values())
    # c: the source is a target too; stones of num_steps = 12 after the robot's bodies, step_10 before step_2
    names = c["target_frame_names"]
    assert c["n"] == 3 and c["num_steps"] == 12 and len(names) == 17 + 12 and "torso" in names
    assert names.index("step_10") == names.index("step_1") + 1 < names.index("step_2")
    assert names.index("walker3d") < names.index("step_0")
    assert c["upd"] == [0, 1, 2, 3, 3]  # a masked reset, then a second read in the last update
    stone = c["bodies"].index("step_3")
    assert np.array_equal(c["pose"][:, stone, 3:], np.broadcast_to(np.float32([1, 0, 0, 0])[None, :, None], (4, 4, 3)))
    assert os.path.getsize(fc.GOLDEN) < 500_000


@needs_cxx
def test_plain_build_equals_the_restatement_bit_for_bit(program_outputs, restated):
    cases, outs, stdout = program_outputs
    print(stdout)
    assert f"frame_transformer: {len(cases)} cases" in stdout and "layout and rows: 0 mismatches" in stdout
    _same_as_restatement(cases, outs, restated)


@needs_cxx
def test_sanitized_build_runs_clean_and_equals_the_restatement(tmp_path, restated):
    exe = str(tmp_path / "frame_transformer_check_san")
    fc.build_program(exe, fc.SANITIZE)
    cases = fc.all_cases()
    stdout, outs = fc.run_program(exe, str(tmp_path), cases)
    assert "layout and rows: 0 mismatches" in stdout
    _same_as_restatement(cases, outs, restated)


def _against_reference(cases, outputs):
    seen = 0
    for c, (source, target) in zip(cases, outputs):
        if "e_ref" not in c:
            continue
        rec = [c["upd"][r] for r in c["stored"]]
        got = {"source": source[rec].astype(np.float64), "target": target[rec].astype(np.float64)}
        for buf, fields in (("source", fc.SOURCE_FIELDS), ("target", fc.TARGET_FIELDS)):
            for field, lo, hi in fields:
                err, e_ref = np.abs(got[buf][:, lo:hi] - c[buf + "64"][:, lo:hi]).max(), c["e_ref"][field]
                print(f"case {c['name']} {field}: error {err:.3e}, E_ref {e_ref:.3e}, ratio "
                      f"{err / e_ref if e_ref else 0.0:.3f} (bound 2)")
                assert err <= 2.0 * e_ref, (c["name"], field, err, e_ref)
                seen += 1
    assert seen == 18


@needs_cxx
def test_outputs_against_the_reference_in_float64(program_outputs):
    cases, outs, _ = program_outputs
    _against_reference(cases, [(o["source"], o["target"]) for o in outs])


def test_restatement_against_the_reference_in_float64(restated):
    """No compiler needed: the same bound on the NumPy restatement."""
    _against_reference(fc.all_cases(), restated)


@needs_cxx
def test_hand_cases_give_their_exact_answers(program_outputs):
    cases, outs, _ = program_outputs
    seen = []
    for c, o in zip(cases, outs):
        if "expect_source" not in c:
            continue
        assert np.array_equal(o["source"], c["expect_source"]), (c["name"], o["source"][0, :, 0])
        assert np.array_equal(o["target"], c["expect_target"]), (c["name"], o["target"][0, :, :, 0].T)
        seen.append(c["name"])
    assert seen == ["h_identity", "h_body_180z", "h_source_offset", "h_target_offset", "h_both", "h_stone"]


def test_restatement_answers_the_hand_cases_and_the_switches_matter_for_bits():
    """No compiler needed: the NumPy restatement on the hand cases; and on the fixture's motion, applying an identity
    offset is not the same bits as skipping it -- the reason the switches are the reference's."""
    for c in fc.hand_cases():
        s, t = fc.replay(c)
        assert np.array_equal(s, c["expect_source"]) and np.array_equal(t, c["expect_target"]), c["name"]
    a = next(c for c in fc.load_cases() if c["name"] == "a")
    skipped = fc.replay(a)
    applied = fc.replay(dict(a, apply_source=True, apply_target=True))
    assert not np.array_equal(skipped[0][:, 3:7], applied[0][:, 3:7])  # quat_mul(q, (1, 0, 0, 0)) != q somewhere
    assert not np.array_equal(skipped[1], applied[1])
    assert np.abs(skipped[1] - applied[1]).max() < 1e-5


@pytest.mark.skipif(not os.path.isdir(REFERENCE), reason="no reference checkout given (ALLSTEPS_REFERENCE)")
def test_fixture_regenerates_bit_for_bit():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "golden", "gen_frame_transformer.py"), "--check",
                        "--reference", REFERENCE], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert "identical" in r.stdout
