"""The ray caster's shared code (csrc/allsteps_ray_caster.h) on the host.

tests/ray_caster_check.cpp is a stand-alone program (its own main) around the header.  Built once plain and once with
-fsanitize=address,undefined; both run directly.  Its output must equal tests/golden/ray_caster_host.npz -- what the
GPU kernel is held to -- bit for bit, and the hand cases e (_ray_caster_cases.E_SCENES) their stated exact answers.

Frames: the header's world rays against the reference's own float64 world rays (tests/golden/ray_caster.npz, from
the reference's RayCaster code: gen_ray_caster.py) within 4 E_ref per case, E_ref being the reference's own
float32-against-float64 difference on the same inputs; 2 E_ref for case f, which uses no transcendentals.  (The
bounds include/as_detmath.h states -- as_atan2f <= 2.5 ulp, as_sincosf about 2 ulp -- imply no more than that here:
a yaw error of 2.5 ulp of pi, 6e-7 rad, moves a grid corner 0.94 m from the axis by 5.6e-7 m, under E_ref = 8.3e-7 m,
which is itself dominated by the rounding of z = 20 + root height.)

Hits: each ray's own float32 world start and direction promoted to double, then the float64 slab oracle of
_ray_caster_cases (independent of the header): equal surfaces, |hit - hit64|inf <= 8 eps32 (|o|inf + |c|inf + |h|inf
+ t |d|inf); rays within 1e-4 m of a box edge skipped, at most 2 % per case; stone hits at least 20 % per case."""

import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _ray_caster_cases as rc  # noqa: E402

REFERENCE = os.environ.get("ALLSTEPS_REFERENCE", "")
needs_cxx = pytest.mark.skipif(rc.CXX is None, reason="no host C++ compiler")


@pytest.fixture(scope="module")
def program_outputs(tmp_path_factory):
    """The plain build's outputs on every case: (cases, outputs per case, stdout)."""
    tmp = tmp_path_factory.mktemp("ray_caster_plain")
    exe = str(tmp / "ray_caster_check")
    rc.build_program(exe)
    cases = rc.all_cases()
    stdout, outs = rc.run_program(exe, str(tmp), cases)
    return cases, outs, stdout


def _same_as_host_fixture(cases, outs):
    host = rc.load_host()
    assert set(host) == {c["name"] for c in cases}
    for c, r in zip(cases, outs):
        h = host[c["name"]]
        assert np.array_equal(r["hits"].view(np.uint32), h["hits"].view(np.uint32)), c["name"]
        assert np.array_equal(r["surface"], h["surface"]) and h["surface"].dtype == np.int8, c["name"]
        assert np.array_equal(r["pose"].view(np.uint32), h["pose"].view(np.uint32)), c["name"]


def test_fixture_has_the_cases_the_issue_names():
    cases = {c["name"]: c for c in rc.load_cases()}
    assert set(cases) == {"y", "f", "d"}
    y, f, d = cases["y"], cases["f"], cases["d"]
    assert (y["n"], y["num_rays"], y["attach_yaw_only"]) == (24, 187, True)
    assert y["cfg"]["offset_pos"] == [0.0, 0.0, 20.0] and y["cfg"]["size"] == [1.6, 1.0]
    assert y["cfg"]["resolution"] == 0.1 and y["cfg"]["mesh_prim_paths"] == ["/World/ground"]
    assert (f["n"], f["num_rays"], f["attach_yaw_only"]) == (24, 63, False)
    assert f["cfg"]["offset_pos"] == [0.1, 0.0, 0.3] and f["cfg"]["offset_rot"][2] != 0.0 and f["cfg"]["size"] == [0.8, 0.6]
    assert d["cfg"]["direction"] == [0.3, 0.0, -1.0] and d["cfg"]["ordering"] == "yx" and d["num_rays"] == 187
    for k in ("root_pos", "root_quat", "stones"):
        assert np.array_equal(d[k], y[k])  # "case y with ..."
    for c in cases.values():
        assert c["starts_w"].dtype == np.float32 and c["starts_w64"].dtype == np.float64
        assert c["starts_w"].shape == (c["n"], c["num_rays"], 3) and 0 < c["e_ref"] < 1e-5
        e = max(np.abs(c["starts_w"] - c["starts_w64"]).max(), np.abs(c["dirs_w"] - c["dirs_w64"]).max())
        assert e == c["e_ref"]
        # the poses: 0.5-1.3 m over a stone, tilted up to 0.6 rad, yaw over the circle
        q = c["root_quat"].astype(np.float64)
        tilt = np.arccos(np.clip(1 - 2 * (q[1] ** 2 + q[2] ** 2), -1, 1))
        yaw = np.arctan2(2 * (q[0] * q[3] + q[1] * q[2]), 1 - 2 * (q[2] ** 2 + q[3] ** 2))
        assert tilt.max() <= 0.6 + 1e-6 and tilt.max() > 0.3 and yaw.min() < -2 and yaw.max() > 2
    assert os.path.getsize(rc.GOLDEN) < 500_000


@needs_cxx
def test_plain_build_equals_the_host_fixture_bit_for_bit(program_outputs):
    cases, outs, stdout = program_outputs
    print(stdout)
    assert f"ray caster: {len(cases)} cases" in stdout and ", 0 mismatches" in stdout.split("ray caster:")[1]
    assert "layout and codes: 0 mismatches" in stdout
    _same_as_host_fixture(cases, outs)


@needs_cxx
def test_sanitized_build_runs_clean_and_equals_the_host_fixture(tmp_path):
    exe = str(tmp_path / "ray_caster_check_san")
    rc.build_program(exe, rc.SANITIZE)
    cases = rc.all_cases()
    stdout, outs = rc.run_program(exe, str(tmp_path), cases)
    assert "layout and codes: 0 mismatches" in stdout
    _same_as_host_fixture(cases, outs)


@needs_cxx
def test_hand_cases_give_their_exact_answers(program_outputs):
    cases, outs, _ = program_outputs
    seen = 0
    for c, r in zip(cases, outs):
        if "expect_hits" not in c:
            continue
        assert np.array_equal(r["hits"].view(np.uint32), c["expect_hits"].view(np.uint32)), \
            (c["name"], r["hits"][:, :, 0].T, c["expect_hits"][:, :, 0].T)
        assert np.array_equal(r["surface"], c["expect_surface"]), (c["name"], r["surface"][:, 0])
        seen += c["num_rays"]
    assert seen == sum(len(s[3]) for s in rc.E_SCENES) >= 18


@needs_cxx
def test_frames_against_the_reference_in_float64(program_outputs):
    cases, outs, _ = program_outputs
    for c, r in zip(cases, outs):
        if "e_ref" not in c:
            continue
        starts, dirs = r["starts_w"].transpose(2, 1, 0), r["dirs_w"].transpose(2, 1, 0)
        err = max(np.abs(starts - c["starts_w64"]).max(), np.abs(dirs - c["dirs_w64"]).max())
        factor = 2.0 if c["name"] == "f" else 4.0
        print(f"case {c['name']}: frame error {err:.3e}, E_ref {c['e_ref']:.3e}, ratio {err / c['e_ref']:.3f} "
              f"(bound {factor})")
        assert err <= factor * c["e_ref"], c["name"]
        if c["attach_yaw_only"]:  # directions are the local ones, as bits
            assert np.array_equal(dirs.view(np.uint32), c["dirs_w"].view(np.uint32))


@needs_cxx
def test_hits_against_the_float64_oracle(program_outputs):
    cases, outs, _ = program_outputs
    for c, r in zip(cases, outs):
        if "e_ref" not in c:
            continue
        skipped, stone_share, worst = rc.check_hits(
            c["name"], r["starts_w"].transpose(2, 1, 0), r["dirs_w"].transpose(2, 1, 0), r["hits"].transpose(2, 1, 0),
            r["surface"].T, rc.stones_nk3(c["stones"]), c["half"], c["surfaces"], c["max_distance"], c["ground_z"])
        print(f"case {c['name']}: skipped {skipped:.4%}, stone hits {stone_share:.2%}, worst error / bound {worst:.3f}")
        assert skipped <= 0.02 and stone_share >= 0.20, c["name"]


def test_oracle_answers_the_hand_cases_too():
    """The float64 oracle, which shares no code with the header, gives the hand cases' stated answers."""
    for c in rc.hand_cases():
        o = np.ascontiguousarray(c["rays"][:3].T)[None].astype(np.float64)  # the world ray is the local one
        d = np.ascontiguousarray(c["rays"][3:].T)[None].astype(np.float64)
        t, s, hit = rc.oracle64(o, d, rc.stones_nk3(c["stones"]), c["half"], c["surfaces"], c["max_distance"], 0.0)
        assert np.array_equal(s[0], c["expect_surface"][:, 0]), c["name"]
        assert np.array_equal(hit[0], c["expect_hits"][:, :, 0].T.astype(np.float64)), c["name"]


@pytest.mark.skipif(not os.path.isdir(REFERENCE), reason="no reference checkout given (ALLSTEPS_REFERENCE)")
def test_fixture_regenerates_bit_for_bit():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "golden", "gen_ray_caster.py"), "--check",
                        "--reference", REFERENCE], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert "identical" in r.stdout
