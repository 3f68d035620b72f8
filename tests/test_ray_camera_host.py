"""The ray-cast camera's shared code (csrc/allsteps_ray_camera.h) and host side (envs/ray_camera.py) without a device.

tests/ray_camera_check.cpp is a stand-alone program (its own main) around the header.  Built once plain and once with
-fsanitize=address,undefined; both run directly.  Its output must equal the NumPy float32 restatement
(_ray_camera_cases.restate) -- what the GPU kernel is held to -- bit for bit on every case, and the hand cases their
stated exact answers.

Against the fixture (tests/golden/ray_camera.npz, from the reference's own RayCasterCamera code: gen_ray_camera.py):
the intrinsic matrices equal the reference's float32 values exactly (Python-float arithmetic stored to float32);
every other array lies within 2 E_ref of the reference's float64 run, E_ref being the reference's own
float32-against-float64 difference on the same inputs -- the project's margin for arithmetic without
transcendentals.  Quaternions are compared up to sign; NaN and inf positions must be identical.  The measured ratios
are printed."""

import dataclasses
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _ray_camera_cases as cc  # noqa: E402

REFERENCE = os.environ.get("ALLSTEPS_REFERENCE", "")
needs_cxx = pytest.mark.skipif(cc.CXX is None, reason="no host C++ compiler")


@pytest.fixture(scope="module")
def fx():
    return cc.load_fixture()


def _cases(fx) -> list:
    """The hand cases and the fixture's world case under every clipping and surface selection."""
    out = cc.hand_cases()
    mx = fx["meta"]["max_distance"]
    for clip in ("none", "max", "zero"):
        out.append(dict(cc.world_case(fx, clipping=cc.CLIP[clip], max_distance=mx), name=f"w_{clip}"))
    out.append(dict(cc.world_case(fx, surfaces=cc.GROUND), name="w_ground"))
    out.append(dict(cc.world_case(fx, surfaces=cc.STONES, clipping=cc.CLIP_ZERO, max_distance=mx), name="w_stones"))
    return out


@pytest.fixture(scope="module")
def cases(fx):
    return _cases(fx)


@pytest.fixture(scope="module")
def restated(cases):
    return [cc.restate(c) for c in cases]


def _equal_restatement(cases, outs, restated):
    for c, r, w in zip(cases, outs, restated):
        for k, _ in cc.OUTPUTS:
            assert cc.same_bits(r[k], w[k]) == 0, (c["name"], k)


@needs_cxx
def test_host_program_equals_the_restatement_bit_for_bit(tmp_path, cases, restated):
    exe = str(tmp_path / "ray_camera_check")
    cc.build_program(exe)
    stdout, outs = cc.run_program(exe, str(tmp_path), cases)
    print(stdout)
    assert " 0 mismatches" in stdout.splitlines()[-2] and "layout and codes: 0 mismatches" in stdout
    _equal_restatement(cases, outs, restated)


@needs_cxx
def test_sanitized_host_program_equals_the_restatement_bit_for_bit(tmp_path, cases, restated):
    """The same program under AddressSanitizer and UBSan, run directly (nothing is preloaded)."""
    exe = str(tmp_path / "ray_camera_check_san")
    cc.build_program(exe, cc.SANITIZE)
    stdout, outs = cc.run_program(exe, str(tmp_path), cases)
    assert "layout and codes: 0 mismatches" in stdout
    _equal_restatement(cases, outs, restated)


def test_world_case_has_hits_misses_and_stones(cases, restated):
    r = restated[[c["name"] for c in cases].index("w_none")]
    assert (r["surface"] >= 0).sum() > 50 and (r["surface"] == cc.HIT_GROUND).sum() > 50
    assert (r["surface"] == cc.MISS).sum() > 50
    assert np.array_equal(np.isnan(r["plane"]), np.isinf(r["camera"]))
    assert np.array_equal(np.isinf(r["normals"]).all(-1), r["surface"] == cc.MISS)
    hit = r["surface"] != cc.MISS
    assert np.array_equal(np.abs(r["normals"][hit]).sum(-1), np.ones(hit.sum(), np.float32))  # axis-aligned, unit
    assert len({tuple(x) for x in r["normals"][r["surface"] >= 0]}) >= 3  # tops and sides


def test_hand_cases_have_their_exact_answers(cases, restated):
    seen = 0
    for c, r in zip(cases, restated):
        if "expect" not in c:
            continue
        for k, want in c["expect"].items():
            got = r[k]
            assert got.shape == want.shape, (c["name"], k)
            assert np.array_equal(np.isnan(got), np.isnan(want)), (c["name"], k, got, want)
            fin = ~np.isnan(want)
            assert np.array_equal(got[fin], want[fin]), (c["name"], k, got.ravel(), want.ravel())
        seen += 1
    assert seen == len(cc.HAND) >= 9


# ------------------------------------------------------------------------------------------- against the fixture
def _ratio(name, got, want64, e_ref, up_to_sign=False) -> float:
    """max |got - want64| / E_ref over the finite entries; NaN and inf positions must be identical."""
    got, want = np.asarray(got, np.float64), np.asarray(want64, np.float64)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    if up_to_sign:
        want = np.where(np.sum(got * want, -1, keepdims=True) < 0, -want, want)
    assert np.array_equal(np.isnan(got), np.isnan(want)), (name, "NaN positions differ")
    assert np.array_equal(np.isposinf(got), np.isposinf(want)), (name, "+inf positions differ")
    assert np.array_equal(np.isneginf(got), np.isneginf(want)), (name, "-inf positions differ")
    fin = np.isfinite(want)
    err = float(np.abs(got[fin] - want[fin]).max())
    ratio = err / e_ref if e_ref > 0 else (0.0 if err == 0.0 else np.inf)
    print(f"{name}: max error {err:.3e}, E_ref {e_ref:.3e}, ratio {ratio:.3f}")
    return ratio


def _pattern(fields: dict):
    from allsteps_isaaclab_amd.utils.patterns import PinholeCameraPatternCfg

    if fields.get("intrinsic_matrix"):
        p = PinholeCameraPatternCfg.from_intrinsic_matrix(fields["intrinsic_matrix"], fields["width"],
                                                          fields["height"], focal_length=fields["focal_length"])
        for f in dataclasses.fields(p):
            if f.name != "func":
                assert getattr(p, f.name) == fields[f.name], f.name  # the same Python-float arithmetic
        return p
    return PinholeCameraPatternCfg(**{k: v for k, v in fields.items() if k != "intrinsic_matrix"})


def _spec(pattern, **kw):
    from allsteps_isaaclab_amd.envs.ray_camera import RayCameraSpec
    from allsteps_isaaclab_amd.utils.sensors import RayCasterCameraCfg

    cfg = RayCasterCameraCfg(prim_path="/World/envs/env_.*/Robot/base", mesh_prim_paths=["/World/ground"],
                             pattern_cfg=pattern, **kw)
    return RayCameraSpec(cfg, root_body="base", step_dt=0.02)


@pytest.mark.parametrize("name", ["p0", "p1", "p2"])
def test_patterns_against_the_reference(fx, name):
    fields = dict(fx["meta"]["patterns"][name])
    if name == "p0":
        fields["vertical_aperture"] = None  # the defaults: the spec fills it in as the reference does
    spec = _spec(_pattern(fields))
    assert spec.intrinsics.dtype == np.float32 and np.array_equal(spec.intrinsics, fx[f"{name}_intrinsics"])
    assert spec.dirs.shape == (3, fields["width"] * fields["height"]) and spec.dirs.dtype == np.float32
    assert _ratio(f"{name}_dirs", spec.dirs.T, fx[f"{name}_dirs64"], fx["meta"]["e_ref"][f"{name}_dirs"]) <= 2.0


def test_pattern_pixel_order_is_row_major(fx):
    """Pixel (row v, column u) is ray v W + u: along a row y (left) falls, down a column z (up) falls."""
    spec = _spec(_pattern(dict(fx["meta"]["patterns"]["p1"])))
    d = spec.dirs.reshape(3, 6, 8)
    assert (np.diff(d[1], axis=1) < 0).all() and (np.diff(d[2], axis=0) < 0).all() and (d[0] > 0).all()


@pytest.mark.parametrize("convention", ["opengl", "ros", "world"])
def test_offset_quaternion_against_the_reference(fx, convention):
    from allsteps_isaaclab_amd.envs.ray_camera import offset_quat_to_world

    for i, rot in enumerate(fx["meta"]["o_rots"]):
        key = f"o_{convention}_{i}"
        got = np.asarray(offset_quat_to_world(rot, convention), np.float32)
        assert _ratio(key, got, fx[key + "64"], fx["meta"]["e_ref"][key], up_to_sign=True) <= 2.0
        spec = _spec(_pattern(dict(fx["meta"]["patterns"]["p1"])),
                     offset=_offset_cfg(rot=tuple(rot), convention=convention))
        assert np.array_equal(spec.offset[3:], got) and np.array_equal(spec.offset[:3], np.zeros(3, np.float32))


def _offset_cfg(**kw):
    from allsteps_isaaclab_amd.utils.sensors import RayCasterCameraCfg

    return RayCasterCameraCfg.OffsetCfg(**kw)


def test_world_poses_and_directions_against_the_reference(fx, cases, restated):
    from allsteps_isaaclab_amd.envs.ray_camera import quat_from_world_torch

    r = restated[[c["name"] for c in cases].index("w_none")]
    e = fx["meta"]["e_ref"]
    assert _ratio("w_pos_w", r["pose"][:3].T, fx["w_pos_w64"], e["w_pos_w"]) <= 2.0
    assert _ratio("w_quat_w_world", r["pose"][3:].T, fx["w_quat_w_world64"], e["w_quat_w_world"], True) <= 2.0
    assert _ratio("w_dirs_w", r["dirs_w"], fx["w_dirs_w64"], e["w_dirs_w"]) <= 2.0
    quat = torch.from_numpy(np.ascontiguousarray(r["pose"][3:].T))
    for conv in ("ros", "opengl"):
        got = quat_from_world_torch(quat, conv).numpy()
        assert got.dtype == np.float32
        assert _ratio(f"w_quat_w_{conv}", got, fx[f"w_quat_w_{conv}64"], e[f"w_quat_w_{conv}"], True) <= 2.0


def test_spec_reproduces_the_fixture_inputs_of_the_world_case(fx):
    """The spec's own directions and offset for case w's cfg.  The directions: within 3 E_ref of the reference's
    float32 ones (the spec's lie within 2 E_ref of the float64 run -- case p0 -- and the reference's own within
    E_ref).  The offset quaternion: up to sign within one float32 unit in the last place of 1 of the reference's."""
    m = fx["meta"]["w"]
    spec = _spec(_pattern(dict(fx["meta"]["patterns"]["p0"], vertical_aperture=None)),
                 offset=_offset_cfg(pos=tuple(m["cfg"]["offset_pos"]), rot=tuple(m["cfg"]["offset_rot"]),
                                    convention=m["cfg"]["convention"]))
    assert np.abs(spec.dirs - fx["w_dirs"]).max() <= 3 * fx["meta"]["e_ref"]["p0_dirs"]
    ref = fx["w_offset"][:, 0]
    assert np.array_equal(spec.offset[:3], ref[:3])
    q = spec.offset[3:] * np.sign(np.dot(spec.offset[3:], ref[3:]))
    assert np.abs(q - ref[3:]).max() <= 2 ** -23


@pytest.mark.parametrize("clip", ["none", "max", "zero"])
def test_post_processing_against_the_reference(fx, clip):
    """Case z: the reference's post-processing of a depth image the fixture supplies (the same array in its float32
    and float64 runs), here through the restatement with that depth in place of the cast's."""
    meta = fx["meta"]
    assert min(meta["z"].values()) > 50  # clipped, unclipped, misses, stone hits
    c = cc.world_case(fx, clipping=cc.CLIP[clip], max_distance=meta["max_distance"])
    r = cc.restate(c, depth=fx["z_depth"])
    e = meta["e_ref"]
    assert _ratio(f"z_{clip}_plane", r["plane"], fx[f"z_{clip}_plane64"], e[f"z_{clip}_plane"]) <= 2.0
    assert _ratio(f"z_{clip}_camera", r["camera"], fx[f"z_{clip}_camera64"], e[f"z_{clip}_camera"]) <= 2.0
    if clip == "none":
        assert np.array_equal(np.isnan(r["plane"]), np.isinf(fx["z_depth"]))
        assert np.array_equal(r["camera"], fx["z_depth"])
    else:
        assert np.isfinite(r["plane"]).all() and np.isfinite(r["camera"]).all()
        assert r["camera"].max() <= np.float32(meta["max_distance"])


@pytest.mark.parametrize("convention", ["ros", "world"])
def test_set_world_poses_against_the_reference(fx, convention):
    from allsteps_isaaclab_amd.envs.ray_camera import world_pose_offsets

    ids = fx["s_env_ids"]
    rp = torch.from_numpy(np.ascontiguousarray(fx["w_root_pos"][:, ids].T))
    rq = torch.from_numpy(np.ascontiguousarray(fx["w_root_quat"][:, ids].T))
    pos, quat = world_pose_offsets(rp, rq, torch.from_numpy(fx["s_positions"]), torch.from_numpy(fx["s_orientations"]),
                                   convention)
    assert pos.dtype == torch.float32 and quat.dtype == torch.float32
    want = fx[f"s_{convention}_offset64"]
    e = fx["meta"]["e_ref"]
    assert _ratio(f"s_{convention}_offset_pos", pos.numpy(), want[:3, ids].T, e[f"s_{convention}_offset_pos"]) <= 2.0
    assert _ratio(f"s_{convention}_offset_quat", quat.numpy(), want[3:, ids].T, e[f"s_{convention}_offset_quat"],
                  up_to_sign=True) <= 2.0
    others = np.setdiff1d(np.arange(want.shape[1]), ids)
    assert np.array_equal(fx[f"s_{convention}_offset"][:, others], fx["w_offset"][:, others])  # untouched envs


def test_fixture_is_small():
    assert os.path.getsize(cc.GOLDEN) < 500_000


@pytest.mark.skipif(not os.path.isdir(REFERENCE), reason="no reference checkout given (ALLSTEPS_REFERENCE)")
def test_fixture_regenerates_bit_for_bit():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "golden", "gen_ray_camera.py"), "--check",
                        "--reference", REFERENCE], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    assert "identical" in r.stdout
