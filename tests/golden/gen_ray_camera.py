"""Generate tests/golden/ray_camera.npz from the reference's own ray-cast camera code.

Loads ``isaaclab/sensors/ray_caster/patterns/patterns.py`` (and ``patterns_cfg.py``, for ``from_intrinsic_matrix``),
``isaaclab/utils/math.py``, ``isaaclab/sensors/sensor_base.py``, ``isaaclab/sensors/ray_caster/ray_caster.py``,
``isaaclab/sensors/ray_caster/ray_caster_camera.py`` and ``isaaclab/sensors/camera/camera_data.py`` of a reference
checkout BY PATH, with stub modules of this file's own (and gen_ray_caster.py's) for the Isaac / Omniverse / warp
packages they import.  A ``RayCasterCamera`` is built with ``object.__new__``; its view is a fake
``ArticulationView`` that returns recorded root poses.  Patterns, intrinsics, offsets, poses and the post-processing
are the reference's real ``_initialize_rays_impl``, ``_update_buffers_impl`` and ``set_world_poses``;
``raycast_mesh`` -- the warp mesh query, which is not installed -- is replaced by a stub that records the world rays
it is handed and returns a depth array this file supplies.

Every array comes twice: as the reference computes it in float32, and ``<name>64`` from the same code on the same
float32 inputs promoted to float64.  ``meta`` (JSON) holds the cfgs and, per array, ``e_ref`` = max |f32 - f64| over
the finite entries: the reference's own float32 noise on these inputs.

  p   patterns p0 (the defaults at 19 x 13), p1 (8 x 6, both aperture offsets, an explicit vertical_aperture), p2
      (16 x 16 via from_intrinsic_matrix): <p>_intrinsics (3, 3), <p>_dirs (R, 3)
  o   o_<convention>_<i>: _offset_quat for the conventions x {identity, the tilted quaternion of gen_imu.py case b}
  w   n = 24 root poses over stone walks (gen_ray_caster.py's), pattern p0, an offset pitched 0.45 rad down, given
      in "ros": w_root_pos (3, n), w_root_quat (4, n), w_stones (60, n), w_dirs (3, R), w_offset (7, n) -- the
      reference's _offset_pos | _offset_quat -- and w_pos_w, w_quat_w_world, w_quat_w_ros, w_quat_w_opengl, w_dirs_w
      (n, R, 3), the world directions handed to raycast_mesh
  z   the post-processing on w: z_depth (n, R) float32 -- this file's float64 analytic cast of the float64 world rays
      rounded to float32, +inf for misses, the SAME array in both runs -- and z_<clip>_plane / z_<clip>_camera (n, R)
      under "none", "max" and "zero" with max_distance chosen so that clipped pixels, unclipped pixels and misses
      all occur
  s   set_world_poses on w's sensor for envs s_env_ids with s_positions / s_orientations, in "ros" and in "world":
      s_<convention>_offset (7, n)

    python tests/golden/gen_ray_camera.py --reference DIR [--check]

--check regenerates into memory and compares with the committed file array by array, bit for bit.
"""

from __future__ import annotations

import argparse
import copy
import dataclasses
import json
import math
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import gen_ray_caster as grc  # noqa: E402
from refload import _mod  # noqa: E402

import _ray_caster_cases as rcc  # noqa: E402  (the float64 slab oracle)

OUT = os.path.join(HERE, "ray_camera.npz")
HALF = grc.HALF
NUM_STONES = grc.NUM_STONES
MAX_DISTANCE = 3.0
CONVENTIONS = ("opengl", "ros", "world")
TYPES = ["distance_to_image_plane", "distance_to_camera", "normals"]


def _configclass(cls):
    """Stands in for isaaclab.utils.configclass: a keyword-only dataclass (fields without a default may follow
    fields with one) whose mutable defaults become factories."""
    for k, v in list(vars(cls).items()):
        if not k.startswith("__") and isinstance(v, (list, dict, set)):
            setattr(cls, k, dataclasses.field(default_factory=lambda v=v: copy.deepcopy(v)))
    return dataclasses.dataclass(cls, kw_only=True)


class _Mesh:
    """Stands in for isaaclab.utils.warp.raycast_mesh: keeps the world rays, returns the depth it was given."""

    def __init__(self):
        self.calls = []
        self.depth = None  # (n, R) or None: all misses

    def __call__(self, ray_starts, ray_directions, mesh=None, max_dist=1e6, return_distance=False,
                 return_normal=False, **kw):
        assert max_dist == 1e6
        self.calls.append((ray_starts.clone(), ray_directions.clone()))
        shape = ray_starts.shape[:2]
        depth = (torch.full(shape, float("inf"), dtype=ray_starts.dtype) if self.depth is None
                 else torch.from_numpy(self.depth).to(ray_starts.dtype))
        hits = ray_starts + depth.unsqueeze(-1) * ray_directions
        return hits, depth.clone(), torch.full_like(ray_starts, float("inf")), None


def load_reference(root: str):
    """(patterns module, patterns_cfg module, math module, camera module, mesh stub) of the reference at ``root``."""
    pt, mt, _, _ = grc.load_reference(root)
    pkg = os.path.join(root, grc.PKG)
    _mod("isaacsim.core.utils")
    _mod("isaacsim.core.utils.stage")
    sys.modules["isaaclab.utils"].configclass = _configclass
    sys.modules["isaaclab.sensors.ray_caster.patterns"].patterns = pt
    pc = grc._load("isaaclab.sensors.ray_caster.patterns.patterns_cfg",
                   os.path.join(pkg, "sensors", "ray_caster", "patterns", "patterns_cfg.py"),
                   "isaaclab.sensors.ray_caster.patterns")
    cd = grc._load("isaaclab.sensors.camera.camera_data", os.path.join(pkg, "sensors", "camera", "camera_data.py"),
                   "isaaclab.sensors.camera")
    _mod("isaaclab.sensors.camera", CameraData=cd.CameraData)
    mesh = _Mesh()
    sys.modules["isaaclab.utils.warp"].raycast_mesh = mesh
    cam = grc._load("isaaclab.sensors.ray_caster.ray_caster_camera",
                    os.path.join(pkg, "sensors", "ray_caster", "ray_caster_camera.py"), "isaaclab.sensors.ray_caster")
    return pt, pc, mt, cam, mesh


def make_camera(cam, pattern, transforms: torch.Tensor, *, offset_pos=(0.0, 0.0, 0.0), offset_rot=(1.0, 0.0, 0.0, 0.0),
                convention="ros", clipping="none", max_distance=1e6):
    s = object.__new__(cam.RayCasterCamera)
    s._initialize_handle = s._invalidate_initialize_handle = s._debug_vis_handle = None  # SensorBase.__del__
    s.cfg = types.SimpleNamespace(
        prim_path="/World/envs/env_.*/Robot/base", mesh_prim_paths=["/World/ground"],
        offset=types.SimpleNamespace(pos=tuple(offset_pos), rot=tuple(offset_rot), convention=convention),
        attach_yaw_only=False, pattern_cfg=pattern, max_distance=max_distance, drift_range=(0.0, 0.0),
        update_period=0.0, history_length=0, debug_vis=False, data_types=list(TYPES), depth_clipping_behavior=clipping)
    s._is_visualizing = False
    s._device = "cpu"
    s._view = grc.ArticulationView(transforms)
    s._data = sys.modules["isaaclab.sensors.camera"].CameraData()
    s.meshes = {"/World/ground": None}
    s._initialize_rays_impl()  # float32: the pattern, the intrinsics and the offset as the reference forms them
    return s


def promote(s, dtype) -> None:
    """The sensor's float tensors in ``dtype`` (the values unchanged)."""
    for k in ("ray_starts", "ray_directions", "_offset_quat", "_offset_pos", "drift", "ray_hits_w"):
        setattr(s, k, getattr(s, k).to(dtype))
    s._view.transforms = s._view.transforms.to(dtype)
    for k in ("pos_w", "quat_w_world", "intrinsic_matrices"):
        setattr(s._data, k, getattr(s._data, k).to(dtype))
    s._data.output = {k: v.to(dtype) for k, v in s._data.output.items()}


def e_ref(a32: np.ndarray, a64: np.ndarray, up_to_sign: bool = False) -> float:
    a, b = a32.astype(np.float64), a64
    if up_to_sign:
        b = np.where((np.sum(a * b, -1, keepdims=True) < 0), -b, b)
    fin = np.isfinite(b)
    assert np.array_equal(fin, np.isfinite(a)) and np.array_equal(np.isnan(a), np.isnan(b))
    with np.errstate(invalid="ignore"):
        return float(np.abs(a - b)[fin].max()) if fin.any() else 0.0


class default_dtype:
    """The reference makes some constants (pixel grids, the convention matrices) in torch's default dtype: a float64
    run sets it for the duration."""

    def __init__(self, dtype):
        self.dtype = dtype

    def __enter__(self):
        torch.set_default_dtype(self.dtype)

    def __exit__(self, *exc):
        torch.set_default_dtype(torch.float32)


def tilted() -> np.ndarray:
    rot = np.array([0.8, 0.3, -0.4, 0.2])  # gen_imu.py case b
    return (rot / np.linalg.norm(rot)).astype(np.float32)


def generate(reference: str) -> dict:
    pt, pc, mt, cam, mesh = load_reference(reference)
    rng = np.random.default_rng(20261022)
    arrays: dict[str, np.ndarray] = {}
    meta: dict = {"e_ref": {}, "half": list(HALF), "max_distance": MAX_DISTANCE}

    def put(name, a32, a64, up_to_sign=False):
        arrays[name], arrays[name + "64"] = np.ascontiguousarray(a32), np.ascontiguousarray(a64)
        assert arrays[name].dtype == np.float32 and arrays[name + "64"].dtype == np.float64, name
        meta["e_ref"][name] = e_ref(arrays[name], arrays[name + "64"], up_to_sign)

    one = torch.tensor([[0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0]])  # a root at the origin, (x, y, z, w) identity

    # ---- p: patterns
    k2 = [310.5, 0.0, 8.25, 0.0, 295.0, 7.5, 0.0, 0.0, 1.0]
    patterns = {
        "p0": pc.PinholeCameraPatternCfg(width=19, height=13),
        "p1": pc.PinholeCameraPatternCfg(width=8, height=6, focal_length=12.0, horizontal_aperture=18.0,
                                         vertical_aperture=15.5, horizontal_aperture_offset=0.031,
                                         vertical_aperture_offset=-0.047),
        "p2": pc.PinholeCameraPatternCfg.from_intrinsic_matrix(k2, width=16, height=16, focal_length=18.0),
    }
    meta["patterns"] = {}
    for name, p in patterns.items():
        fields = {f.name: getattr(p, f.name) for f in dataclasses.fields(p) if f.name != "func"}
        s = make_camera(cam, copy.copy(p), one)
        k32 = s._data.intrinsic_matrices[0].numpy().copy()
        d32 = s.ray_directions[0].numpy().copy()
        assert not bool(s.ray_starts.any())
        with default_dtype(torch.float64):
            _, d64 = pt.pinhole_camera_pattern(p, s._data.intrinsic_matrices.to(torch.float64), "cpu")
        arrays[f"{name}_intrinsics"] = k32
        put(f"{name}_dirs", d32, d64[0].numpy())
        meta["patterns"][name] = dict(fields, intrinsic_matrix=k2 if name == "p2" else None)

    # ---- o: the offset quaternion per convention
    rots = [np.array([1.0, 0.0, 0.0, 0.0], np.float32), tilted()]
    for conv in CONVENTIONS:
        for i, rot in enumerate(rots):
            s = make_camera(cam, copy.copy(patterns["p1"]), one, offset_rot=[float(x) for x in rot], convention=conv)
            with default_dtype(torch.float64):
                q64 = mt.convert_camera_frame_orientation_convention(
                    torch.from_numpy(rot.astype(np.float64))[None], origin=conv, target="world")
            put(f"o_{conv}_{i}", s._offset_quat[0].numpy().copy(), q64[0].numpy(), up_to_sign=True)
    meta["o_rots"] = [[float(x) for x in r] for r in rots]

    # ---- w: world poses and directions
    n = 24
    stones = grc.stone_walk(rng, n)
    pos, quat = grc.root_poses(rng, stones)
    xyzw = torch.from_numpy(np.concatenate([pos, quat[:, 1:], quat[:, :1]], 1))
    # pitched 0.45 rad down about the camera's y axis ("world" convention), handed over in "ros"
    pitch = torch.tensor([[math.cos(0.225), 0.0, math.sin(0.225), 0.0]])
    rot_ros = mt.convert_camera_frame_orientation_convention(pitch, origin="world", target="ros")[0]
    w_cfg = dict(offset_pos=(0.3, 0.02, 0.25), offset_rot=[float(x) for x in rot_ros], convention="ros")
    env_ids = list(range(n))

    def world(dtype, depth=None, clipping="none", max_distance=1e6):
        s = make_camera(cam, copy.copy(patterns["p0"]), xyzw, clipping=clipping, max_distance=max_distance, **w_cfg)
        local = (s.ray_directions[0].numpy().copy(), s._offset_pos.numpy().copy(), s._offset_quat.numpy().copy())
        promote(s, dtype)
        del mesh.calls[:]
        mesh.depth = depth
        with default_dtype(dtype):
            s._update_buffers_impl(env_ids)
        (starts, dirs), = mesh.calls
        assert dirs.dtype == dtype and bool((starts == s._data.pos_w.unsqueeze(1)).all())
        return s, local, dirs.numpy().copy()

    s32, local, dw32 = world(torch.float32)
    s64, _, dw64 = world(torch.float64)
    R = local[0].shape[0]
    arrays["w_root_pos"] = np.ascontiguousarray(pos.T)
    arrays["w_root_quat"] = np.ascontiguousarray(quat.T)
    arrays["w_stones"] = np.ascontiguousarray(stones.reshape(n, 3 * NUM_STONES).T)
    arrays["w_dirs"] = np.ascontiguousarray(local[0].T)
    arrays["w_offset"] = np.ascontiguousarray(np.concatenate([local[1], local[2]], 1).T)
    put("w_pos_w", s32._data.pos_w.numpy(), s64._data.pos_w.numpy())
    put("w_dirs_w", dw32, dw64)
    for k in ("quat_w_world", "quat_w_ros", "quat_w_opengl"):
        with default_dtype(torch.float64):
            q64 = getattr(s64._data, k).numpy().copy()
        put(f"w_{k}", getattr(s32._data, k).numpy().copy(), q64, up_to_sign=True)
    meta["w"] = dict(n=n, width=19, height=13, half=list(HALF), cfg=w_cfg)

    # ---- z: the post-processing on a supplied depth
    starts64 = np.broadcast_to(s64._data.pos_w.numpy()[:, None, :], dw64.shape)
    t64, surf, _ = rcc.oracle64(starts64, dw64, stones.astype(np.float64), HALF, rcc.GROUND | rcc.STONES, 1e6, 0.0)
    depth = np.where(surf == rcc.MISS, np.inf, t64).astype(np.float32)
    assert depth.shape == (n, R)
    miss, far, near = np.isinf(depth), np.isfinite(depth) & (depth > MAX_DISTANCE), depth <= MAX_DISTANCE
    assert miss.sum() > 50 and far.sum() > 50 and near.sum() > 50 and (surf >= 0).sum() > 50, \
        (miss.sum(), far.sum(), near.sum(), (surf >= 0).sum())
    arrays["z_depth"] = depth
    meta["z"] = dict(misses=int(miss.sum()), clipped=int(far.sum()), unclipped=int(near.sum()),
                     stone_hits=int((surf >= 0).sum()))
    for clip in ("none", "max", "zero"):
        a = world(torch.float32, depth, clip, MAX_DISTANCE)[0]._data.output
        b = world(torch.float64, depth, clip, MAX_DISTANCE)[0]._data.output
        for key, short in (("distance_to_image_plane", "plane"), ("distance_to_camera", "camera")):
            put(f"z_{clip}_{short}", a[key].numpy().reshape(n, R).copy(), b[key].numpy().reshape(n, R).copy())
        if clip == "none":
            assert np.array_equal(np.isnan(arrays["z_none_plane"]), miss)
    mesh.depth = None

    # ---- s: set_world_poses
    ids = [0, 3, 7, 8, 21]
    positions = (pos[ids] + rng.uniform(-0.5, 0.5, (len(ids), 3))).astype(np.float32)
    q = rng.normal(size=(len(ids), 4))
    orientations = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(np.float32)
    arrays["s_env_ids"] = np.asarray(ids, np.int64)
    arrays["s_positions"], arrays["s_orientations"] = positions, orientations
    for conv in ("ros", "world"):
        out = []
        for dtype in (torch.float32, torch.float64):
            s = make_camera(cam, copy.copy(patterns["p0"]), xyzw, **w_cfg)
            promote(s, dtype)
            with default_dtype(dtype):
                s.set_world_poses(torch.from_numpy(positions).to(dtype), torch.from_numpy(orientations).to(dtype),
                                  ids, convention=conv)
            out.append(np.concatenate([s._offset_pos.numpy(), s._offset_quat.numpy()], 1).T.copy())
        arrays[f"s_{conv}_offset"], arrays[f"s_{conv}_offset64"] = out
        meta["e_ref"][f"s_{conv}_offset_pos"] = e_ref(out[0][:3].T, out[1][:3].T)
        meta["e_ref"][f"s_{conv}_offset_quat"] = e_ref(out[0][3:].T, out[1][3:].T, up_to_sign=True)
    for k, v in meta["e_ref"].items():
        # (the unclipped depths of case z reach hundreds of metres towards the horizon: their noise scales with them)
        cap = 1e-5 if not k.startswith("z_none") else 1e-5 * float(depth[np.isfinite(depth)].max())
        assert 0.0 <= v < cap, (k, v)
    arrays["meta"] = np.array(json.dumps(meta))
    return arrays


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reference", default=os.environ.get("ALLSTEPS_REFERENCE"), help="root of a reference checkout")
    ap.add_argument("--check", action="store_true", help="compare with the committed file instead of writing it")
    a = ap.parse_args(argv)
    if not a.reference:
        ap.error("--reference DIR (or ALLSTEPS_REFERENCE) is needed")
    arrays = generate(a.reference)
    if a.check:
        have = dict(np.load(OUT)) if os.path.exists(OUT) else {}
        same = set(have) == set(arrays) and all(
            have[k].dtype == arrays[k].dtype and have[k].shape == arrays[k].shape
            and have[k].tobytes() == arrays[k].tobytes() for k in arrays)
        print(f"ray_camera.npz: {'identical' if same else 'DIFFERS'} ({len(arrays)} arrays)")
        return 0 if same else 1
    np.savez_compressed(OUT, **{k: arrays[k] for k in sorted(arrays)})
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes)")
    return 0


if __name__ == "__main__":
    sys.exit(main())
