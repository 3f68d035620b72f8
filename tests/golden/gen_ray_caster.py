"""Generate tests/golden/ray_caster.npz from the reference's own ray-caster code.

Loads ``isaaclab/sensors/ray_caster/patterns/patterns.py``, ``isaaclab/utils/math.py``, ``isaaclab/sensors/
sensor_base.py`` and ``isaaclab/sensors/ray_caster/ray_caster.py`` (with its ``ray_caster_data.py``) of a reference
checkout BY PATH, with stub modules of this file's own for the Isaac / Omniverse / warp packages they import.  A
``RayCaster`` is built with ``object.__new__``; its view is a fake ``ArticulationView`` that returns recorded root
poses.  The rays are the reference's real ``_initialize_rays_impl`` (pattern, offset) and ``_update_buffers_impl``
(yaw-only or full attachment); ``raycast_mesh`` -- the warp mesh query, which is not what the fixture is about and
is not installed -- is replaced by a recorder of the world rays it is handed.

Every case holds (n envs, R rays; arrays named ``<case>_<name>``):
  rays_local   (6, R) float32   local start xyz | direction xyz after the cfg's offset (ray_starts[0], ray_directions[0])
  root_pos     (3, n), root_quat (4, n) float32 (w, x, y, z), stones (60, n) float32: the device layout
  starts_w, dirs_w        (n, R, 3) float32   the world rays the reference hands to raycast_mesh
  starts_w64, dirs_w64    (n, R, 3) float64   the same code on the same float32 inputs promoted to float64
and in ``cases`` (JSON) the cfg, ``half`` (the stones' half extents) and ``e_ref``, the largest absolute difference
between the float32 and the float64 world rays: the reference's own float32 noise on these inputs.

  y   the velocity task's height scanner (velocity_env_cfg.py:66-73): offset z = 20, attach_yaw_only, grid 0.1 over
      1.6 x 1.0 (187 rays); 24 envs whose roots sit 0.5-1.3 m above one of the first ten stones of a task-like
      walk, yaw over the full circle, tilts up to 0.6 rad
  f   attach_yaw_only = False, grid 0.1 over 0.8 x 0.6 (63 rays), offset pos (0.1, 0, 0.3) and a tilted rot
  d   y with direction (0.3, 0, -1) and ordering "yx"

    python tests/golden/gen_ray_caster.py --reference DIR [--check]

--check regenerates into memory and compares with the committed file array by array, bit for bit.
"""

from __future__ import annotations

import argparse
import importlib.util
import json
import math
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from refload import _Any, _mod  # noqa: E402

OUT = os.path.join(HERE, "ray_caster.npz")
PKG = os.path.join("source", "isaaclab", "isaaclab")
HALF = (0.25, 0.4, 0.1125)  # half of step_size (0.5, 0.8, 0.225)
NUM_STONES = 20


def _load(name: str, path: str, package: str):
    spec = importlib.util.spec_from_file_location(name, path)
    m = importlib.util.module_from_spec(spec)
    m.__package__ = package
    sys.modules[name] = m
    parent, _, leaf = name.rpartition(".")
    if parent in sys.modules:
        setattr(sys.modules[parent], leaf, m)
    spec.loader.exec_module(m)
    return m


class ArticulationView:
    """Stands in for physx.ArticulationView: recorded root transforms (n, 7), position | quaternion (x, y, z, w)."""

    def __init__(self, transforms: torch.Tensor):
        self.transforms = transforms
        self.count = len(transforms)

    def get_root_transforms(self):
        return self.transforms


class _Recorder:
    """Stands in for isaaclab.utils.warp.raycast_mesh: keeps the world rays, returns no hits."""

    def __init__(self):
        self.calls = []

    def __call__(self, ray_starts, ray_directions, max_dist=1e6, mesh=None, **kw):
        self.calls.append((ray_starts.clone(), ray_directions.clone()))
        return torch.full_like(ray_starts, float("inf")), None, None, None


def load_reference(root: str):
    """(patterns module, math module, ray_caster module, recorder) of the reference at ``root``."""
    pkg = os.path.join(root, PKG)
    for name in ("omni", "omni.kit", "omni.physics", "omni.physics.tensors", "omni.physics.tensors.impl", "isaaclab",
                 "isaaclab.utils", "isaaclab.sensors", "isaaclab.sensors.ray_caster", "isaaclab.sensors.ray_caster.patterns",
                 "isaaclab.terrains", "isaaclab.terrains.trimesh", "isaacsim", "isaacsim.core"):
        _mod(name)
    for name, leaf in (("omni", "kit"), ("omni", "physics"), ("omni.physics", "tensors"),
                       ("omni.physics.tensors", "impl")):
        setattr(sys.modules[name], leaf, sys.modules[f"{name}.{leaf}"])
    sys.modules["omni.kit"].app = _mod("omni.kit.app")
    sys.modules["omni"].timeline = _mod("omni.timeline")
    sys.modules["omni"].log = _mod("omni.log", warn=_Any(), info=_Any())
    api = _mod("omni.physics.tensors.impl.api", ArticulationView=ArticulationView,
               RigidBodyView=type("RigidBodyView", (), {}))
    sys.modules["omni.physics.tensors.impl"].api = api
    _mod("warp", Mesh=_Any)
    _mod("isaacsim.core.prims", XFormPrim=type("XFormPrim", (), {}))
    _mod("pxr", UsdGeom=_Any(), UsdPhysics=_Any(), PhysxSchema=_Any())
    sys.modules["isaaclab"].sim = _mod("isaaclab.sim")
    _mod("isaaclab.markers", VisualizationMarkers=_Any)
    _mod("isaaclab.terrains.trimesh.utils", make_plane=_Any())
    rec = _Recorder()
    _mod("isaaclab.utils.warp", convert_to_warp_mesh=_Any(), raycast_mesh=rec)
    mt = _load("isaaclab.utils.math", os.path.join(pkg, "utils", "math.py"), "isaaclab.utils")
    pt = _load("isaaclab.sensors.ray_caster.patterns.patterns",
               os.path.join(pkg, "sensors", "ray_caster", "patterns", "patterns.py"),
               "isaaclab.sensors.ray_caster.patterns")
    _load("isaaclab.sensors.sensor_base", os.path.join(pkg, "sensors", "sensor_base.py"), "isaaclab.sensors")
    _load("isaaclab.sensors.ray_caster.ray_caster_data",
          os.path.join(pkg, "sensors", "ray_caster", "ray_caster_data.py"), "isaaclab.sensors.ray_caster")
    rc = _load("isaaclab.sensors.ray_caster.ray_caster", os.path.join(pkg, "sensors", "ray_caster", "ray_caster.py"),
               "isaaclab.sensors.ray_caster")
    return pt, mt, rc, rec


def make_sensor(rc, pt, cfg: dict, transforms: torch.Tensor):
    s = object.__new__(rc.RayCaster)
    s._initialize_handle = s._invalidate_initialize_handle = s._debug_vis_handle = None  # SensorBase.__del__
    pattern = types.SimpleNamespace(func=pt.grid_pattern, resolution=cfg["resolution"], size=cfg["size"],
                                    direction=tuple(cfg["direction"]), ordering=cfg["ordering"])
    s.cfg = types.SimpleNamespace(prim_path=cfg["prim_path"], mesh_prim_paths=cfg["mesh_prim_paths"],
                                  offset=types.SimpleNamespace(pos=tuple(cfg["offset_pos"]), rot=tuple(cfg["offset_rot"])),
                                  attach_yaw_only=cfg["attach_yaw_only"], pattern_cfg=pattern,
                                  max_distance=cfg["max_distance"], drift_range=(0.0, 0.0), update_period=0.0,
                                  history_length=0, debug_vis=False)
    s._is_visualizing = False
    s._device = "cpu"
    s._view = ArticulationView(transforms)
    s._data = sys.modules["isaaclab.sensors.ray_caster.ray_caster_data"].RayCasterData()
    s.meshes = {cfg["mesh_prim_paths"][0]: None}
    return s


def world_rays(rc, pt, rec, cfg: dict, pos: np.ndarray, quat: np.ndarray):
    """The reference on root poses pos (n, 3), quat (n, 4) (w, x, y, z), float32: local rays (6, R), and the world
    rays in float32 and in float64 (the float32 local rays and poses promoted)."""
    xyzw = np.concatenate([pos, quat[:, 1:], quat[:, :1]], 1)
    out = []
    local = None
    for dtype in (torch.float32, torch.float64):
        s = make_sensor(rc, pt, cfg, torch.from_numpy(xyzw).to(dtype))
        s._initialize_rays_impl()  # float32: the pattern and the offset as the reference forms them
        if local is None:
            local = np.concatenate([s.ray_starts[0].numpy().T, s.ray_directions[0].numpy().T]).astype(np.float32)
        s.ray_starts, s.ray_directions = s.ray_starts.to(dtype), s.ray_directions.to(dtype)
        s.drift = s.drift.to(dtype)
        for k in ("pos_w", "quat_w", "ray_hits_w"):
            setattr(s._data, k, getattr(s._data, k).to(dtype))
        del rec.calls[:]
        s._update_buffers_impl(list(range(len(pos))))
        (starts, dirs), = rec.calls
        assert starts.dtype == dtype and dirs.dtype == dtype
        assert np.array_equal(s._data.pos_w.numpy(), pos) and np.array_equal(s._data.quat_w.numpy(), quat)
        out += [starts.numpy().copy(), dirs.numpy().copy()]
    return (local, *out)


def stone_walk(rng, n: int) -> np.ndarray:
    """(n, 20, 3) stone centres of a task-like walk at a low curriculum level: 0.65-0.9 m apart along a heading that
    starts within 0.05 rad of +x and turns by at most 0.05 rad a stone, the feet's sides alternating, heights
    drifting within [0.05, 0.5].  (Nearly straight on purpose: the slanted rays of case d come down about 6 m
    ahead of the root in +x, and should still find the walk's later stones there.)"""
    c = np.zeros((n, NUM_STONES, 3))
    for e in range(n):
        heading = rng.uniform(-0.05, 0.05)
        p = np.array([0.0, 0.0, rng.uniform(0.1, 0.3)])
        for k in range(NUM_STONES):
            if k:
                heading += rng.uniform(-0.05, 0.05)
                dr = rng.uniform(0.65, 0.9)
                p = p + np.array([dr * math.cos(heading), dr * math.sin(heading), rng.uniform(-0.08, 0.08)])
                p[2] = min(max(p[2], 0.05), 0.5)
            side = 0.13 if k % 2 else -0.13
            c[e, k] = p + np.array([-side * math.sin(heading), side * math.cos(heading), 0.0])
    return c.astype(np.float32)


def root_poses(rng, stones: np.ndarray):
    """Roots 0.5-1.3 m above one of each env's first ten stones; yaw over the circle, tilt up to 0.6 rad."""
    n = len(stones)
    k = rng.integers(0, 10, n)
    pos = stones[np.arange(n), k].astype(np.float64)
    pos += np.stack([rng.uniform(-0.2, 0.2, n), rng.uniform(-0.2, 0.2, n), rng.uniform(0.5, 1.3, n)], 1)
    yaw, tilt, axis = rng.uniform(-math.pi, math.pi, n), rng.uniform(0.0, 0.6, n), rng.uniform(-math.pi, math.pi, n)
    qy = np.stack([np.cos(yaw / 2), np.zeros(n), np.zeros(n), np.sin(yaw / 2)], 1)
    qt = np.stack([np.cos(tilt / 2), np.sin(tilt / 2) * np.cos(axis), np.sin(tilt / 2) * np.sin(axis), np.zeros(n)], 1)
    w1, v1, w2, v2 = qy[:, :1], qy[:, 1:], qt[:, :1], qt[:, 1:]
    q = np.concatenate([w1 * w2 - (v1 * v2).sum(1, keepdims=True), w1 * v2 + w2 * v1 + np.cross(v1, v2)], 1)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    return pos.astype(np.float32), q.astype(np.float32)


def generate(reference: str) -> dict:
    pt, mt, rc, rec = load_reference(reference)
    rng = np.random.default_rng(20261021)
    n = 24
    base = dict(prim_path="/World/envs/env_.*/Robot/base", mesh_prim_paths=["/World/ground"], max_distance=1e6,
                offset_rot=[1.0, 0.0, 0.0, 0.0], direction=[0.0, 0.0, -1.0], ordering="xy")
    cfgs = {
        "y": dict(base, offset_pos=[0.0, 0.0, 20.0], attach_yaw_only=True, resolution=0.1, size=[1.6, 1.0]),
        "f": dict(base, offset_pos=[0.1, 0.0, 0.3], offset_rot=[math.cos(0.1), 0.0, math.sin(0.1), 0.0],
                  attach_yaw_only=False, resolution=0.1, size=[0.8, 0.6]),
    }
    cfgs["d"] = dict(cfgs["y"], direction=[0.3, 0.0, -1.0], ordering="yx")
    arrays: dict[str, np.ndarray] = {}
    cases = []
    scenes = {}
    for name in ("y", "f", "d"):
        if name == "d":
            stones, pos, quat = scenes["y"]  # "case y with ..."
        else:
            stones = stone_walk(rng, n)
            pos, quat = root_poses(rng, stones)
        scenes[name] = (stones, pos, quat)
        cfg = cfgs[name]
        local, s32, d32, s64, d64 = world_rays(rc, pt, rec, cfg, pos, quat)
        e_ref = float(max(np.abs(s32.astype(np.float64) - s64).max(), np.abs(d32.astype(np.float64) - d64).max()))
        assert 0.0 < e_ref < 1e-5, (name, e_ref)
        arrays[f"{name}_rays_local"] = local
        arrays[f"{name}_root_pos"] = np.ascontiguousarray(pos.T)
        arrays[f"{name}_root_quat"] = np.ascontiguousarray(quat.T)
        arrays[f"{name}_stones"] = np.ascontiguousarray(stones.reshape(n, 3 * NUM_STONES).T)
        arrays[f"{name}_starts_w"], arrays[f"{name}_dirs_w"] = s32, d32
        arrays[f"{name}_starts_w64"], arrays[f"{name}_dirs_w64"] = s64, d64
        cases.append({"name": name, "n": n, "num_rays": int(local.shape[1]), "cfg": cfg, "half": list(HALF),
                      "ground_z": 0.0, "e_ref": e_ref})
    assert [c["num_rays"] for c in cases] == [187, 63, 187]
    arrays["cases"] = np.array(json.dumps(cases))
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
        print(f"ray_caster.npz: {'identical' if same else 'DIFFERS'} ({len(arrays)} arrays)")
        return 0 if same else 1
    np.savez_compressed(OUT, **{k: arrays[k] for k in sorted(arrays)})
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes)")
    return 0


if __name__ == "__main__":
    sys.exit(main())
