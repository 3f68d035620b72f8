"""Generate tests/golden/frame_transformer.npz from the reference's own FrameTransformer sensor code.

Loads ``isaaclab/sensors/sensor_base.py``, ``isaaclab/sensors/frame_transformer/frame_transformer.py`` (with its
``frame_transformer_data.py``) and ``isaaclab/utils/math.py`` of a reference checkout BY PATH, with stub modules of
this file's own for the Isaac / Omniverse packages they import.  The fakes: a stage, a list of prim paths that
``sim_utils.find_matching_prims`` matches segment by segment as regular expressions (prims with
``GetPath().pathString`` and ``HasAPI``); a simulation context (device, backend, physics dt); and a PhysX simulation
view whose ``create_rigid_body_view(patterns)`` lists its ``prim_paths`` pattern-major (every env of the first
pattern, then of the second, ...) and whose ``get_transforms`` returns the recorded poses in that order with
quaternions in (x, y, z, w) order, as PhysX does.  A ``FrameTransformer`` is built with ``object.__new__``; the
reference's real ``_initialize_impl`` (through it ``SensorBase._initialize_impl``) resolves the frames and makes the
buffers, every update is the real ``update(dt)``, every read the real ``.data`` (through it
``_update_outdated_buffers`` and ``_update_buffers_impl``), every reset the real ``reset(env_ids)``.

All arrays are env-minor, the layout of the device buffers.  Per motion M and case X:
  M_pose     (U, B, 7, n) float32    the link poses of the motion's bodies per update: pos 3 | quat 4 (w, x, y, z)
  X_source64 (K, 7, n) float64       source_pos_w 3 | source_quat_w 4 after the records ``stored`` of the case, from
  X_target64 (K, 14, F, n) float64   the run on float64 tensors (the same float32 inputs and offsets, promoted):
                                     target_pos_w 3 | target_quat_w 4 | target_pos_source 3 | target_quat_source 4
and in ``cases`` (json): n, the motion and its ``bodies`` (the names of M_pose's axis B; ``step_<i>`` are stones),
``robot_bodies`` (the stage's robot body list) and ``num_steps``, the cfg (prim_path, source_frame_offset,
target_frames with prim_path / name / offset, offsets as float32 values), the reference's ``target_frame_names`` and
its two switches, ``stored`` and e_ref, per output field max |float32 run - float64 run| over ALL records.  One frame
per body in every case: where several frames sit on one body the reference's order is a Python set's.

  a   n = 67, 24 updates, read after every update; walker body list; source torso, targets ``.*_foot``; no offsets
      (both switches off)
  b   the same motion; a tilted, unnormalised source offset; left_foot with an offset (named toe), right_foot without
      (the target switch on: the identity offset is applied too)
  c   n = 3: source torso, targets ``.*`` (so the source is also a target) and the stones ``step_.*`` of num_steps =
      12 (step_10 comes before step_2); no offsets; a masked reset and a second read in the last update

    python tests/golden/gen_frame_transformer.py --reference DIR [--check]

--check regenerates into memory and compares with the committed file array by array, bit for bit.
"""

from __future__ import annotations

import argparse
import importlib.util
import json
import os
import re
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "frame_transformer.npz")
PKG = os.path.join("source", "isaaclab", "isaaclab")
SOURCE_FIELDS = (("source_pos_w", 0, 3), ("source_quat_w", 3, 7))
TARGET_FIELDS = (("target_pos_w", 0, 3), ("target_quat_w", 3, 7), ("target_pos_source", 7, 10),
                 ("target_quat_source", 10, 14))
DT = 1 / 240
WALKER = ["walker3d", "head", "torso", "waist", "pelvis", "right_thigh", "right_shin", "right_foot", "left_thigh",
          "left_shin", "left_foot", "right_upper_arm", "right_lower_arm", "right_hand", "left_upper_arm",
          "left_lower_arm", "left_hand"]
NS = "/World/envs/env_.*"


class _Any:
    def __init__(self, *a, **k):
        pass

    def __getattr__(self, name):
        return _Any()

    def __call__(self, *a, **k):
        return _Any()


def _mod(name: str, **attrs) -> types.ModuleType:
    m = types.ModuleType(name)
    m.__path__ = []
    for k, v in attrs.items():
        setattr(m, k, v)
    sys.modules[name] = m
    parent, _, leaf = name.rpartition(".")
    if parent in sys.modules:
        setattr(sys.modules[parent], leaf, m)
    return m


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


# ------------------------------------------------------------------------------------------------ the fakes
class _Prim:
    def __init__(self, path: str, rigid: bool):
        self._path, self._rigid = path, rigid

    def GetPath(self):
        return types.SimpleNamespace(pathString=self._path)

    def HasAPI(self, api):
        return self._rigid


class _World:
    """The stage, the simulation context and the PhysX views of one run."""

    def __init__(self, n: int, robot_bodies: list, num_steps: int, dtype):
        self.n, self.dtype = n, dtype
        self.prims = []
        for e in range(n):
            env = f"/World/envs/env_{e}"
            self.prims += [_Prim(env, False), _Prim(f"{env}/Robot", False)]
            self.prims += [_Prim(f"{env}/Robot/{b}", True) for b in robot_bodies]
            self.prims += [_Prim(f"{env}/step_{i}", True) for i in range(num_steps)]
        self.pose = {}  # body name -> (7, n) float32 of the current update
        self.device, self.backend = "cpu", "torch"

    # sim_utils
    def instance(self):
        return self

    def get_physics_dt(self):
        return DT

    def find_matching_prims(self, expr: str) -> list:
        parts = expr.split("/")
        return [p for p in self.prims if len(p._path.split("/")) == len(parts)
                and all(re.fullmatch(a, b) is not None for a, b in zip(parts, p._path.split("/")))]

    # physx
    def create_simulation_view(self, backend):
        assert backend == self.backend
        return self

    def set_subspace_roots(self, root):
        assert root == "/"

    def create_rigid_body_view(self, patterns: list):
        return _BodyView(self, patterns)


class _BodyView:
    def __init__(self, world: _World, patterns: list):
        self._w = world
        self._names = [p.rsplit("/", 1)[-1] for p in patterns]
        for p in patterns:
            assert "/env_*/" in p, p
        # pattern-major: every env of a pattern before the next pattern
        self.prim_paths = [p.replace("env_*", f"env_{e}") for p in patterns for e in range(world.n)]

    def get_transforms(self):
        rows = [torch.from_numpy(self._w.pose[b].T.copy()) for b in self._names]  # each (n, 7), (w, x, y, z)
        t = torch.cat(rows).to(self._w.dtype)
        return torch.cat([t[:, :3], t[:, 4:7], t[:, 3:4]], 1)  # PhysX: (x, y, z, w)


def load_reference(root: str):
    """The reference's frame_transformer module at ``root``, over its real sensor_base, data class and utils.math."""
    pkg = os.path.join(root, PKG)
    for name in ("omni", "omni.kit", "omni.physics", "omni.physics.tensors", "omni.physics.tensors.impl", "isaacsim",
                 "isaacsim.core", "isaacsim.core.utils", "isaaclab", "isaaclab.utils", "isaaclab.sensors",
                 "isaaclab.sensors.frame_transformer"):
        _mod(name)
    _mod("omni.kit.app")
    _mod("omni.timeline")
    _mod("omni.log", verbose=lambda *a, **k: None, info=lambda *a, **k: None, warn=lambda *a, **k: None)
    _mod("omni.physics.tensors.impl.api")
    _mod("isaacsim.core.utils.stage")
    _mod("pxr", UsdPhysics=_Any())
    _mod("isaaclab.sim")
    _mod("isaaclab.markers", VisualizationMarkers=_Any)
    sub = os.path.join(pkg, "sensors", "frame_transformer")
    _load("isaaclab.utils.math", os.path.join(pkg, "utils", "math.py"), "isaaclab.utils")
    _load("isaaclab.sensors.sensor_base", os.path.join(pkg, "sensors", "sensor_base.py"), "isaaclab.sensors")
    _load("isaaclab.sensors.frame_transformer.frame_transformer_data", os.path.join(sub, "frame_transformer_data.py"),
          "isaaclab.sensors.frame_transformer")
    return _load("isaaclab.sensors.frame_transformer.frame_transformer", os.path.join(sub, "frame_transformer.py"),
                 "isaaclab.sensors.frame_transformer")


def make_sensor(ft, world: _World, cfg: dict):
    sim = sys.modules["isaaclab.sim"]
    sim.SimulationContext = types.SimpleNamespace(instance=world.instance)
    sim.find_matching_prims = world.find_matching_prims
    api = sys.modules["omni.physics.tensors.impl.api"]
    api.create_simulation_view = world.create_simulation_view
    ns = types.SimpleNamespace
    s = object.__new__(ft.FrameTransformer)
    s._initialize_handle = s._invalidate_initialize_handle = s._debug_vis_handle = None  # SensorBase.__del__
    s.cfg = ns(update_period=0.0, history_length=0, debug_vis=False, prim_path=cfg["prim_path"],
               source_frame_offset=ns(pos=tuple(cfg["source_frame_offset"]["pos"]),
                                      rot=tuple(cfg["source_frame_offset"]["rot"])),
               target_frames=[ns(prim_path=t["prim_path"], name=t["name"],
                                 offset=ns(pos=tuple(t["offset"]["pos"]), rot=tuple(t["offset"]["rot"])))
                              for t in cfg["target_frames"]])
    s._is_visualizing = False
    s._data = sys.modules["isaaclab.sensors.frame_transformer.frame_transformer_data"].FrameTransformerData()
    s._initialize_impl()  # the real one, SensorBase's included
    assert s._num_envs == world.n
    if world.dtype != torch.float32:  # the float64 run: the same float32 offsets and zeros, promoted
        for k in ("source_pos_w", "source_quat_w", "target_pos_w", "target_quat_w", "target_pos_source",
                  "target_quat_source"):
            setattr(s._data, k, getattr(s._data, k).to(world.dtype))
        for k in ("_source_frame_offset_pos", "_source_frame_offset_quat", "_target_frame_offset_pos",
                  "_target_frame_offset_quat"):
            if hasattr(s, k):
                setattr(s, k, getattr(s, k).to(world.dtype))
    return s


def _rows(s):
    d = s._data
    source = np.concatenate([d.source_pos_w.numpy().T, d.source_quat_w.numpy().T]).copy()  # (7, n)
    target = np.concatenate([getattr(d, k).numpy().transpose(2, 1, 0) for k, _, _ in TARGET_FIELDS]).copy()  # (14, F, n)
    return source, target


def run_reference(ft, pose, bodies, robot_bodies, num_steps, cfg, resets, dtype):
    """The reference over pose (U, B, 7, n); returns (upd, names, switches, source, target) per record."""
    updates, _, _, n = pose.shape
    world = _World(n, robot_bodies, num_steps, dtype)
    s = make_sensor(ft, world, cfg)
    zero_s, zero_t = _rows(s)
    assert not zero_s.any() and not zero_t.any()  # the buffers hold zeros before the first update
    upd, source, target = [], [], []

    def record(u):
        s.data  # the read: recomputes the outdated envs
        assert not bool(s._is_outdated.any())
        a, b = _rows(s)
        upd.append(u)
        source.append(a)
        target.append(b)

    for u in range(updates):
        world.pose = {b: pose[u, i] for i, b in enumerate(bodies)}
        s.update(DT)
        record(u)
        if u in resets:
            s.reset(resets[u])
            assert int(s._is_outdated.sum()) == len(resets[u])
            record(u)
    switches = (bool(s._apply_source_frame_offset), bool(s._apply_target_frame_offset))
    return np.array(upd, np.int32), list(s._data.target_frame_names), switches, np.stack(source), np.stack(target)


def motion(rng, updates: int, n: int, bodies: list):
    """Smooth random link poses, float32 (U, B, 7, n): any orientation per body; a stone keeps (1, 0, 0, 0)."""
    t = np.arange(updates)[:, None] * DT * 4  # (U, 1)
    out = np.zeros((updates, len(bodies), 7, n))

    def wave(scale, rows):
        f = rng.uniform(0.5, 6.0, (rows, 1, n))
        ph = rng.uniform(0, 2 * np.pi, (rows, 1, n))
        a = rng.uniform(0.3, 1.0, (rows, 1, n)) * scale
        return (a * np.sin(2 * np.pi * f * t[None] + ph)).transpose(1, 0, 2)  # (U, rows, n)

    for i, b in enumerate(bodies):
        out[:, i, :3] = wave(0.5, 3) + rng.uniform(-2, 2, (1, 3, n)) + np.array([0.0, 0.0, 1.0])[None, :, None]
        if b.startswith("step_"):
            out[:, i, 3] = 1.0
        else:
            q = wave(1.0, 4) + rng.normal(0, 1, (1, 4, n))
            out[:, i, 3:] = q / np.linalg.norm(q, axis=1, keepdims=True)
    return out.astype(np.float32)


def f32(values) -> list:
    return [float(np.float32(x)) for x in values]


def offset(pos=(0, 0, 0), rot=(1, 0, 0, 0)) -> dict:
    return {"pos": f32(pos), "rot": f32(rot)}


def run_case(ft, arrays, cases, name, motion_name, pose, bodies, robot_bodies, num_steps, cfg, resets=None, stored=None):
    resets = resets or {}
    upd, names, sw, source, target = run_reference(ft, pose, bodies, robot_bodies, num_steps, cfg, resets,
                                                   torch.float32)
    upd64, names64, sw64, source64, target64 = run_reference(ft, pose, bodies, robot_bodies, num_steps, cfg, resets,
                                                             torch.float64)
    assert source.dtype == np.float32 and target.dtype == np.float32
    assert source64.dtype == np.float64 and target64.dtype == np.float64
    assert np.array_equal(upd, upd64) and names == names64 and sw == sw64
    e_ref = {k: float(np.abs(source[:, lo:hi] - source64[:, lo:hi]).max()) for k, lo, hi in SOURCE_FIELDS}
    e_ref.update({k: float(np.abs(target[:, lo:hi] - target64[:, lo:hi]).max()) for k, lo, hi in TARGET_FIELDS})
    stored = list(range(len(upd))) if stored is None else stored
    arrays.update({f"{name}_source64": source64[stored], f"{name}_target64": target64[stored]})
    cases.append({"name": name, "n": int(pose.shape[3]), "updates": int(pose.shape[0]), "records": int(len(upd)),
                  "upd": upd.tolist(), "motion": motion_name, "bodies": bodies, "robot_bodies": robot_bodies,
                  "num_steps": num_steps, "cfg": cfg, "target_frame_names": names, "apply_source_offset": sw[0],
                  "apply_target_offset": sw[1], "stored": stored, "e_ref": e_ref})
    return names, sw, source, target


def generate(reference: str) -> dict:
    ft = load_reference(reference)
    rng = np.random.default_rng(20261020)
    arrays: dict[str, np.ndarray] = {}
    cases: list = []

    # ---- a: torso -> .*_foot, no offsets
    n, updates = 67, 24
    bodies = ["torso", "left_foot", "right_foot"]
    pose = motion(rng, updates, n, bodies)
    arrays["m_pose"] = pose
    stored = [0, 1, 2] + list(range(5, updates, 6))
    cfg_a = {"prim_path": f"{NS}/Robot/torso", "source_frame_offset": offset(),
             "target_frames": [{"prim_path": f"{NS}/Robot/.*_foot", "name": None, "offset": offset()}]}
    names, sw, source, target = run_case(ft, arrays, cases, "a", "m", pose, bodies, WALKER, 0, cfg_a, stored=stored)
    assert names == ["left_foot", "right_foot"] and sw == (False, False)
    assert np.array_equal(source, pose[:, 0]) and np.array_equal(target[:, :7, 0], pose[:, 1])

    # ---- b: the same motion; a tilted, unnormalised source offset; one target with an offset, one without
    rot = (0.8, 0.3, -0.4, 0.2)  # |rot| != 1: used as given
    cfg_b = {"prim_path": f"{NS}/Robot/torso", "source_frame_offset": offset((0.05, -0.02, 0.1), rot),
             "target_frames": [{"prim_path": f"{NS}/Robot/right_foot", "name": None, "offset": offset()},
                               {"prim_path": f"{NS}/Robot/left_foot", "name": "toe",
                                "offset": offset((0.12, 0.0, -0.03), (0.9, -0.1, 0.3, 0.2))}]}
    names, sw, source, target = run_case(ft, arrays, cases, "b", "m", pose, bodies, WALKER, 0, cfg_b, stored=stored)
    assert names == ["toe", "right_foot"] and sw == (True, True)  # left_foot sorts first, whatever the cfg's order

    # ---- c: n = 3, the source is also a target, stones
    n, updates, num_steps = 3, 4, 12
    bodies = WALKER + [f"step_{i}" for i in range(num_steps)]
    pose = motion(rng, updates, n, bodies)
    arrays["c_pose"] = pose
    cfg_c = {"prim_path": f"{NS}/Robot/torso", "source_frame_offset": offset(),
             "target_frames": [{"prim_path": f"{NS}/step_.*", "name": None, "offset": offset()},
                               {"prim_path": f"{NS}/Robot/.*", "name": None, "offset": offset()}]}
    names, sw, source, target = run_case(ft, arrays, cases, "c", "c", pose, bodies, WALKER, num_steps, cfg_c,
                                         resets={3: [1]})
    assert sw == (False, False) and names == sorted(WALKER) + sorted(f"step_{i}" for i in range(num_steps))
    assert names.index("step_10") < names.index("step_2") and "torso" in names
    k = names.index("torso")  # the source as a target: its own pose
    assert np.array_equal(target[:, 0:7, k], source)
    assert np.array_equal(target[-1], target[-2])  # the masked reset recomputed the same state

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
        print(f"frame_transformer.npz: {'identical' if same else 'DIFFERS'} ({len(arrays)} arrays)")
        return 0 if same else 1
    np.savez_compressed(OUT, **{k: arrays[k] for k in sorted(arrays)})
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes)")
    for c in json.loads(str(arrays["cases"])):
        print(c["name"], c["records"], "records,", c["target_frame_names"], "e_ref",
              {k: f"{v:.2e}" for k, v in c["e_ref"].items()})
    return 0


if __name__ == "__main__":
    sys.exit(main())
