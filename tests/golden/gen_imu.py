"""Generate tests/golden/imu.npz from the reference's own IMU sensor code.

Loads ``isaaclab/sensors/sensor_base.py``, ``isaaclab/sensors/imu/imu.py`` (with its ``imu_data.py``) and
``isaaclab/utils/math.py`` of a reference checkout BY PATH, with stub modules of this file's own for the Isaac /
Omniverse packages they import.  An ``Imu`` is built with ``object.__new__``; its buffers are made by the real
``_initialize_buffers_impl`` over a fake rigid-body view whose ``get_transforms`` returns the recorded poses with
quaternions in (x, y, z, w) order, as PhysX does, and whose ``get_velocities`` and ``get_coms`` return fresh clones
(the reference adds into what it is handed).  Every sensor update is the reference's real ``Imu.update(dt)`` (through
it ``SensorBase.update``: the timestamp and the outdated test), every read the real ``.data`` (through it
``_update_outdated_buffers`` and ``_update_buffers_impl``), every reset the real ``Imu.reset(env_ids)``.

All arrays are env-minor, the layout of the device buffers.  Per case X:
  X_pose   (U, 7, n) float32   the body's link pose per update: pos 3 | quat 4 (w, x, y, z)
  X_vel    (U, 6, n) float32   its centre-of-mass linear | angular velocity
  X_upd    (R,) int32          per record (a read of .data): the update whose pose and velocities it saw
  X_mask   (R, n) uint8        the envs that were outdated at that read -- the ones it recomputed
  X_data64 (K, 19, n) float64  pos_w 3 | quat_w 4 | lin_vel_b 3 | ang_vel_b 3 | lin_acc_b 3 | ang_acc_b 3 after the
                               records ``stored`` of the case, from the run on float64 tensors (the same float32
                               inputs and constants, promoted)
and in ``cases`` (json): n, dt, the constants offset_pos, offset_rot, com, gravity_bias as float32 values, ``stored``
and e_ref, per output field max |float32 run - float64 run| over ALL records.  The float64 run divides by
float64(float32(dt)), the divisor the float32 run rounds dt to, so that e_ref is the float32 run's rounding error
alone.  To stay a small file the fixture keeps the float64 outputs only (case a: the first three records and every
sixth after; b, c: all; b reads case a's pose and vel); ``--full PATH`` also writes every record of both runs, data
and prev, to PATH for a look by hand.

  a   n = 67, 48 updates, read after every update; smooth random poses and velocities (tilt up to 0.6 rad, |w| up to
      6 rad/s); identity offset, default bias, c != 0
  b   the same motion; offset pos (0.1, -0.05, 0.2), a rotated non-axis offset quaternion, bias (0, 0, 0); read only
      after every fourth update; some envs reset after that read and then read again
  c   n = 3: reads after masked resets in an update that was already read; the untouched envs keep their buffers

    python tests/golden/gen_imu.py --reference DIR [--check]

--check regenerates into memory and compares with the committed file array by array, bit for bit.
"""

from __future__ import annotations

import argparse
import importlib.util
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "imu.npz")
PKG = os.path.join("source", "isaaclab", "isaaclab")
FIELDS = (("pos_w", 0, 3), ("quat_w", 3, 7), ("lin_vel_b", 7, 10), ("ang_vel_b", 10, 13), ("lin_acc_b", 13, 16),
          ("ang_acc_b", 16, 19))
DT = 1 / 240


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


def load_reference(root: str):
    """The reference's imu module at ``root``, over its real sensor_base, imu_data and utils.math."""
    pkg = os.path.join(root, PKG)
    for name in ("omni", "omni.kit", "omni.physics", "omni.physics.tensors", "omni.physics.tensors.impl", "isaacsim",
                 "isaacsim.core", "isaacsim.core.utils", "isaaclab", "isaaclab.utils", "isaaclab.sensors",
                 "isaaclab.sensors.imu"):
        _mod(name)
    _mod("omni.kit.app")
    _mod("omni.timeline")
    _mod("omni.physics.tensors.impl.api")
    _mod("isaacsim.core.utils.stage")
    _mod("pxr", UsdPhysics=_Any())
    _mod("isaaclab.sim")
    _mod("isaaclab.markers", VisualizationMarkers=_Any)
    _load("isaaclab.utils.math", os.path.join(pkg, "utils", "math.py"), "isaaclab.utils")
    _load("isaaclab.sensors.sensor_base", os.path.join(pkg, "sensors", "sensor_base.py"), "isaaclab.sensors")
    _load("isaaclab.sensors.imu.imu_data", os.path.join(pkg, "sensors", "imu", "imu_data.py"), "isaaclab.sensors.imu")
    return _load("isaaclab.sensors.imu.imu", os.path.join(pkg, "sensors", "imu", "imu.py"), "isaaclab.sensors.imu")


class _BodyView:
    """Stands in for the PhysX RigidBodyView: the recorded pose and velocities of the current update."""

    def __init__(self, n: int, com: torch.Tensor):
        self.count = n
        self.transforms = self.velocities = None
        self.coms = torch.cat([com.repeat(n, 1), torch.zeros(n, 3, dtype=com.dtype), torch.ones(n, 1, dtype=com.dtype)],
                              1)

    def get_transforms(self):
        return self.transforms.clone()

    def get_velocities(self):
        return self.velocities.clone()

    def get_coms(self):
        return self.coms.clone()


def make_sensor(imu, n: int, const: dict, dtype):
    s = object.__new__(imu.Imu)
    s._initialize_handle = s._invalidate_initialize_handle = s._debug_vis_handle = None  # SensorBase.__del__
    s.cfg = types.SimpleNamespace(update_period=0.0, history_length=0, debug_vis=False, prim_path="/World/body",
                                  offset=types.SimpleNamespace(pos=tuple(const["offset_pos"]),
                                                               rot=tuple(const["offset_rot"])),
                                  gravity_bias=tuple(const["gravity_bias"]))
    s._is_visualizing = False
    s._device = "cpu"
    s._num_envs = n
    # SensorBase._initialize_impl (sensor_base.py:227-231)
    s._is_outdated = torch.ones(n, dtype=torch.bool)
    s._timestamp = torch.zeros(n)
    s._timestamp_last_update = torch.zeros_like(s._timestamp)
    # Imu.__init__ (imu.py:62) and the real _initialize_buffers_impl (imu.py:184-203) over the fake view
    s._data = sys.modules["isaaclab.sensors.imu.imu_data"].ImuData()
    s._view = _BodyView(n, torch.tensor(const["com"], dtype=torch.float32).to(dtype))
    s._initialize_buffers_impl()
    if dtype != torch.float32:  # the float64 run: the same float32 constants and zeros, promoted
        for k in ("pos_w", "quat_w", "lin_vel_b", "ang_vel_b", "lin_acc_b", "ang_acc_b"):
            setattr(s._data, k, getattr(s._data, k).to(dtype))
        for k in ("_prev_lin_vel_w", "_prev_ang_vel_w", "_offset_pos_b", "_offset_quat_b", "_gravity_bias_w"):
            setattr(s, k, getattr(s, k).to(dtype))
    return s


def _data_rows(s) -> np.ndarray:
    d = s._data
    return np.concatenate([getattr(d, k).numpy().T for k, _, _ in FIELDS]).copy()  # (19, n)


def _prev_rows(s) -> np.ndarray:
    return np.concatenate([s._prev_lin_vel_w.numpy().T, s._prev_ang_vel_w.numpy().T]).copy()  # (6, n)


def run_reference(imu, pose, vel, const, read, resets, dtype):
    """The reference over pose (U, 7, n) / vel (U, 6, n); returns (upd, mask, data, prev) per record."""
    updates, _, n = pose.shape
    s = make_sensor(imu, n, const, dtype)
    dt = DT if dtype == torch.float32 else float(np.float32(DT))
    upd, mask, data, prev = [], [], [], []

    def record(u):
        upd.append(u)
        mask.append(s._is_outdated.numpy().astype(np.uint8).copy())
        s.data  # the read: recomputes the outdated envs
        assert not bool(s._is_outdated.any())
        data.append(_data_rows(s))
        prev.append(_prev_rows(s))

    for u in range(updates):
        p = torch.from_numpy(pose[u].T.copy()).to(dtype)
        s._view.transforms = torch.cat([p[:, :3], p[:, 4:7], p[:, 3:4]], 1)  # PhysX: (x, y, z, w)
        s._view.velocities = torch.from_numpy(vel[u].T.copy()).to(dtype)
        s.update(dt)
        if read[u]:
            record(u)
        if resets[u].any():
            assert read[u]
            s.reset(np.nonzero(resets[u])[0].tolist())
            record(u)
    return np.array(upd, np.int32), np.stack(mask), np.stack(data), np.stack(prev)


def motion(rng, updates: int, n: int, full_range: bool = True):
    """Smooth random poses (tilt up to 0.6 rad, any yaw) and velocities (|w| up to 6 rad/s), float32."""
    t = np.arange(updates)[:, None] * DT  # (U, 1)

    def wave(scale, rows):
        f = rng.uniform(0.5, 6.0, (rows, 1, n))
        ph = rng.uniform(0, 2 * np.pi, (rows, 1, n))
        a = rng.uniform(0.3, 1.0, (rows, 1, n)) * scale
        return (a * np.sin(2 * np.pi * f * t[None] + ph)).transpose(1, 0, 2)  # (U, rows, n)

    pos = wave(0.5, 3) + rng.uniform(-2, 2, (1, 3, n)) + np.array([0.0, 0.0, 1.3])[None, :, None]
    yaw = wave(1.5, 1)[:, 0] + rng.uniform(-np.pi, np.pi, (1, n))
    tilt = 0.3 + 0.3 * wave(1.0, 1)[:, 0]  # in [0, 0.6]
    az = wave(2.0, 1)[:, 0] + rng.uniform(-np.pi, np.pi, (1, n))
    # q = yaw about z, then a tilt about an axis in the xy plane
    qy = np.stack([np.cos(yaw / 2), 0 * yaw, 0 * yaw, np.sin(yaw / 2)], 1)
    qt = np.stack([np.cos(tilt / 2), np.sin(tilt / 2) * np.cos(az), np.sin(tilt / 2) * np.sin(az), 0 * az], 1)
    w1, x1, y1, z1 = (qy[:, k] for k in range(4))
    w2, x2, y2, z2 = (qt[:, k] for k in range(4))
    q = np.stack([w1 * w2 - x1 * x2 - y1 * y2 - z1 * z2, w1 * x2 + x1 * w2 + y1 * z2 - z1 * y2,
                  w1 * y2 - x1 * z2 + y1 * w2 + z1 * x2, w1 * z2 + x1 * y2 - y1 * x2 + z1 * w2], 1)
    assert tilt.min() >= 0 and tilt.max() <= 0.6 and (tilt.max() > 0.5 or not full_range)
    lin = wave(2.0, 3)
    ang = wave(1.0, 3)
    ang *= np.minimum(1.0, 6.0 / np.linalg.norm(ang, axis=1, keepdims=True)) * rng.uniform(1.0, 6.0, (1, 1, n))
    ang *= np.minimum(1.0, 6.0 / np.linalg.norm(ang, axis=1, keepdims=True))
    assert np.linalg.norm(ang, axis=1).max() <= 6.0 + 1e-9 and (np.linalg.norm(ang, axis=1).max() > 4 or not full_range)
    pose = np.concatenate([pos, q], 1).astype(np.float32)
    return pose, np.concatenate([lin, ang], 1).astype(np.float32)


def f32(values) -> list:
    return [float(np.float32(x)) for x in values]


FULL: dict = {}  # every record of both runs (--full)


def run_case(imu, arrays, cases, name, pose, vel, const, read, resets, stored=None, motion_of=None):
    upd, mask, data, prev = run_reference(imu, pose, vel, const, read, resets, torch.float32)
    upd64, mask64, data64, _ = run_reference(imu, pose, vel, const, read, resets, torch.float64)
    assert data.dtype == np.float32 and prev.dtype == np.float32 and data64.dtype == np.float64
    assert np.array_equal(upd, upd64) and np.array_equal(mask, mask64)
    e_ref = {k: float(np.abs(data[:, lo:hi] - data64[:, lo:hi]).max()) for k, lo, hi in FIELDS}
    stored = list(range(len(upd))) if stored is None else stored
    if motion_of is None:
        arrays.update({f"{name}_pose": pose, f"{name}_vel": vel})
    arrays.update({f"{name}_upd": upd, f"{name}_mask": mask, f"{name}_data64": data64[stored]})
    FULL.update({f"{name}_data": data, f"{name}_prev": prev, f"{name}_data64": data64})
    cases.append({"name": name, "n": int(pose.shape[2]), "dt": DT, "updates": int(pose.shape[0]),
                  "records": int(len(upd)), "motion": motion_of or name, "stored": stored, **const, "e_ref": e_ref})
    return mask


def generate(reference: str) -> dict:
    imu = load_reference(reference)
    rng = np.random.default_rng(20261020)
    arrays: dict[str, np.ndarray] = {}
    cases: list = []

    # ---- a: read after every update
    n, updates = 67, 48
    pose, vel = motion(rng, updates, n)
    const_a = {"offset_pos": f32((0, 0, 0)), "offset_rot": f32((1, 0, 0, 0)), "com": f32((0.013, -0.021, 0.052)),
               "gravity_bias": f32((0, 0, 9.81))}
    none = np.zeros((updates, n), bool)
    mask = run_case(imu, arrays, cases, "a", pose, vel, const_a, np.ones(updates, bool), none,
                    stored=[0, 1, 2] + list(range(5, updates, 6)))
    assert mask.all() and len(mask) == updates

    # ---- b: a tilted offset, no bias, read every fourth update, resets after the read
    rot = np.array([0.8, 0.3, -0.4, 0.2])
    rot /= np.linalg.norm(rot)  # a rotated, non-axis offset quaternion; used as its float32 rounding gives it
    const_b = {"offset_pos": f32((0.1, -0.05, 0.2)), "offset_rot": f32(rot), "com": const_a["com"],
               "gravity_bias": f32((0, 0, 0))}
    read = np.zeros(updates, bool)
    read[3::4] = True
    resets = np.zeros((updates, n), bool)
    resets[3::4] = rng.random((updates // 4, n)) < 0.12
    mask = run_case(imu, arrays, cases, "b", pose, vel, const_b, read, resets, motion_of="a")
    assert resets.sum() >= n, resets.sum()  # resets then read: at least n times
    assert np.array_equal(mask[1::2], resets[3::4].astype(np.uint8)) and mask[0::2].all()

    # ---- c: n = 3, masked resets in updates already read
    n, updates = 3, 4
    pose, vel = motion(rng, updates, n, full_range=False)
    resets = np.zeros((updates, n), bool)
    resets[1, 1] = True
    resets[2, [0, 2]] = True
    mask = run_case(imu, arrays, cases, "c", pose, vel, const_b | {"gravity_bias": f32((0, 0, 9.81))},
                    np.ones(updates, bool), resets)
    d, p = FULL["c_data"], FULL["c_prev"]
    assert mask.tolist() == [[1, 1, 1], [1, 1, 1], [0, 1, 0], [1, 1, 1], [1, 0, 1], [1, 1, 1]]
    # the untouched envs' buffers are unchanged, the reset ones recomputed against their own new prev
    assert np.array_equal(d[2][:, [0, 2]], d[1][:, [0, 2]]) and np.array_equal(p[2], p[1])
    assert not np.array_equal(d[2][13:16, 1], d[1][13:16, 1]) and (d[2][16:19, 1] == 0).all()
    assert np.array_equal(d[4][:, 1], d[3][:, 1]) and not np.array_equal(d[4][13:16, 0], d[3][13:16, 0])

    arrays["cases"] = np.array(json.dumps(cases))
    return arrays


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reference", default=os.environ.get("ALLSTEPS_REFERENCE"), help="root of a reference checkout")
    ap.add_argument("--check", action="store_true", help="compare with the committed file instead of writing it")
    ap.add_argument("--full", metavar="PATH", help="also write every record of the float32 and float64 runs to PATH")
    a = ap.parse_args(argv)
    if not a.reference:
        ap.error("--reference DIR (or ALLSTEPS_REFERENCE) is needed")
    arrays = generate(a.reference)
    if a.full:
        np.savez_compressed(a.full, **FULL)
    if a.check:
        have = dict(np.load(OUT)) if os.path.exists(OUT) else {}
        same = set(have) == set(arrays) and all(
            have[k].dtype == arrays[k].dtype and have[k].shape == arrays[k].shape
            and have[k].tobytes() == arrays[k].tobytes() for k in arrays)
        print(f"imu.npz: {'identical' if same else 'DIFFERS'} ({len(arrays)} arrays)")
        return 0 if same else 1
    np.savez_compressed(OUT, **{k: arrays[k] for k in sorted(arrays)})
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes)")
    for c in json.loads(str(arrays["cases"])):
        print(c["name"], c["records"], "records, e_ref", {k: f"{v:.2e}" for k, v in c["e_ref"].items()})
    return 0


if __name__ == "__main__":
    sys.exit(main())
