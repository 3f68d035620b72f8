"""Generate tests/golden/contact_timers.npz from the reference's own contact-sensor code.

Loads ``isaaclab/sensors/sensor_base.py`` and ``isaaclab/sensors/contact_sensor/contact_sensor.py`` (with its
``contact_sensor_data.py``) of a reference checkout BY PATH, with stub modules of this file's own for the Isaac /
Omniverse packages they import.  A ``ContactSensor`` is built with ``object.__new__`` and its buffers are set by
hand (track_air_time = True, history_length = 4, update_period = 0: allsteps_env_cfg.py:119-130); its
``contact_physx_view.get_net_contact_forces`` is a fake that returns recorded forces.  Every sensor update is the
reference's real ``SensorBase.update(dt)`` (the float32 timestamp arithmetic, the outdated test) and through it
``_update_buffers_impl``; resets are the real ``ContactSensor.reset(env_ids)`` followed by a read of ``.data``, as
the task makes one after its resets (an update of the reset envs with zero elapsed time, which leaves the zeros).

The recorded forces are ``impulse / float32(dt)`` in float32 of impulses the fixture keeps: the step's contact
report holds impulses, and csrc/allsteps_contact_timers.h divides them the same way.  All arrays are env-minor,
the layout of the device buffers: impulses (updates, B, 3, n), timers (records, 4, B, n) in the row order
current_air, last_air, current_contact, last_contact, timestamps (records, n), resets (updates, n) -- the envs
reset AFTER that update; timers and timestamps are recorded after the resets.

  a   n = 70, B = 2, 240 updates at dt = 1/240, threshold 1.0: contact made and broken several times per body,
      off-axis forces, resets of some envs after every fourth update (an env step); a record per update
  b   n = 3, B = 2, 3600 updates without a reset (the longest episode, 900 steps x 4): the elapsed time is the
      float32 difference of two timestamps and drifts from dt in the last bits as the timestamp grows; a record
      per fourth update; the impulses are two vectors per body (in contact / in the air) picked by a pattern
  c0  threshold edges at the default threshold 1.0: a force of exactly the threshold along each axis (not a
      contact), one float32 ulp above it, zero force, negative components
  c1  the same at the non-default threshold 2.0

    python tests/golden/gen_contact_timers.py --reference DIR [--check]

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
OUT = os.path.join(HERE, "contact_timers.npz")
PKG = os.path.join("source", "isaaclab", "isaaclab")
ROWS = ("current_air_time", "last_air_time", "current_contact_time", "last_contact_time")


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
    spec.loader.exec_module(m)
    return m


def load_reference(root: str):
    """The reference's contact_sensor module at ``root``, over its real sensor_base and contact_sensor_data."""
    pkg = os.path.join(root, PKG, "sensors")
    for name in ("omni", "omni.kit", "omni.physics", "omni.physics.tensors", "omni.physics.tensors.impl", "isaaclab",
                 "isaaclab.utils", "isaaclab.sensors", "isaaclab.sensors.contact_sensor"):
        _mod(name)
    _mod("omni.kit.app")
    _mod("omni.timeline")
    _mod("omni.physics.tensors.impl.api")
    _mod("carb")
    _mod("pxr", PhysxSchema=_Any())
    _mod("isaaclab.sim")
    _mod("isaaclab.utils.string")
    _mod("isaaclab.utils.math", convert_quat=_Any())
    _mod("isaaclab.markers", VisualizationMarkers=_Any)
    _load("isaaclab.sensors.sensor_base", os.path.join(pkg, "sensor_base.py"), "isaaclab.sensors")
    _load("isaaclab.sensors.contact_sensor.contact_sensor_data",
          os.path.join(pkg, "contact_sensor", "contact_sensor_data.py"), "isaaclab.sensors.contact_sensor")
    return _load("isaaclab.sensors.contact_sensor.contact_sensor",
                 os.path.join(pkg, "contact_sensor", "contact_sensor.py"), "isaaclab.sensors.contact_sensor")


class _ContactView:
    """Stands in for the PhysX RigidContactView: the recorded forces of the current update, (n * B, 3)."""

    def __init__(self):
        self.forces = None

    def get_net_contact_forces(self, dt):
        return self.forces.clone()


def make_sensor(cs, n: int, bodies: int, dt: float, threshold: float):
    s = object.__new__(cs.ContactSensor)
    s._initialize_handle = s._invalidate_initialize_handle = s._debug_vis_handle = None  # SensorBase.__del__
    s.cfg = types.SimpleNamespace(track_air_time=True, force_threshold=threshold, history_length=4,
                                  update_period=0.0, filter_prim_paths_expr=[], track_pose=False)
    s._is_visualizing = False
    s._device = "cpu"
    s._num_envs, s._num_bodies, s._sim_physics_dt = n, bodies, dt
    # SensorBase._initialize_impl (sensor_base.py:227-231)
    s._is_outdated = torch.ones(n, dtype=torch.bool)
    s._timestamp = torch.zeros(n)
    s._timestamp_last_update = torch.zeros_like(s._timestamp)
    # ContactSensor._initialize_impl (contact_sensor.py:294-312)
    s._data = sys.modules["isaaclab.sensors.contact_sensor.contact_sensor_data"].ContactSensorData()
    s._data.net_forces_w = torch.zeros(n, bodies, 3)
    s._data.net_forces_w_history = torch.zeros(n, 4, bodies, 3)
    for row in ROWS:
        setattr(s._data, row, torch.zeros(n, bodies))
    s._contact_physx_view = _ContactView()
    return s


def _timers(s) -> np.ndarray:
    return np.stack([getattr(s._data, row).numpy().T.copy() for row in ROWS])  # (4, B, n)


def run_case(cs, arrays, name, imp, dt, threshold, resets=None, stride=1, store_impulses=True):
    """The reference over impulses (U, B, 3, n); returns the case's entry and the branch counts."""
    updates, bodies, _, n = imp.shape
    dt32 = np.float32(dt)
    forces = (imp / dt32).astype(np.float32)  # get_net_contact_forces(dt): an IEEE float32 division
    # off-axis forces stay clear of the threshold, so that torch.norm's rounding and a sqrtf of the three squares
    # summed in order cannot disagree about the contact
    f64 = forces.astype(np.float64)
    norm = np.sqrt((f64 ** 2).sum(2))
    off_axis = (forces != 0).sum(2) > 1
    assert (np.abs(norm - threshold)[off_axis] > 1e-3 * threshold).all(), name
    s = make_sensor(cs, n, bodies, dt, threshold)
    out_t, out_ts = [], []
    seen = dict(first_contact=0, first_detach=0, stay_air=0, stay_contact=0, reset_nonzero=0)
    for u in range(updates):
        air0, con0 = s._data.current_air_time.clone(), s._data.current_contact_time.clone()
        s._contact_physx_view.forces = torch.from_numpy(np.ascontiguousarray(forces[u].transpose(2, 0, 1))).reshape(
            n * bodies, 3)
        s.update(dt)
        contact = torch.from_numpy(norm[u].T > threshold)
        seen["first_contact"] += int(((air0 > 0) & contact).sum())
        seen["first_detach"] += int(((con0 > 0) & ~contact).sum())
        seen["stay_air"] += int(((air0 > 0) & ~contact).sum())
        seen["stay_contact"] += int(((con0 > 0) & contact).sum())
        if resets is not None and resets[u].any():
            ids = np.nonzero(resets[u])[0].tolist()
            seen["reset_nonzero"] += int((_timers(s)[:, :, ids] != 0).any((0, 1)).sum())
            s.reset(ids)
            s.data  # the task's read after its resets: updates the reset envs with zero elapsed time
        if (u + 1) % stride == 0:
            out_t.append(_timers(s))
            out_ts.append(s._timestamp.numpy().copy())
    if store_impulses:
        arrays[f"{name}_impulses"] = imp
    if resets is not None:
        arrays[f"{name}_resets"] = resets.astype(np.uint8)
    arrays[f"{name}_timers"] = np.stack(out_t)
    arrays[f"{name}_timestamp"] = np.stack(out_ts)
    return {"name": name, "dt": dt, "threshold": threshold, "updates": updates, "stride": stride, "n": n,
            "bodies": bodies}, seen


def impulse_for(force: np.float32, dt32: np.float32) -> np.float32:
    """An impulse whose float32 quotient by dt32 is exactly ``force``."""
    lo = hi = np.float32(force * dt32)
    for _ in range(4):  # the product, then its float32 neighbours, three either side
        for c in (lo, hi):
            if np.float32(c / dt32) == force:
                return np.float32(c)
        lo, hi = np.nextafter(lo, np.float32(-np.inf)), np.nextafter(hi, np.float32(np.inf))
    raise ValueError(f"no impulse divides to {force!r}")


def _directions(rng, shape):
    v = rng.normal(0.0, 1.0, shape + (3,))
    v[..., 2] = np.abs(v[..., 2]) + 1.0  # mostly upwards, never along one axis alone
    return v / np.linalg.norm(v, axis=-1, keepdims=True)


def case_a_impulses(rng, updates, n, bodies, dt32):
    """Runs of contact (|f| in [2, 600] N) and of air (zero, or |f| in [0.01, 0.9] N) of 1 .. 24 updates."""
    imp = np.zeros((updates, bodies, 3, n), np.float32)
    for e in range(n):
        for b in range(bodies):
            u, contact = 0, bool(rng.integers(2))
            while u < updates:
                run = int(rng.integers(1, 25))
                for k in range(u, min(u + run, updates)):
                    if k == u or rng.integers(4) == 0:  # the force holds for a few updates (and the file packs)
                        if contact:
                            mag = float(np.exp(rng.uniform(np.log(2.0), np.log(600.0))))
                        else:
                            mag = 0.0 if rng.integers(2) else float(rng.uniform(0.01, 0.9))
                        v = (_directions(rng, ()) * mag * float(dt32)).astype(np.float32)
                    imp[k, b, :, e] = v
                u += run
                contact = not contact
    return imp


def threshold_case(threshold: float, dt32: np.float32):
    """(U, 2, 3, n) impulses around ``threshold``: env e < 3 tests axis e with the exact threshold, env 3 + e one
    ulp above it; body 1 takes the negated force.  The rows alternate the edge with zero and clear forces so that
    every timer moves."""
    thr = np.float32(threshold)
    above = np.nextafter(thr, np.float32(np.inf))
    at, up = impulse_for(thr, dt32), impulse_for(above, dt32)
    big, small = np.float32(8) * thr * dt32, thr / np.float32(4) * dt32
    seq = {"at": [big, at, at, big, 0.0, at, big, big, at, 0.0, big, at],
           "up": [0.0, up, up, 0.0, big, up, 0.0, small, up, up, 0.0, up]}
    n, updates = 6, 12
    imp = np.zeros((updates, 2, 3, n), np.float32)
    for e in range(n):
        for u, v in enumerate(seq["at" if e < 3 else "up"]):
            imp[u, 0, e % 3, e] = v
            imp[u, 1, e % 3, e] = -np.float32(v)
    return imp


def generate(reference: str) -> dict:
    cs = load_reference(reference)
    rng = np.random.default_rng(20261020)
    arrays: dict[str, np.ndarray] = {}
    cases = []
    dt = 1 / 240
    dt32 = np.float32(dt)

    # ---- a: contact made and broken, resets after env steps
    n, bodies, updates = 70, 2, 240
    imp = case_a_impulses(rng, updates, n, bodies, dt32)
    resets = np.zeros((updates, n), bool)
    resets[3::4] = rng.random((updates // 4, n)) < 0.04
    c, seen = run_case(cs, arrays, "a", imp, dt, 1.0, resets)
    assert all(v > 0 for v in seen.values()), seen  # every branch of the update occurs, and a reset of live timers
    assert seen["first_contact"] > 4 * n and seen["first_detach"] > 4 * n, seen
    cases.append(c)

    # ---- b: 3600 updates without a reset
    n, updates = 3, 3600
    pattern = np.zeros((updates, bodies, n), np.uint8)  # env 0: body 0 always in the air, body 1 always in contact
    u = np.arange(updates)
    pattern[:, 1, 0] = 1
    pattern[:, 0, 1] = (u // 700) % 2  # env 1: long phases
    pattern[:, 1, 1] = (u // 1100 + 1) % 2
    pattern[:, 0, 2] = (u % 37) < 30   # env 2: a gait
    pattern[:, 1, 2] = ((u + 18) % 37) < 30
    vec = np.zeros((2, bodies, 3, n), np.float32)  # [0]: in the air, [1]: in contact
    vec[0] = (_directions(rng, (bodies, n)).transpose(0, 2, 1) * rng.uniform(0.0, 0.5, (bodies, 1, n)) * dt).astype(
        np.float32)
    vec[1] = (_directions(rng, (bodies, n)).transpose(0, 2, 1) * rng.uniform(50, 300, (bodies, 1, n)) * dt).astype(
        np.float32)
    imp = np.where(pattern[:, :, None, :] != 0, vec[1][None], vec[0][None]).astype(np.float32)
    arrays["b_pattern"], arrays["b_vectors"] = pattern, vec
    c, seen = run_case(cs, arrays, "b", imp, dt, 1.0, stride=4, store_impulses=False)
    ts = arrays["b_timestamp"]
    steps = np.diff(ts[:, 0])
    assert len(np.unique(steps)) > 1, "the timestamp's steps never left one value: no drift in this run"
    cases.append(c)

    # ---- c: threshold edges
    for k, thr in enumerate((1.0, 2.0)):
        c, seen = run_case(cs, arrays, f"c{k}", threshold_case(thr, dt32), dt, thr)
        t = arrays[f"c{k}_timers"]
        # the exact threshold is not a contact (env 0, update 1: in the air after a contact), an ulp above it is
        assert t[1, 0, 0, 0] > 0 and t[1, 2, 0, 0] == 0 and t[1, 2, 0, 3] > 0 and t[1, 0, 0, 3] == 0
        cases.append(c)

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
        print(f"contact_timers.npz: {'identical' if same else 'DIFFERS'} ({len(arrays)} arrays)")
        return 0 if same else 1
    np.savez_compressed(OUT, **{k: arrays[k] for k in sorted(arrays)})
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes)")
    return 0


if __name__ == "__main__":
    sys.exit(main())
