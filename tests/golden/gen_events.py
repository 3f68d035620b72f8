"""Generate tests/golden/events.npz from the reference's own event code.

Loads ``isaaclab/managers/event_manager.py`` and ``isaaclab/envs/mdp/events.py`` of a reference checkout BY PATH,
with stub modules of this file's own for the Isaac / Omniverse packages they import and the reference's real
``isaaclab/utils/math.py``, and runs ``EventManager.apply(mode="interval", dt=...)`` with
``push_by_setting_velocity`` terms on the CPU.  The manager is built with ``object.__new__`` and its term lists
and ``_interval_term_time_left`` are set by hand; ``torch.rand`` of both modules is replaced by recorded draws,
kept per (step, term, env) and handed out for the envs that fire.  The fixture holds inputs, draws and the
reference's outputs:

  a   two terms over 40 steps at dt = 4/240, n = 66, intervals short enough that every env fires several times,
      ranges that are Python floats and not float32 values; the initial timers are the reference's expression
      ``rand(n) * (hi - lo) + lo`` (event_manager.py:384) on recorded draws
  b   one step from hand-set timers that straddle the ``time_left < 1e-6`` test: exactly dt, one ulp either side,
      a sweep of ulps around dt + 1e-6
  c   a term with an empty velocity_range (a root velocity of -0.0 becomes +0.0)

    python tests/golden/gen_events.py [--reference DIR] [--check]

--check regenerates into memory and compares with the committed file byte for byte.
"""

from __future__ import annotations

import argparse
import importlib.util
import io
import json
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "events.npz")
DEFAULT_REFERENCE = os.environ.get("ALLSTEPS_REFERENCE", "/root/reference")
PKG = os.path.join("source", "isaaclab", "isaaclab")
N = 66


class _Any:
    def __init__(self, *a, **k):
        pass

    def __getattr__(self, name):
        return _Any()

    def __call__(self, *a, **k):
        return _Any()


class _SceneEntityCfg:
    def __init__(self, name, **kwargs):
        self.name = name
        self.body_ids = slice(None)


class _ManagerBase:
    device = "cpu"


class _Draws:
    """Stands in for a module's ``torch``: ``rand`` hands out the recorded draws of the envs that fire.  The
    term being served is known from the read of its ``interval_range_s`` (event_manager.py:220), the envs from the
    manager's own ``time_left < 1e-6`` at that moment."""

    def __init__(self):
        self.mgr = None
        self.term = None
        self.ids = None
        self.iv = self.push = self.fired = None

    def __getattr__(self, name):
        return getattr(torch, name)

    def rand(self, *size, device=None):
        if len(size) == 1 and isinstance(size[0], (tuple, torch.Size)):
            size = tuple(size[0])
        k = self.term
        if len(size) == 1:  # the interval resample
            self.ids = (self.mgr._interval_term_time_left[k] < 1e-6).nonzero().flatten()
            assert len(self.ids) == size[0], (len(self.ids), size)
            self.fired[k, self.ids] = 1
            return self.iv[k][self.ids]
        assert tuple(size) == (len(self.ids), 6), (size, len(self.ids))  # sample_uniform of the push
        return self.push[k][self.ids]


class _Term:
    """An EventTermCfg stand-in: reading ``interval_range_s`` tells the draws which term is being served."""

    is_global_time = False

    def __init__(self, draws, index, func, interval_range_s, params):
        self._draws, self._index, self._range = draws, index, interval_range_s
        self.func, self.params = func, params

    @property
    def interval_range_s(self):
        self._draws.term = self._index
        return self._range


class _Asset:
    device = "cpu"

    def __init__(self, vel):
        self.data = types.SimpleNamespace(root_vel_w=vel)

    def write_root_velocity_to_sim(self, vel, env_ids=None):
        self.data.root_vel_w[env_ids] = vel


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
    """(event_manager module, events module, draws) of the reference at ``root``."""
    pkg = os.path.join(root, PKG)
    for name in ("omni", "omni.physics", "omni.physics.tensors", "omni.physics.tensors.impl",
                 "omni.physics.tensors.impl.api", "carb", "isaaclab", "isaaclab.utils", "isaaclab.envs",
                 "isaaclab.envs.mdp"):
        _mod(name)
    _mod("omni.log", warn=lambda *a, **k: None)
    _mod("prettytable", PrettyTable=_Any)
    _mod("isaaclab.sim")
    _mod("isaaclab.actuators", ImplicitActuator=_Any)
    _mod("isaaclab.assets", Articulation=_Any, DeformableObject=_Any, RigidObject=_Any)
    _mod("isaaclab.terrains", TerrainImporter=_Any)
    term_base = type("ManagerTermBase", (), {})
    term_cfg = type("EventTermCfg", (), {})
    _mod("isaaclab.managers", EventTermCfg=term_cfg, ManagerTermBase=term_base, SceneEntityCfg=_SceneEntityCfg)
    _mod("isaaclab.managers.manager_base", ManagerBase=_ManagerBase, ManagerTermBase=term_base)
    _mod("isaaclab.managers.manager_term_cfg", EventTermCfg=term_cfg)
    math_mod = _load("isaaclab.utils.math", os.path.join(pkg, "utils", "math.py"), "isaaclab.utils")
    sys.modules["isaaclab.utils"].math = math_mod
    em = _load("isaaclab.managers.event_manager", os.path.join(pkg, "managers", "event_manager.py"),
               "isaaclab.managers")
    ev = _load("isaaclab.envs.mdp.events", os.path.join(pkg, "envs", "mdp", "events.py"), "isaaclab.envs.mdp")
    draws = _Draws()
    em.torch = draws
    math_mod.torch = draws  # sample_uniform's torch.rand
    return em, ev, draws


def _uniform24(rng, shape):
    return rng.integers(0, 1 << 24, shape).astype(np.float32) / np.float32(1 << 24)


def _orders_differ(lo: float, hi: float) -> bool:
    return np.float32(hi - lo) != np.float32(hi) - np.float32(lo)


def run_case(em, ev, draws, arrays, name, terms, dt, steps, vel0, time_left0, rng):
    """``steps`` calls of the reference's EventManager.apply(mode="interval", dt=dt) from the given state."""
    k = len(terms)
    cfgs = [_Term(draws, i, ev.push_by_setting_velocity, t["interval_range_s"],
                  {"velocity_range": {a: tuple(b) for a, b in t["velocity_range"].items()},
                   "asset_cfg": _SceneEntityCfg("robot")}) for i, t in enumerate(terms)]
    asset = _Asset(torch.from_numpy(vel0.copy()))
    mgr = object.__new__(em.EventManager)
    mgr._mode_term_names = {"interval": [t["name"] for t in terms]}
    mgr._mode_term_cfgs = {"interval": cfgs}
    mgr._mode_class_term_cfgs = {"interval": []}
    mgr._interval_term_time_left = [torch.from_numpy(time_left0[i].copy()) for i in range(k)]
    mgr._env = types.SimpleNamespace(scene={"robot": asset}, num_envs=N)
    draws.mgr = mgr
    iv = _uniform24(rng, (steps, k, N))
    push = _uniform24(rng, (steps, k, N, 6))
    tl = np.zeros((steps, k, N), np.float32)
    fired = np.zeros((steps, k, N), np.uint8)
    vel = np.zeros((steps, N, 6), np.float32)
    for s in range(steps):
        draws.iv, draws.push = torch.from_numpy(iv[s]), torch.from_numpy(push[s])
        draws.fired = fired[s]
        draws.term = draws.ids = None
        mgr.apply(mode="interval", dt=dt)
        tl[s] = np.stack([x.numpy() for x in mgr._interval_term_time_left])
        vel[s] = asset.data.root_vel_w.numpy()
    arrays.update({f"{name}_vel0": vel0, f"{name}_time_left0": time_left0, f"{name}_iv_draws": iv,
                   f"{name}_push_draws": push, f"{name}_time_left": tl, f"{name}_fired": fired, f"{name}_vel": vel})
    return {"name": name, "dt": dt, "steps": steps, "terms": terms}


def generate(reference: str) -> dict:
    em, ev, draws = load_reference(reference)
    rng = np.random.default_rng(20251020)
    arrays: dict[str, np.ndarray] = {}
    cases = []
    dt = 4 / 240

    # ---- a: two terms, 40 steps; ranges that are not float32 values
    terms = [{"name": "push_robot", "interval_range_s": [0.05, 0.18],
              "velocity_range": {"x": [-0.3, 0.7], "y": [-0.41, 0.43], "yaw": [-0.11, 0.23]}},
             {"name": "push_again", "interval_range_s": [0.03, 0.27],
              "velocity_range": {"x": [0.1, 0.3], "y": [-0.07, 0.07], "z": [-0.05, 0.15], "roll": [-0.2, 0.1],
                                 "pitch": [0.07, 0.31], "yaw": [-0.9, -0.6]}}]
    # the double and the float32 subtraction give different widths for these, so the fixture pins which is which
    assert all(_orders_differ(*t["interval_range_s"]) for t in terms)
    assert sum(_orders_differ(*r) for t in terms for r in t["velocity_range"].values()) >= 4
    u0 = _uniform24(rng, (2, N))
    tl0 = np.stack([(torch.from_numpy(u0[i]) * (t["interval_range_s"][1] - t["interval_range_s"][0])
                     + t["interval_range_s"][0]).numpy() for i, t in enumerate(terms)])  # event_manager.py:384
    arrays["a_init_draws"] = u0
    vel0 = rng.normal(0.0, 0.8, (N, 6)).astype(np.float32)
    cases.append(run_case(em, ev, draws, arrays, "a", terms, dt, 40, vel0, tl0, rng))
    assert arrays["a_fired"].sum(0).min() >= 2, "every env must fire several times in every term"

    # ---- b: one step from timers around the fire test
    dt32 = np.float32(dt)
    ulp = np.spacing(dt32)
    tl = [dt32, dt32 - ulp, dt32 + ulp, np.float32(0.0), -dt32, np.float32(2) * dt32, np.float32(1e-6),
          np.float32(dt + 1e-6), np.float32(dt + 9.9e-7), np.float32(dt + 1.01e-6), np.float32(dt / 2),
          np.float32(1.0)]
    tl += [dt32 + np.float32(m) * ulp for m in range(515, 515 + N - len(tl))]
    tl0 = np.asarray(tl, np.float32).reshape(1, N)
    terms = [{"name": "push_robot", "interval_range_s": [0.04, 0.28],
              "velocity_range": {"x": [-0.5, 0.5], "roll": [-0.13, 0.17]}}]
    vel0 = rng.normal(0.0, 0.8, (N, 6)).astype(np.float32)
    cases.append(run_case(em, ev, draws, arrays, "b", terms, dt, 1, vel0, tl0, rng))
    f = arrays["b_fired"][0, 0]
    assert f[:3].all() and 0 < f[12:].sum() < N - 12, "the sweep must straddle the test"

    # ---- c: an empty velocity_range
    terms = [{"name": "no_push", "interval_range_s": [0.02, 0.06], "velocity_range": {}}]
    vel0 = rng.normal(0.0, 0.8, (N, 6)).astype(np.float32)
    vel0[0, 0] = -0.0
    vel0[1, 4] = -0.0
    tl0 = (_uniform24(rng, (1, N)) * np.float32(0.04) + np.float32(0.02)).astype(np.float32)
    cases.append(run_case(em, ev, draws, arrays, "c", terms, dt, 10, vel0, tl0, rng))
    assert arrays["c_fired"].sum(0).min() >= 1

    arrays["cases"] = np.array(json.dumps(cases))
    return arrays


def serialise(arrays: dict) -> bytes:
    buf = io.BytesIO()
    np.savez(buf, **{k: arrays[k] for k in sorted(arrays)})
    return buf.getvalue()


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reference", default=DEFAULT_REFERENCE, help="root of a reference checkout")
    ap.add_argument("--check", action="store_true", help="compare with the committed file instead of writing it")
    a = ap.parse_args(argv)
    data = serialise(generate(a.reference))
    if a.check:
        same = os.path.exists(OUT) and open(OUT, "rb").read() == data
        print(f"events.npz: {'identical' if same else 'DIFFERS'} ({len(data)} bytes)")
        return 0 if same else 1
    with open(OUT, "wb") as f:
        f.write(data)
    print(f"wrote {OUT} ({len(data)} bytes)")
    return 0


if __name__ == "__main__":
    sys.exit(main())
