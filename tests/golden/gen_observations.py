"""Generate tests/golden/observations.npz from the reference's own observation code.

Loads ``isaaclab/managers/observation_manager.py``, ``isaaclab/utils/buffers/circular_buffer.py``,
``isaaclab/envs/mdp/observations.py``, ``isaaclab/utils/noise/noise_model.py`` and ``isaaclab/utils/math.py`` of a
reference checkout BY PATH, with stub modules of this file's own for the Isaac / Omniverse packages they import, and
drives the real ``ObservationManager.reset(env_ids)`` / ``compute()`` on the CPU over a stub env, in the order of
``ManagerBasedRLEnv.step``: the reset of the step's done envs (their last action becomes zero, as
``action_manager.reset`` leaves it), then compute.  The stub env's robot, command term, ray caster and IMU data are
recorded arrays; the robot's base-frame quantities are the expressions of articulation_data.py:513-515, 604-619 over
the reference's ``quat_rotate_inverse``.  The manager's base class is a stub that keeps the cfg and calls the real
``_prepare_terms``; the cfg classes it checks with ``isinstance`` are this project's (same fields).

``torch.rand_like`` / ``torch.randn_like`` of noise_model.py are replaced by recorded draws: each term's noise
function is wrapped so that the call knows the term's first column, and the draw of column c of the group (before the
history) for env e in step s is ``draws[s, c, e]`` -- a uniform in [0, 1) or a unit normal, as the term's noise takes
it.  Nothing else is replaced: the noise formulas, the clip, the scale and the CircularBuffer are the reference's.

Every array is in the kernel's layout: sources field-major / env-minor (rows, n), the actions (n, A), the expected
group output (steps, n, columns) with a term's history slots side by side, oldest first.  Inputs are multiples of
2^-8 (and draws of 2^-12) so that the file compresses; the outputs carry full float32 results.

Cases (n = 66, 12 joints, 12 actions, a 3 x 3 ray pattern, one IMU, one command term):

  a   the velocity task's policy group: base_lin_vel, base_ang_vel, projected_gravity, generated_commands,
      joint_pos_rel, joint_vel_rel, last_action, height_scan with clip (-1, 1); uniform noise on every term but the
      commands and the actions, 12 steps; reset masks at steps 0, 3, 4, 7, 10, env 5 in two steps running
  b   the same group, inputs and draws with group history_length = 3, 8 steps; resets such that in step 5 there are
      envs at push count 0, 1, 2 and >= 3
  c   one term each of the remaining functions -- base_pos_z, root_pos_w, root_quat_w (make_quat_unique, with w < 0
      and w = +-0), root_lin_vel_w, root_ang_vel_w, joint_pos / joint_pos_limit_normalized / joint_vel on joint_ids
      subsets, imu_orientation, imu_ang_vel, imu_lin_acc, height_scan unclipped and clipped with +inf hits, joint_vel
      with a NaN through clip -- with gaussian, constant and uniform noise in all three operations, per-column
      parameters and a tuple scale; 57 columns (not a multiple of 4), 3 steps
  d   concatenate_terms=False: joint_pos with history 2 and flatten_history_dim=False, base_ang_vel with history 3;
      case c's inputs, 3 steps, a reset in step 1

    python tests/golden/gen_observations.py [--reference DIR] [--check]

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
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "observations.npz")
DEFAULT_REFERENCE = os.environ.get("ALLSTEPS_REFERENCE", "/root/reference")
PKG = os.path.join("source", "isaaclab", "isaaclab")
N, J, A, R = 66, 12, 12, 9

if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


class _Any:
    def __init__(self, *a, **k):
        pass

    def __getattr__(self, name):
        return _Any()

    def __call__(self, *a, **k):
        return _Any()


class _ManagerTermBase:
    pass


class _ManagerBase:
    """manager_base.py ``ManagerBase`` as far as ObservationManager needs it: keep the cfg and the env, prepare the
    terms.  The scene entities of the fixture's terms carry resolved joint_ids already."""

    def __init__(self, cfg, env):
        self.cfg, self._env = cfg, env
        self._prepare_terms()

    def _resolve_common_term_cfg(self, term_name, term_cfg, min_argc=1):
        assert callable(term_cfg.func), term_name


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


class _Draws:
    """Which draws the next rand_like / randn_like hands out: the step's (columns, n) array and the term's column."""

    def __init__(self):
        self.step = None
        self.col = 0

    def take(self, data: torch.Tensor) -> torch.Tensor:
        w = data.shape[1]
        return torch.from_numpy(np.ascontiguousarray(self.step[self.col:self.col + w].T))


class _Torch:
    """Stands in for noise_model's ``torch``: rand_like / randn_like hand out the recorded draws."""

    def __init__(self, draws: _Draws):
        self._d = draws

    def __getattr__(self, name):
        return getattr(torch, name)

    def rand_like(self, data):
        return self._d.take(data)

    randn_like = rand_like


def load_reference(root: str):
    """(observation_manager, observations, noise_model, math modules, draws) of the reference at ``root``."""
    from allsteps_isaaclab_amd.utils.events import SceneEntityCfg
    from allsteps_isaaclab_amd.utils.observations import ObservationGroupCfg, ObservationTermCfg

    pkg = os.path.join(root, PKG)
    for name in ("omni", "carb", "isaaclab", "isaaclab.utils", "isaaclab.envs", "isaaclab.envs.mdp",
                 "isaaclab.utils.noise"):
        _mod(name)
    _mod("omni.log", warn=lambda *a, **k: None)
    _mod("prettytable", PrettyTable=_Any)
    _mod("isaaclab.assets", Articulation=_Any, RigidObject=_Any)
    _mod("isaaclab.sensors", Camera=_Any, Imu=_Any, RayCaster=_Any, RayCasterCamera=_Any, TiledCamera=_Any)
    _mod("isaaclab.utils.modifiers", ModifierBase=_Any, ModifierCfg=_Any)
    _mod("isaaclab.managers", SceneEntityCfg=SceneEntityCfg)
    _mod("isaaclab.managers.manager_base", ManagerBase=_ManagerBase, ManagerTermBase=_ManagerTermBase)
    _mod("isaaclab.managers.manager_term_cfg", ObservationGroupCfg=ObservationGroupCfg,
         ObservationTermCfg=ObservationTermCfg)
    math_mod = _load("isaaclab.utils.math", os.path.join(pkg, "utils", "math.py"), "isaaclab.utils")
    buf = _load("isaaclab.utils.buffers.circular_buffer", os.path.join(pkg, "utils", "buffers", "circular_buffer.py"),
                "isaaclab.utils.buffers")
    _mod("isaaclab.utils.buffers", CircularBuffer=buf.CircularBuffer)
    nm = _load("isaaclab.utils.noise.noise_model", os.path.join(pkg, "utils", "noise", "noise_model.py"),
               "isaaclab.utils.noise")
    om = _load("isaaclab.managers.observation_manager", os.path.join(pkg, "managers", "observation_manager.py"),
               "isaaclab.managers")
    ob = _load("isaaclab.envs.mdp.observations", os.path.join(pkg, "envs", "mdp", "observations.py"),
               "isaaclab.envs.mdp")
    draws = _Draws()
    nm.torch = _Torch(draws)
    return om, ob, nm, math_mod, draws


def verify_stub_formulas(ref) -> dict:
    """The one stand-in, rand_like / randn_like, leaves the noise formulas the reference's: with the real torch
    functions on a seeded generator state the wrapped call and the plain call agree bit for bit."""
    _, _, nm, _, draws = ref
    out = {}
    data = torch.linspace(-2.0, 3.0, N * 5).reshape(N, 5)
    for name, cfg in (("uniform", types.SimpleNamespace(operation="add", n_min=-0.13, n_max=0.29)),
                      ("gaussian", types.SimpleNamespace(operation="scale", mean=0.07, std=0.31))):
        torch.manual_seed(99)
        u = (torch.rand_like if name == "uniform" else torch.randn_like)(data)
        draws.step, draws.col = np.ascontiguousarray(u.numpy().T), 0
        got = getattr(nm, name + "_noise")(data, cfg)
        real, nm.torch = nm.torch, torch
        torch.manual_seed(99)
        want = getattr(nm, name + "_noise")(data, cfg)
        nm.torch = real
        out[name] = bool(torch.equal(got, want))
        assert out[name], name
    return out


# ------------------------------------------------------------------------------------------------ cases
def _q8(x):
    return (np.round(np.asarray(x, np.float64) * 256.0) / 256.0).astype(np.float32)


def _uniform12(rng, shape):
    return (rng.integers(0, 1 << 12, shape).astype(np.float32) / np.float32(1 << 12)).astype(np.float32)


LIMITS = np.stack([_q8(np.linspace(-2.5, -0.5, J)), _q8(np.linspace(0.75, 2.75, J))], -1)  # soft limits (J, 2)
DEFAULT_Q = _q8(np.linspace(-0.4, 0.7, J))
DEFAULT_QD = _q8(np.linspace(0.05, -0.05, J))


def make_inputs(rng, steps: int, special: bool) -> dict:
    q = rng.normal(0.0, 1.0, (steps, 4, N))
    q = _q8(q / np.linalg.norm(q, axis=1, keepdims=True) * (1.0 + 1e-3 * rng.normal(size=(steps, 1, N))))
    x = {"root_pos": _q8(rng.normal(0.0, 1.5, (steps, 3, N))), "root_quat": q,
         "root_lin": _q8(rng.normal(0.0, 1.0, (steps, 3, N))), "root_ang": _q8(rng.normal(0.0, 2.0, (steps, 3, N))),
         "q": _q8(rng.normal(0.0, 1.0, (steps, J, N))), "qd": _q8(rng.normal(0.0, 4.0, (steps, J, N))),
         "actions": _q8(rng.normal(0.0, 0.8, (steps, N, A))), "commands": _q8(rng.normal(0.0, 1.0, (steps, 1, 3, N))),
         "ray_hits": _q8(rng.normal(0.0, 0.6, (steps, 3, R, N))), "ray_pose": _q8(rng.normal(0.6, 0.3, (steps, 7, N))),
         "imu": _q8(rng.normal(0.0, 3.0, (steps, 19, 1, N)))}
    # the sensors and the command hold their values for three steps, as they do between updates and resamples
    for k in ("commands", "ray_hits", "ray_pose"):
        for s in range(steps):
            x[k][s] = x[k][s - s % 3]
    x["ray_hits"][:, 2, 4, 7::11] = np.inf  # misses
    if special:
        x["root_quat"][:, 0, 0] = -0.0
        x["root_quat"][:, 0, 1] = 0.0
        x["root_quat"][:, 0, 2:12] = -np.abs(x["root_quat"][:, 0, 2:12]) - np.float32(1 / 256)
        x["ray_hits"][:, 2, 0, 3::5] = np.inf
        x["qd"][:, 0, 4::9] = np.nan
        x["qd"][:, 8, 5::13] = np.inf
    return x


def _noise(kind, op, p0, p1=None):
    return {"kind": kind, "operation": op, "p0": p0, "p1": p1}


def _term(name, func, params=None, noise=None, clip=None, scale=None, history=0, flatten=True):
    return {"name": name, "func": func, "params": params or {}, "noise": noise, "clip": clip, "scale": scale,
            "history_length": history, "flatten_history_dim": flatten}


def policy_terms() -> list:
    u = lambda lo, hi: _noise("uniform", "add", lo, hi)  # noqa: E731
    return [_term("base_lin_vel", "base_lin_vel", noise=u(-0.1, 0.1)),
            _term("base_ang_vel", "base_ang_vel", noise=u(-0.2, 0.2)),
            _term("projected_gravity", "projected_gravity", noise=u(-0.05, 0.05)),
            _term("velocity_commands", "generated_commands", {"command_name": "base_velocity"}),
            _term("joint_pos", "joint_pos_rel", noise=u(-0.01, 0.01)),
            _term("joint_vel", "joint_vel_rel", noise=u(-1.5, 1.5)),
            _term("actions", "last_action"),
            _term("height_scan", "height_scan", {"sensor": "height_scanner"}, noise=u(-0.1, 0.1), clip=(-1.0, 1.0))]


def other_terms() -> list:
    return [
        _term("base_pos_z", "base_pos_z", noise=_noise("gaussian", "add", 0.02, 0.3)),
        _term("root_pos_w", "root_pos_w", noise=_noise("constant", "add", [0.1, -0.2, 0.3]), scale=(0.5, 2.0, 1.3)),
        _term("root_quat_w", "root_quat_w", {"make_quat_unique": True}),
        _term("root_lin_vel_w", "root_lin_vel_w", noise=_noise("gaussian", "scale", 1.0, [0.1, 0.2, 0.3])),
        _term("root_ang_vel_w", "root_ang_vel_w", noise=_noise("constant", "scale", 1.7), scale=0.3),
        _term("joint_pos", "joint_pos", {"joint_ids": [0, 3, 4, 7, 11]}, noise=_noise("uniform", "scale", 0.8, 1.2)),
        _term("joint_pos_norm", "joint_pos_limit_normalized", {"joint_ids": [1, 2, 9, 10]},
              noise=_noise("uniform", "add", [-0.1, -0.2, -0.3, -0.4], [0.4, 0.3, 0.2, 0.1])),
        _term("joint_vel", "joint_vel", {"joint_ids": [5, 6, 8]}, noise=_noise("gaussian", "abs", 0.5, 2.0), clip=(-3.0, 3.5)),
        _term("imu_orientation", "imu_orientation", {"imu": "imu"}, noise=_noise("constant", "abs", 0.25)),
        _term("imu_ang_vel", "imu_ang_vel", {"imu": "imu"}, noise=_noise("uniform", "abs", -1.0, 1.0), scale=0.25),
        _term("imu_lin_acc", "imu_lin_acc", {"imu": "imu"}, clip=(-4.0, 4.0), scale=(0.1, 0.1, 0.05)),
        _term("height_scan", "height_scan", {"sensor": "height_scanner", "offset": 0.3}),
        _term("height_scan_clipped", "height_scan", {"sensor": "height_scanner"}, clip=(-1.0, 1.0), scale=2.0),
        _term("joint_vel_nan", "joint_vel", {"joint_ids": [0, 7, 8]}, clip=(-5.0, 5.0)),
    ]


def split_terms() -> list:
    return [_term("joint_pos", "joint_pos", {"joint_ids": [2, 3, 5]}, noise=_noise("uniform", "add", -0.1, 0.1),
                  history=2, flatten=False),
            _term("base_ang_vel", "base_ang_vel", scale=0.25, history=3)]


def _mask(ids):
    m = np.zeros(N, np.uint8)
    m[list(ids)] = 1
    return m


def case_specs() -> list:
    ra = {0: range(0, N, 5), 3: (5, 17, 40, 65), 4: (5, 18), 7: range(1, N, 7), 10: (0, 64, 65)}
    rb = {0: range(N), 2: (9,), 3: (1, 2, 3), 4: (4, 5, 6, 1), 5: (7, 8, 4), 7: (0, 65)}
    return [
        {"name": "a", "inputs": "a", "steps": 12, "enable_corruption": True, "concatenate_terms": True,
         "history_length": None, "flatten_history_dim": True, "terms": policy_terms(),
         "reset": [_mask(ra.get(s, ())) for s in range(12)]},
        {"name": "b", "inputs": "a", "steps": 8, "enable_corruption": True, "concatenate_terms": True,
         "history_length": 3, "flatten_history_dim": True, "terms": policy_terms(),
         "reset": [_mask(rb.get(s, ())) for s in range(8)]},
        {"name": "c", "inputs": "c", "steps": 3, "enable_corruption": True, "concatenate_terms": True,
         "history_length": None, "flatten_history_dim": True, "terms": other_terms(),
         "reset": [_mask(()), _mask((3, 4)), _mask(())]},
        {"name": "d", "inputs": "c", "steps": 3, "enable_corruption": True, "concatenate_terms": False,
         "history_length": None, "flatten_history_dim": True, "terms": split_terms(),
         "reset": [_mask(()), _mask((0, 10, 65)), _mask(())]},
    ]


# ------------------------------------------------------------------------------------------------ the stub env
class _RobotData:
    """articulation_data.py:513-515, 604-619 over the reference's math; the rest are recorded arrays."""

    def __init__(self, math_mod):
        self._m = math_mod
        self.GRAVITY_VEC_W = torch.tensor((0.0, 0.0, -1.0)).repeat(N, 1)
        self.default_joint_pos = torch.from_numpy(DEFAULT_Q).repeat(N, 1)
        self.default_joint_vel = torch.from_numpy(DEFAULT_QD).repeat(N, 1)
        self.soft_joint_pos_limits = torch.from_numpy(LIMITS).unsqueeze(0).repeat(N, 1, 1)

    root_lin_vel_b = property(lambda self: self._m.quat_rotate_inverse(self.root_quat_w, self.root_lin_vel_w))
    root_ang_vel_b = property(lambda self: self._m.quat_rotate_inverse(self.root_quat_w, self.root_ang_vel_w))
    projected_gravity_b = property(lambda self: self._m.quat_rotate_inverse(self.root_quat_w, self.GRAVITY_VEC_W))


class _Scene(dict):
    pass


class StubEnv:
    def __init__(self, math_mod):
        self.num_envs, self.device = N, "cpu"
        self.robot = types.SimpleNamespace(data=_RobotData(math_mod))
        self.ray = types.SimpleNamespace(data=types.SimpleNamespace())
        self.imu = types.SimpleNamespace(data=types.SimpleNamespace())
        self.scene = _Scene(robot=self.robot, imu=self.imu)
        self.scene.env_origins = torch.zeros(N, 3)
        self.scene.sensors = {"height_scanner": self.ray}
        self.action_manager = types.SimpleNamespace(action=torch.zeros(N, A))
        self._command = torch.zeros(N, 3)
        self.command_manager = types.SimpleNamespace(get_command=lambda name: self._command)

    def load(self, x: dict, s: int, reset: np.ndarray) -> None:
        t = lambda a: torch.from_numpy(np.ascontiguousarray(a))  # noqa: E731
        d = self.robot.data
        d.root_pos_w, d.root_quat_w = t(x["root_pos"][s].T), t(x["root_quat"][s].T)
        d.root_lin_vel_w, d.root_ang_vel_w = t(x["root_lin"][s].T), t(x["root_ang"][s].T)
        d.joint_pos, d.joint_vel = t(x["q"][s].T), t(x["qd"][s].T)
        self.ray.data.pos_w = t(x["ray_pose"][s][:3].T)
        self.ray.data.ray_hits_w = t(x["ray_hits"][s].transpose(2, 1, 0))
        im = x["imu"][s][:, 0]
        self.imu.data.quat_w, self.imu.data.ang_vel_b, self.imu.data.lin_acc_b = t(im[3:7].T), t(im[10:13].T), t(im[13:16].T)
        self._command = t(x["commands"][s][0].T)
        a = t(x["actions"][s]).clone()
        a[torch.from_numpy(reset.astype(bool))] = 0.0  # action_manager.reset(env_ids)
        self.action_manager.action = a


def build_group(ref, spec: dict):
    """The case's group as the reference's cfg objects (this project's cfg classes, the reference's functions)."""
    from allsteps_isaaclab_amd.utils.events import SceneEntityCfg
    from allsteps_isaaclab_amd.utils.observations import ObservationGroupCfg, ObservationTermCfg

    _, ob, nm, _, draws = ref
    group = ObservationGroupCfg(concatenate_terms=spec["concatenate_terms"],
                                enable_corruption=spec["enable_corruption"], history_length=spec["history_length"],
                                flatten_history_dim=spec["flatten_history_dim"])
    col = 0
    for t in spec["terms"]:
        p = dict(t["params"])
        params = {}
        if "joint_ids" in p:
            params["asset_cfg"] = SceneEntityCfg("robot", joint_ids=p.pop("joint_ids"))
        if "sensor" in p:
            params["sensor_cfg"] = SceneEntityCfg(p.pop("sensor"))
        if "imu" in p:
            params["asset_cfg"] = SceneEntityCfg(p.pop("imu"))
        params.update(p)
        noise = None
        if t["noise"] is not None:
            nz = t["noise"]
            val = lambda v: torch.tensor(v, dtype=torch.float32) if isinstance(v, list) else v  # noqa: E731
            names = {"constant": ("bias", None), "uniform": ("n_min", "n_max"), "gaussian": ("mean", "std")}[nz["kind"]]
            real = getattr(nm, nz["kind"] + "_noise")

            def func(data, cfg, _real=real, _col=col):
                draws.col = _col
                return _real(data, cfg)

            noise = types.SimpleNamespace(func=func, operation=nz["operation"])
            setattr(noise, names[0], val(nz["p0"]))
            if names[1]:
                setattr(noise, names[1], val(nz["p1"]))
        cfg = ObservationTermCfg(func=getattr(ob, t["func"]), params=params, noise=noise,
                                 clip=None if t["clip"] is None else tuple(t["clip"]),
                                 scale=tuple(t["scale"]) if isinstance(t["scale"], (list, tuple)) else t["scale"],
                                 history_length=t["history_length"], flatten_history_dim=t["flatten_history_dim"])
        setattr(group, t["name"], cfg)
        col += _WIDTH[t["func"]](params)
    return group, col


_WIDTH = {"base_pos_z": lambda p: 1, "base_lin_vel": lambda p: 3, "base_ang_vel": lambda p: 3,
          "projected_gravity": lambda p: 3, "root_pos_w": lambda p: 3, "root_quat_w": lambda p: 4,
          "root_lin_vel_w": lambda p: 3, "root_ang_vel_w": lambda p: 3, "generated_commands": lambda p: 3,
          "last_action": lambda p: A, "height_scan": lambda p: R, "imu_orientation": lambda p: 4,
          "imu_ang_vel": lambda p: 3, "imu_lin_acc": lambda p: 3}
for _k in ("joint_pos", "joint_pos_rel", "joint_pos_limit_normalized", "joint_vel", "joint_vel_rel"):
    _WIDTH[_k] = lambda p: len(p["asset_cfg"].joint_ids) if "asset_cfg" in p else J


def run_case(ref, spec: dict, x: dict, draws_arr: np.ndarray) -> np.ndarray:
    om, _, _, math_mod, draws = ref
    env = StubEnv(math_mod)
    env.load(x, 0, np.zeros(N, np.uint8))
    draws.step = draws_arr[0]
    group, d0 = build_group(ref, spec)
    assert d0 == draws_arr.shape[1], (d0, draws_arr.shape)
    mgr = om.ObservationManager({spec["name"]: group}, env)  # (_prepare_terms calls every function once)
    outs = []
    for s in range(spec["steps"]):
        reset = spec["reset"][s]
        env.load(x, s, reset)
        draws.step = draws_arr[s]
        ids = np.nonzero(reset)[0]
        if len(ids):
            mgr.reset(torch.from_numpy(ids))
        res = mgr.compute()[spec["name"]]
        if isinstance(res, dict):
            res = torch.cat([v.reshape(N, -1) for v in res.values()], dim=-1)
        outs.append(res.numpy().astype(np.float32).copy())
    return np.stack(outs)


def generate(reference: str) -> dict:
    ref = load_reference(reference)
    verified = verify_stub_formulas(ref)
    rng = np.random.default_rng(20261021)
    inputs = {"a": make_inputs(rng, 12, False), "c": make_inputs(rng, 3, True)}
    specs = case_specs()
    out = {}
    for key, x in inputs.items():
        for k, v in x.items():
            out[f"in_{key}_{k}"] = v
    d0 = {}
    for spec in specs:
        name = spec["name"]
        if spec["inputs"] == name or name == "d":
            _, cols = build_group(ref, spec)
            u = _uniform12(rng, (len(inputs[spec["inputs"]]["q"]), cols, N))
            z = _q8(rng.normal(0.0, 1.0, u.shape))
            c = 0
            for t in spec["terms"]:  # unit normals where the term's noise is gaussian
                params = dict(t["params"])
                if "joint_ids" in params:
                    params["asset_cfg"] = types.SimpleNamespace(joint_ids=params["joint_ids"])
                w = _WIDTH[t["func"]](params)
                if t["noise"] is not None and t["noise"]["kind"] == "gaussian":
                    u[:, c:c + w] = z[:, c:c + w]
                c += w
            d0[name] = u
            out[f"{name}_draws"] = u
        draws_arr = d0[name] if name in d0 else d0[spec["inputs"]]
        out[f"{name}_out"] = run_case(ref, spec, inputs[spec["inputs"]], draws_arr)
        out[f"{name}_reset"] = np.stack(spec["reset"])
    meta = {"n": N, "joints": J, "actions": A, "rays": R, "verified": verified,
            "cases": [{k: v for k, v in s.items() if k != "reset"} | {"draws": s["name"] if s["name"] in d0 else s["inputs"]}
                      for s in specs]}
    out["meta"] = np.frombuffer(json.dumps(meta, sort_keys=True).encode(), np.uint8)
    out["default_joint_pos"], out["default_joint_vel"], out["soft_joint_pos_limits"] = DEFAULT_Q, DEFAULT_QD, LIMITS
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=DEFAULT_REFERENCE)
    ap.add_argument("--check", action="store_true")
    args = ap.parse_args()
    torch.set_num_threads(1)
    arrays = generate(args.reference)
    buf = io.BytesIO()
    np.savez_compressed(buf, **arrays)
    data = buf.getvalue()
    if args.check:
        with open(OUT, "rb") as f:
            same = f.read() == data
        print("observations.npz:", "identical" if same else "DIFFERS")
        sys.exit(0 if same else 1)
    with open(OUT, "wb") as f:
        f.write(data)
    print(f"wrote {OUT}: {len(data)} bytes, {len(arrays)} arrays")


if __name__ == "__main__":
    main()
