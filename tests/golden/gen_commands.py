"""Generate tests/golden/commands.npz from the reference's own command code.

Loads ``isaaclab/managers/command_manager.py`` and ``isaaclab/envs/mdp/commands/velocity_command.py`` of a
reference checkout BY PATH, with stub modules of this file's own for the Isaac / Omniverse packages they import and
the reference's real ``isaaclab/utils/math.py``, builds ``UniformVelocityCommand`` / ``NormalVelocityCommand`` terms
without Isaac and drives them through the reference's ``CommandManager.reset(env_ids)`` and
``CommandManager.compute(dt)`` on the CPU, in the order of ``ManagerBasedRLEnv.step``: the reset of the step's done
envs, then compute.  The robot is a stub whose ``root_lin_vel_b`` / ``root_ang_vel_b`` / ``heading_w`` are the
expressions of articulation_data.py:518-526, 604-619 over the reference's ``quat_rotate_inverse`` / ``quat_apply``.

The draws are replaced by recorded ones, held per (step, phase, term, slot, env) -- phase 0 the reset's resample,
phase 1 the compute's -- and handed out for the envs that resample:

  ``time_left[env_ids].uniform_(lo, hi)``       slot 0 (``time_left`` is wrapped so that the draw is caught)
  ``torch.empty(k).uniform_(lo, hi)``           fma(d, float32(hi) - float32(lo), float32(lo))
  ``torch.empty(k).normal_(mean, std)``         fma(z, float32(std), float32(mean)), z a recorded unit normal

-- one fused multiply-add, rounded once: torch's kernels are compiled with the multiply and the add of these two
fills contracted (the CPU's vector loops, and nvcc's default for the CUDA ones), which ``verify_stub_formulas``
establishes against real torch on a seeded CPU generator: the fused form reproduces ``uniform_`` bit for bit at
every length and ``normal_`` for tensors of 16 elements and more, and the separately rounded form does not.
(``normal_`` on fewer than 16 elements takes a scalar path in double; the fixture's n is 66, but a term that
resamples fewer than 16 envs at once would take it in the reference.  The kernel serves the fused float32 form
for every env.)  The slots of a term's calls, in the reference's call order:

  uniform term, heading_command    0 time | 1 x | 2 y | 3 yaw | 4 heading | 5 is_heading | 6 is_standing
  uniform term, no heading         0 time | 1 x | 2 y | 3 yaw | 6 is_standing
  normal term                      0 time | 1 x, 4 its sign | 2 y, 5 its sign | 3 yaw, 6 its sign | 7 8 9 the zero
                                   tests | 10 is_standing

Cases (n = 66, dt = 4/240; every array in the kernel's field-major / env-minor layout):

  a   two uniform terms over 60 steps: one with heading_command, rel_heading_envs = 0.6, rel_standing_envs = 0.15,
      one without; ranges that are Python floats and not float32 values; random tilted root quaternions and root
      velocities that change every step; a reset mask every few steps, with one reset env forced to time out in the
      step of its reset (a double resample)
  b   a normal term with zero probabilities, 30 steps, resets
  c   one step from hand-set timers that straddle ``time_left <= 0``: exactly dt, one ulp either side
  d   heading errors at and around +-pi and odd multiples (on quaternions whose forward vector is exactly (-1, +0)
      or (1, 0), so that atan2 is exact), forward vectors near the axes, resampling_time_range = (0, 0): every env
      resamples every step.  (A NullCommandCfg-like infinite range is refused by the env's host code and is not a
      fixture case: the reference's own uniform_ gives NaN timers for it.)

Every case starts from the state a reset of every env leaves (``<case>_init_draws``), recorded as ``<case>_*0``.

    python tests/golden/gen_commands.py [--reference DIR] [--check]

--check regenerates into memory and compares with the committed file byte for byte.
"""

from __future__ import annotations

import argparse
import importlib.util
import io
import json
import math
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "commands.npz")
DEFAULT_REFERENCE = os.environ.get("ALLSTEPS_REFERENCE", "/root/reference")
PKG = os.path.join("source", "isaaclab", "isaaclab")
N = 66
DT = 4 / 240
SLOTS = 11
SLOT_ORDER = {"uniform_heading": (0, 1, 2, 3, 4, 5, 6), "uniform": (0, 1, 2, 3, 6),
              "normal": (0, 1, 4, 2, 5, 3, 6, 7, 8, 9, 10)}


class _Any:
    def __init__(self, *a, **k):
        pass

    def __getattr__(self, name):
        return _Any()

    def __call__(self, *a, **k):
        return _Any()


class _ManagerTermBase:
    def __init__(self, cfg, env):
        self.cfg, self._env = cfg, env

    num_envs = property(lambda self: self._env.num_envs)
    device = property(lambda self: self._env.device)


class _ManagerBase:
    pass


def _f32(x):
    return torch.tensor(float(x), dtype=torch.float32)


def fma32(a, b, c) -> np.ndarray:
    """fmaf(a, b, c) elementwise on float32 values: the product is exact in double; where the double sum lands on
    the midpoint of two float32 values its own rounding may have put it there, and the element is redone in
    rationals."""
    from fractions import Fraction

    a, b, c = np.broadcast_arrays(np.asarray(a, np.float32), np.asarray(b, np.float32), np.asarray(c, np.float32))
    r64 = a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)
    out = r64.astype(np.float32)
    tie = (r64.view(np.uint64) & np.uint64(0x1FFFFFFF)) == np.uint64(0x10000000)
    for i in zip(*np.nonzero(tie)):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        lo, hi = sorted((np.nextafter(out[i], np.float32(-np.inf)), np.nextafter(out[i], np.float32(np.inf))))
        out[i] = min((lo, out[i], hi), key=lambda v: (abs(Fraction(float(v)) - exact), int(v.view(np.uint32)) & 1))
    return out


def _fma(d: torch.Tensor, w, lo) -> torch.Tensor:
    return torch.from_numpy(fma32(d.numpy(), w.numpy(), lo.numpy()))


class _Ctx:
    """Which draws the next calls consume: set by the driver (step arrays, phase) and by the reference's own
    ``time_left[env_ids]`` (term, envs)."""

    def __init__(self):
        self.draws = None      # (2, K, SLOTS, N) of the current step
        self.resampled = None  # (2, K, N) uint8, written
        self.phase = 0
        self.term = self.ids = self.order = None
        self.call = 0

    def begin(self, term_index, kind, ids):
        self.term, self.order, self.call = term_index, SLOT_ORDER[kind], 0
        self.ids = torch.arange(N)[ids] if isinstance(ids, slice) else torch.as_tensor(ids).long()
        self.resampled[self.phase, term_index, self.ids.numpy()] = 1

    def next(self, k):
        assert k == len(self.ids), (k, len(self.ids))
        slot = self.order[self.call]
        self.call += 1
        return torch.from_numpy(self.draws[self.phase, self.term, slot])[self.ids]


class _Draw:
    """Stands in for ``torch.empty(k)`` and for ``time_left[env_ids]``: uniform_ / normal_ from recorded draws."""

    def __init__(self, ctx, k):
        self._ctx, self._k = ctx, k

    def uniform_(self, lo, hi):
        return _fma(self._ctx.next(self._k), _f32(hi) - _f32(lo), _f32(lo))

    def normal_(self, mean=0.0, std=1.0):
        return _fma(self._ctx.next(self._k), _f32(std), _f32(mean))


class _TimeLeft:
    """The ``time_left`` of a term: the four uses CommandTerm makes of it (command_manager.py:160-183), with the
    indexed read handing out the recorded time draw."""

    def __init__(self, ctx, term_index, kind):
        self.t = torch.zeros(N)
        self._ctx, self._term, self._kind = ctx, term_index, kind

    def __getitem__(self, ids):
        self._ctx.begin(self._term, self._kind, ids)
        return _Draw(self._ctx, len(self._ctx.ids))

    def __setitem__(self, ids, value):
        self.t[ids] = value

    def __isub__(self, dt):
        self.t -= dt
        return self

    def __le__(self, x):
        return self.t <= x


class _Torch:
    """Stands in for velocity_command's ``torch``: ``empty`` hands out the recorded draws."""

    def __init__(self, ctx):
        self._ctx = ctx

    def __getattr__(self, name):
        return getattr(torch, name)

    def empty(self, k, device=None):
        return _Draw(self._ctx, k)


class _RobotData:
    """articulation_data.py:518-526, 604-619 over the reference's math."""

    FORWARD_VEC_B = torch.tensor([[1.0, 0.0, 0.0]]).repeat(N, 1)

    def __init__(self, math_mod):
        self._m = math_mod
        self.root_quat_w = self.root_lin_vel_w = self.root_ang_vel_w = None

    @property
    def root_lin_vel_b(self):
        return self._m.quat_rotate_inverse(self.root_quat_w, self.root_lin_vel_w)

    @property
    def root_ang_vel_b(self):
        return self._m.quat_rotate_inverse(self.root_quat_w, self.root_ang_vel_w)

    @property
    def heading_w(self):
        forward_w = self._m.quat_apply(self.root_quat_w, self.FORWARD_VEC_B)
        return torch.atan2(forward_w[:, 1], forward_w[:, 0])


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
    """(command_manager module, velocity_command module, math module, ctx) of the reference at ``root``."""
    pkg = os.path.join(root, PKG)
    for name in ("omni", "omni.kit", "carb", "isaaclab", "isaaclab.utils", "isaaclab.envs", "isaaclab.envs.mdp",
                 "isaaclab.envs.mdp.commands"):
        _mod(name)
    _mod("omni.log", warn=lambda *a, **k: None)
    _mod("omni.kit.app", get_app_interface=_Any())
    _mod("prettytable", PrettyTable=_Any)
    _mod("isaaclab.assets", Articulation=_Any)
    _mod("isaaclab.markers", VisualizationMarkers=_Any)
    term_cfg = type("CommandTermCfg", (), {})
    _mod("isaaclab.managers")
    _mod("isaaclab.managers.manager_base", ManagerBase=_ManagerBase, ManagerTermBase=_ManagerTermBase)
    _mod("isaaclab.managers.manager_term_cfg", CommandTermCfg=term_cfg)
    math_mod = _load("isaaclab.utils.math", os.path.join(pkg, "utils", "math.py"), "isaaclab.utils")
    sys.modules["isaaclab.utils"].math = math_mod
    cm = _load("isaaclab.managers.command_manager", os.path.join(pkg, "managers", "command_manager.py"),
               "isaaclab.managers")
    sys.modules["isaaclab.managers"].CommandTerm = cm.CommandTerm
    vc = _load("isaaclab.envs.mdp.commands.velocity_command",
               os.path.join(pkg, "envs", "mdp", "commands", "velocity_command.py"), "isaaclab.envs.mdp.commands")
    ctx = _Ctx()
    vc.torch = _Torch(ctx)
    return cm, vc, math_mod, ctx


def verify_stub_formulas() -> dict:
    """The stub's uniform_ / normal_ against real torch on a seeded CPU generator: the raw draw is what
    uniform_(0, 1) / normal_(0, 1) give from the same generator state."""
    out = {}
    for k in (5, 66):  # torch fills short and long tensors by different loops
        for lo, hi in ((-0.3, 0.7), (0.11, 0.37), (-3.1, 3.1)):
            g = torch.Generator().manual_seed(1234)
            u = torch.empty(k).uniform_(0.0, 1.0, generator=g)
            g.manual_seed(1234)
            r = torch.empty(k).uniform_(lo, hi, generator=g)
            assert torch.equal(r, _fma(u, _f32(hi) - _f32(lo), _f32(lo))), ("uniform_", k, lo, hi)
            out["uniform_unfused_differs"] = out.get("uniform_unfused_differs", False) or \
                not torch.equal(r, u * (_f32(hi) - _f32(lo)) + _f32(lo))
        same = True
        for mean, std in ((0.5, 0.4), (-0.3, 0.6)):
            g = torch.Generator().manual_seed(1234)
            z = torch.empty(k).normal_(0.0, 1.0, generator=g)
            g.manual_seed(1234)
            r = torch.empty(k).normal_(mean, std, generator=g)
            same &= bool(torch.equal(r, _fma(z, _f32(std), _f32(mean))))
        out[f"normal_{k}"] = same
    assert out["normal_66"], "normal_ on 66 elements is not the fused float32 form"
    out["uniform"] = True
    return out


def _uniform24(rng, shape):
    return rng.integers(0, 1 << 24, shape).astype(np.float32) / np.float32(1 << 24)


def _cfg(term: dict):
    """A fixture term as the reference's cfg object (attribute access only)."""
    ranges = types.SimpleNamespace(**{k: (tuple(v) if v is not None else None) for k, v in term["ranges"].items()})
    ranges.heading = getattr(ranges, "heading", None)  # (read by the base constructor of the normal term too)
    return types.SimpleNamespace(
        resampling_time_range=tuple(term["resampling_time_range"]), debug_vis=False, asset_name="robot",
        heading_command=term.get("heading_command", False),
        heading_control_stiffness=term.get("heading_control_stiffness", 1.0),
        rel_standing_envs=term.get("rel_standing_envs", 0.0), rel_heading_envs=term.get("rel_heading_envs", 1.0),
        ranges=ranges)


def _kind(term: dict) -> str:
    return "normal" if term["kind"] == "normal" else "uniform_heading" if term.get("heading_command") else "uniform"


def _random_quat(rng, shape):
    q = rng.normal(0.0, 1.0, (*shape, 4))
    return (q / np.linalg.norm(q, axis=-1, keepdims=True)).astype(np.float32)


class Runner:
    """The reference's manager and terms of one case, and the recording of their state."""

    def __init__(self, ref, terms: list[dict]):
        cm, vc, math_mod, ctx = ref
        self.ctx, self.terms = ctx, terms
        self.data = _RobotData(math_mod)
        robot = types.SimpleNamespace(data=self.data, is_initialized=True)
        env = types.SimpleNamespace(num_envs=N, device="cpu", step_dt=DT, scene={"robot": robot})
        self.mgr = object.__new__(cm.CommandManager)
        self.mgr._terms = {}
        for k, t in enumerate(terms):
            cls = vc.NormalVelocityCommand if t["kind"] == "normal" else vc.UniformVelocityCommand
            term = cls(_cfg(t), env)
            term.time_left = _TimeLeft(ctx, k, _kind(t))
            self.mgr._terms[t["name"]] = term

    def set_root(self, quat, lin, ang):
        self.data.root_quat_w = torch.from_numpy(quat.copy())
        self.data.root_lin_vel_w = torch.from_numpy(lin.copy())
        self.data.root_ang_vel_w = torch.from_numpy(ang.copy())

    def state(self) -> dict:
        """The terms' state in the kernel's layouts: vel (K, 3, N), heading_target (K, N), flags (K, 5, N), time_left
        (K, N), counter (K, N), metrics (K, 2, N)."""
        ts = list(self.mgr._terms.values())
        flag = lambda t, name: getattr(t, name, torch.zeros(N, dtype=torch.bool)).numpy().astype(np.uint8)  # noqa: E731
        return {
            "vel": np.stack([t.vel_command_b.numpy().T for t in ts]).astype(np.float32),
            "heading_target": np.stack([t.heading_target.numpy() for t in ts]).astype(np.float32),
            "flags": np.stack([np.stack([flag(t, a) for a in ("is_heading_env", "is_standing_env", "is_zero_vel_x_env",
                                                              "is_zero_vel_y_env", "is_zero_vel_yaw_env")])
                               for t in ts]),
            "time_left": np.stack([t.time_left.t.numpy() for t in ts]).astype(np.float32),
            "counter": np.stack([t.command_counter.numpy() for t in ts]).astype(np.int32),
            "metrics": np.stack([np.stack([t.metrics["error_vel_xy"].numpy(), t.metrics["error_vel_yaw"].numpy()])
                                 for t in ts]).astype(np.float32),
        }

    def reset(self, ids, draws, resampled):
        """CommandManager.reset(env_ids) on recorded draws (K, SLOTS, N): phase 0."""
        self.ctx.draws, self.ctx.resampled, self.ctx.phase = draws[None], resampled[None], 0
        return self.mgr.reset(env_ids=torch.as_tensor(ids).long())

    def step(self, reset_mask, draws, resampled):
        """One env step: the reset of the masked envs (manager_based_rl_env.py:220-232 -> :347-380), then
        compute(dt) (:234)."""
        self.ctx.draws, self.ctx.resampled = draws, resampled
        ids = torch.from_numpy(reset_mask).nonzero().flatten()
        extras = {}
        if len(ids):
            self.ctx.phase = 0
            extras = self.mgr.reset(env_ids=ids)
        self.ctx.phase = 1
        self.mgr.compute(DT)
        return extras


def run_case(ref, arrays, name, terms, steps, rng, quat=None, reset=None, hook=None, draw_hook=None):
    """A reset of every env from recorded draws, then ``steps`` env steps; ``hook(runner)`` may edit the state
    after the reset, ``draw_hook(init_draws, draws)`` the draws before they are used."""
    K = len(terms)
    run = Runner(ref, terms)
    quat = _random_quat(rng, (steps, N)) if quat is None else quat
    lin = rng.normal(0.0, 0.7, (steps, N, 3)).astype(np.float32)
    ang = rng.normal(0.0, 0.9, (steps, N, 3)).astype(np.float32)
    reset = np.zeros((steps, N), np.uint8) if reset is None else reset
    draws = _uniform24(rng, (steps, 2, K, SLOTS, N))
    init_draws = _uniform24(rng, (K, SLOTS, N))
    for k, t in enumerate(terms):
        if t["kind"] == "normal":  # slots 1..3 are unit normals
            draws[:, :, k, 1:4] = rng.normal(0.0, 1.0, (steps, 2, 3, N)).astype(np.float32)
            init_draws[k, 1:4] = rng.normal(0.0, 1.0, (3, N)).astype(np.float32)
    if draw_hook is not None:
        draw_hook(init_draws, draws)
    run.set_root(quat[0], lin[0], ang[0])
    run.reset(np.arange(N), init_draws, np.zeros((K, N), np.uint8))
    if hook is not None:
        hook(run)
    for key, v in run.state().items():
        arrays[f"{name}_{key}0"] = v
    resampled = np.zeros((steps, 2, K, N), np.uint8)
    out = {key: [] for key in ("vel", "heading_target", "flags", "time_left", "counter", "metrics", "last_metrics")}
    last = np.zeros((K, 2, N), np.float32)
    for s in range(steps):
        run.set_root(quat[s], lin[s], ang[s])
        before = run.state()["metrics"]
        run.step(reset[s], draws[s], resampled[s])
        m = reset[s].astype(bool)
        last = last.copy()
        last[:, :, m] = before[:, :, m]  # what CommandTerm.reset averaged and zeroed, per env
        st = run.state()
        for key in st:
            out[key].append(st[key])
        out["last_metrics"].append(last)
    used = sorted({slot for t in terms for slot in SLOT_ORDER[_kind(t)]})
    arrays.update({f"{name}_{key}": np.stack(v) for key, v in out.items()})
    arrays.update({f"{name}_root_quat": np.ascontiguousarray(quat.transpose(0, 2, 1)),
                   f"{name}_root_lin": np.ascontiguousarray(lin.transpose(0, 2, 1)),
                   f"{name}_root_ang": np.ascontiguousarray(ang.transpose(0, 2, 1)),
                   f"{name}_reset": reset, f"{name}_resampled": resampled,
                   f"{name}_init_draws": np.ascontiguousarray(init_draws[:, used]),
                   # the compute phase's draws of every step; the reset phase's of the steps with a reset only
                   f"{name}_draws": np.ascontiguousarray(draws[:, 1][:, :, used]),
                   f"{name}_reset_steps": np.flatnonzero(reset.any(1)).astype(np.int32),
                   f"{name}_reset_draws": np.ascontiguousarray(draws[reset.any(1), 0][:, :, used])})
    return {"name": name, "dt": DT, "steps": steps, "terms": terms, "slots": used}


def _yaw_quat(yaw):
    return np.array([math.cos(yaw / 2), 0.0, 0.0, math.sin(yaw / 2)], np.float32)


def generate(reference: str) -> dict:
    ref = load_reference(reference)
    checks = verify_stub_formulas()
    rng = np.random.default_rng(20251021)
    arrays: dict[str, np.ndarray] = {}
    cases = []
    dt32 = np.float32(DT)

    # ---- a: two uniform terms, 60 steps; ranges that are not float32 values
    terms = [{"name": "base_velocity", "kind": "uniform", "resampling_time_range": [0.11, 0.37],
              "heading_command": True, "heading_control_stiffness": 0.7, "rel_heading_envs": 0.6,
              "rel_standing_envs": 0.15,
              "ranges": {"lin_vel_x": [-1.1, 1.3], "lin_vel_y": [-0.7, 0.9], "ang_vel_z": [-0.8, 0.9],
                         "heading": [-3.1, 3.1]}},
             {"name": "side_velocity", "kind": "uniform", "resampling_time_range": [0.01, 0.31],
              "rel_standing_envs": 0.1,
              "ranges": {"lin_vel_x": [0.1, 0.3], "lin_vel_y": [-0.07, 0.07], "ang_vel_z": [-0.9, -0.6]}}]
    steps = 60
    reset = np.zeros((steps, N), np.uint8)
    for s in range(3, steps, 5):
        reset[s, rng.choice(N, 7, replace=False)] = 1
    reset[13, 5] = reset[13, 40] = 1

    def force_double(init_draws, draws):  # envs 5 and 40 draw the shortest time in the reset of step 13:
        draws[13, 0, 1, 0, [5, 40]] = 0.0  # term 1's new time_left = 0.01 < dt, so compute resamples them again

    cases.append(run_case(ref, arrays, "a", terms, steps, rng, reset=reset, draw_hook=force_double))
    rs, fl, vel = arrays["a_resampled"], arrays["a_flags"], arrays["a_vel"]
    assert (rs.sum(axis=(0, 1)) >= 2).all(), "every env must resample at least twice in every term"
    assert fl[:, 0, 0].mean() >= 0.25 and fl[:, :, 1].mean(axis=(0, 2)).min() >= 0.05, "heading / standing coverage"
    assert reset.sum() >= 10 and (rs[:, 0] & rs[:, 1]).sum() >= 1, "resets and a double resample"
    assert rs[13, 0, 1, 5] and rs[13, 1, 1, 5]
    moving = (fl[:, 0, 0] == 1) & (fl[:, 0, 1] == 0)
    assert (vel[:, 0, 2][moving] == np.float32(0.9)).any() and (vel[:, 0, 2][moving] == np.float32(-0.8)).any(), \
        "both clip bounds of ang_vel_z must be hit"
    assert ((vel[:, 0, 2][moving] > np.float32(-0.8)) & (vel[:, 0, 2][moving] < np.float32(0.9))).any()

    # ---- b: a normal term with zero probabilities
    terms = [{"name": "base_velocity", "kind": "normal", "resampling_time_range": [0.05, 0.2], "rel_standing_envs": 0.1,
              "ranges": {"mean_vel": [0.5, 0.1, -0.3], "std_vel": [0.4, 0.25, 0.6], "zero_prob": [0.2, 0.3, 0.1]}}]
    steps = 30
    reset = np.zeros((steps, N), np.uint8)
    for s in range(2, steps, 4):
        reset[s, rng.choice(N, 5, replace=False)] = 1
    cases.append(run_case(ref, arrays, "b", terms, steps, rng, reset=reset))
    assert (arrays["b_resampled"].sum(axis=(0, 1)) >= 2).all()
    assert arrays["b_flags"][:, 0, 1:].reshape(steps, 4, N).any(axis=(0, 2)).all(), "every mask of the term is used"

    # ---- c: one step from hand-set timers around the resample test
    ulp = np.spacing(dt32)
    tl = [dt32, dt32 - ulp, dt32 + ulp, np.float32(0.0), -dt32, np.float32(2) * dt32, np.float32(1e-6),
          np.float32(DT / 2), np.float32(1.0)]
    tl += [dt32 + np.float32(m - 28) * ulp for m in range(N - len(tl))]
    tl = np.asarray(tl, np.float32)
    terms = [{"name": "base_velocity", "kind": "uniform", "resampling_time_range": [0.2, 0.5], "heading_command": True,
              "heading_control_stiffness": 0.5, "rel_heading_envs": 0.5, "rel_standing_envs": 0.1,
              "ranges": {"lin_vel_x": [-1.0, 1.0], "lin_vel_y": [-0.4, 0.6], "ang_vel_z": [-1.0, 1.0],
                         "heading": [-math.pi, math.pi]}}]

    def set_timers(run):
        run.mgr._terms["base_velocity"].time_left.t[:] = torch.from_numpy(tl)

    cases.append(run_case(ref, arrays, "c", terms, 1, rng, hook=set_timers))
    r = arrays["c_resampled"][0, 1, 0]
    assert r[0] and r[1] and not r[2] and r[3] and r[4] and not r[5] and 0 < r[9:].sum() < N - 9, \
        "the timers must straddle the test"

    # ---- d: heading errors at and around +-pi, forward vectors near the axes, resampling every step
    terms = [{"name": "base_velocity", "kind": "uniform", "resampling_time_range": [0.0, 0.0], "heading_command": True,
              "heading_control_stiffness": 0.5, "rel_heading_envs": 1.0, "rel_standing_envs": 0.0,
              "ranges": {"lin_vel_x": [-1.0, 1.0], "lin_vel_y": [-1.0, 1.0], "ang_vel_z": [-2.0, 2.0],
                         "heading": [-2 * math.pi, 2 * math.pi]}}]
    steps = 3
    quat = _random_quat(rng, (steps, N))
    back, front = np.array([0, 0, 0, 1], np.float32), np.array([1, 0, 0, 0], np.float32)
    quat[:, 0:4] = back   # forward = (-1, +0) exactly: heading_w = pi in any atan2
    # forward = (-1, -2e-30): quat_apply cannot give y = -0 (its last sum has a +0 term), so the heading of -pi
    # comes from a y far below an ulp of pi: heading_w = -pi in any atan2 that is accurate to an ulp
    quat[:, 4:8] = np.array([1e-30, 0, 0, -1], np.float32)
    quat[:, 8:16] = front  # forward = (1, 0) exactly: heading_w = 0
    eps = [0.0, 1e-7, -1e-7, 1e-4, -1e-4, 3e-3, -3e-3, 1e-9]
    for j, axis in enumerate((0.0, math.pi / 2, math.pi, -math.pi / 2)):  # forward vectors near the four axes
        for i, e in enumerate(eps):
            quat[:, 16 + 8 * j + i] = _yaw_quat(axis + e)
    # heading_target = d 4 pi - 2 pi: d = 0, 1/4, 1/2, 3/4 give -2 pi, -pi, 0, pi; neighbours one draw step away
    grid = np.array([0.0, 0.25, 0.5, 0.75, 0.25 + 2.0 ** -24, 0.25 - 2.0 ** -24, 0.75 + 2.0 ** -24, 0.75 - 2.0 ** -24],
                    np.float32)

    def heading_draws(init_draws, draws):
        for s in range(steps):
            draws[s, 1, 0, 4, 0:8] = np.roll(grid, s)
            draws[s, 1, 0, 4, 8:16] = np.roll(grid, s)

    cases.append(run_case(ref, arrays, "d", terms, steps, rng, quat=quat, draw_hook=heading_draws))
    assert arrays["d_resampled"][:, 1].all(), "every env resamples in every step"
    pi32 = np.float32(math.pi)
    w = arrays["d_vel"][:, 0, 2]
    assert (w == np.float32(0.5) * pi32).any() and (w == np.float32(0.5) * -pi32).any(), "the wrap's +-pi ends are hit"
    assert np.isinf(arrays["d_metrics"]).all(), "max_command_step = 0: the reference's metrics are infinite"

    arrays["cases"] = np.array(json.dumps(cases))
    arrays["stub_checks"] = np.array(json.dumps(checks))
    return arrays


def serialise(arrays: dict) -> bytes:
    buf = io.BytesIO()
    np.savez_compressed(buf, **{k: arrays[k] for k in sorted(arrays)})
    return buf.getvalue()


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--reference", default=DEFAULT_REFERENCE, help="root of a reference checkout")
    ap.add_argument("--check", action="store_true", help="compare with the committed file instead of writing it")
    a = ap.parse_args(argv)
    arrays = generate(a.reference)
    print("stub formulas against torch:", str(arrays["stub_checks"]))
    data = serialise(arrays)
    if a.check:
        same = os.path.exists(OUT) and open(OUT, "rb").read() == data
        print(f"commands.npz: {'identical' if same else 'DIFFERS'} ({len(data)} bytes)")
        return 0 if same else 1
    with open(OUT, "wb") as f:
        f.write(data)
    print(f"wrote {OUT} ({len(data)} bytes)")
    return 0


if __name__ == "__main__":
    sys.exit(main())
