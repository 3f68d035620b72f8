"""Device state of an env's termination manager (``cfg.terminations``) and the ``env.termination_manager`` view of it.

``DirectRLEnv`` builds an :class:`EnvTerminations` once the subclass has its device state and launches
``as_terminations_step`` in ``step`` directly after the step and its in-kernel reset -- after the once-per-step
``as_contact_forces`` where a term reads the net forces -- and before the contact timers, the commands, the interval
events, the rewards and the observation manager: the reference's order, terminations first
(csrc/termination_kernels.h; semantics: csrc/allsteps_terminations.h).  Everything the kernel reads and writes -- the
term descriptors, the index table, the term flags, time_outs / terminated / dones, the flags of the last episode and
the reset request -- lives in fixed device tensors, so a step captured in a HIP graph replays, and ``set_term_cfg``
takes effect in a graph that is already captured.
"""

from __future__ import annotations

from dataclasses import dataclass, field
from functools import partial

import numpy as np
import torch

from .. import _native
from ..utils import terminations as TM
from . import _manager as M
from ._manager import SensorInfo, u8  # noqa: F401  (SensorInfo: re-exported)

_KIND = {name: k for k, name in enumerate(_native.TERMINATION_KINDS)}
_FUNCS = {getattr(TM, name): name for name in TM.SERVED}
_REFUSED = {getattr(TM, name): name for name in TM.REFUSED}


def _unsupported(term: str | None, detail: str) -> "_native.NativeError":
    where = "cfg.terminations" + ("" if term is None else f" term {term!r}")
    return _native.NativeError(f"{where}: {detail}.  The terminations are computed in a HIP kernel (no host fallback); "
                               f"supported: {TM.SUPPORTED}")


@dataclass
class TermContext:
    """What the terms of an env can read -- the host facts the parser checks a cfg against (no device needed)."""

    joint_names: list
    soft_joint_pos_limits: np.ndarray  # (joints, 2) float32
    step_dt: float
    max_episode_length: int
    command_names: list = field(default_factory=list)
    sensors: dict = field(default_factory=dict)  # name -> SensorInfo
    contact_forces: bool = False  # the contact report (cfg.contact_forces): the net forces


@dataclass
class TermSpec:
    """One parsed term: what the descriptor row and the index table's row are made from."""

    name: str
    cfg: object
    kind: int
    time_out: bool
    ids: list
    a: np.ndarray
    b: np.ndarray
    row: int = 0
    p0: np.float32 = np.float32(0.0)
    p1: np.float32 = np.float32(0.0)
    i0: int = 0


_params = partial(M.check_params, _unsupported)
_number = partial(M.number, _unsupported)
_robot_asset = partial(M.robot_asset, _unsupported)
_sensor_bodies = partial(M.sensor_bodies, _unsupported)


def _joints(params: dict, ctx: TermContext, t: str) -> list:
    return M.joint_ids(_unsupported, _robot_asset(params, t), ctx.joint_names, t)


def parse_term(t: str, cfg, ctx: TermContext) -> TermSpec:
    f32 = np.float32
    if not isinstance(cfg, TM.TerminationTermCfg):
        raise TypeError(f"Configuration for the term '{t}' is not of type TerminationTermCfg. Received: "
                        f"'{type(cfg)}'.")
    func = cfg.func
    name = getattr(func, "__name__", repr(func))
    if func is TM.MISSING or not callable(func):
        raise _unsupported(t, f"func = {func!r} is not callable")
    if not isinstance(cfg.params, dict):
        raise _unsupported(t, f"params = {cfg.params!r} is not a dict")
    if not isinstance(cfg.time_out, (bool, np.bool_)):
        raise _unsupported(t, f"time_out = {cfg.time_out!r} is not a bool")
    p = cfg.params
    if func in _REFUSED or name in TM.REFUSED:
        raise _unsupported(t, f"{name}: {TM.REFUSED[name]}")
    if isinstance(func, type) or (func not in _FUNCS and hasattr(func, "reset")):
        raise _unsupported(t, f"func = {name!r} is a class-based term (a ManagerTermBase); the kernel serves the "
                              f"term functions only")
    if func not in _FUNCS:
        raise _unsupported(t, f"func = {name!r} is not a served term function")
    kname = _FUNCS[func]
    z = np.zeros(0, f32)
    spec = TermSpec(t, cfg, _KIND[kname], bool(cfg.time_out), [], z, z)
    if kname == "time_out":
        _params(p, (), (), t)
        spec.i0 = int(ctx.max_episode_length)
    elif kname == "command_resample":
        _params(p, ("command_name",), ("num_resamples",), t)
        if not ctx.command_names:
            raise _unsupported(t, "the term reads a command term, and the env has no command manager: set "
                                  "cfg.commands")
        if p["command_name"] not in ctx.command_names:
            raise _unsupported(t, f"command_name = {p['command_name']!r} names no command term of cfg.commands "
                                  f"({ctx.command_names})")
        k = p.get("num_resamples", 1)
        if not isinstance(k, (int, np.integer)) or isinstance(k, bool):
            raise _unsupported(t, f"num_resamples = {k!r} is not an int")
        spec.row, spec.i0 = ctx.command_names.index(p["command_name"]), int(k)
        spec.p0 = f32(ctx.step_dt)
    elif kname == "bad_orientation":
        _params(p, ("limit_angle",), ("asset_cfg",), t)
        _robot_asset(p, t)
        spec.p0 = _number(p["limit_angle"], "limit_angle", t)
    elif kname == "root_height_below_minimum":
        _params(p, ("minimum_height",), ("asset_cfg",), t)
        _robot_asset(p, t)
        spec.p0 = _number(p["minimum_height"], "minimum_height", t)
    elif kname == "joint_pos_out_of_limit":
        _params(p, (), ("asset_cfg",), t)
        spec.ids = _joints(p, ctx, t)
        lim = np.asarray(ctx.soft_joint_pos_limits, f32)
        spec.a, spec.b = lim[spec.ids, 0], lim[spec.ids, 1]
    elif kname == "joint_pos_out_of_manual_limit":
        _params(p, ("bounds",), ("asset_cfg",), t)
        b = p["bounds"]
        if not isinstance(b, (tuple, list)) or len(b) != 2:
            raise _unsupported(t, f"bounds = {b!r} is not a (lower, upper) pair")
        spec.ids = _joints(p, ctx, t)
        spec.p0, spec.p1 = _number(b[0], "bounds[0]", t), _number(b[1], "bounds[1]", t)
    elif kname == "joint_vel_out_of_manual_limit":
        _params(p, ("max_velocity",), ("asset_cfg",), t)
        spec.ids = _joints(p, ctx, t)
        spec.p0 = _number(p["max_velocity"], "max_velocity", t)
    else:  # illegal_contact
        _params(p, ("threshold", "sensor_cfg"), (), t)
        spec.ids = _sensor_bodies(p, ctx, t)
        spec.p0 = _number(p["threshold"], "threshold", t)
    if len(spec.ids) > _native.MAX_TERMINATION_IDS:
        raise _unsupported(t, f"the term selects {len(spec.ids)} joints or bodies; the index table holds "
                              f"AS_MAX_TERMINATION_IDS = {_native.MAX_TERMINATION_IDS}")
    return spec


class TerminationTerms(M.TermTable):
    """The host side of cfg.terminations: the terms in cfg order, checked (no device needed), and the device tables
    as host arrays."""

    NOUN, TERM_TYPE, KINDS = "Termination", TM.TerminationTermCfg, _native.TERMINATION_KINDS
    WORDS = _native.TERMINATION_TERM_WORDS
    TABLE = (_native.TERMINATION_TABLE_ROWS, _native.MAX_TERMINATION_TERMS, _native.MAX_TERMINATION_IDS)
    LIMIT, COLUMN, MAY_CHANGE = "AS_MAX_TERMINATION_TERMS", ("Time Out", str.center), "params and time_out"
    parse_term, unsupported = staticmethod(parse_term), staticmethod(_unsupported)

    def pack(self, row, ints, t: TermSpec) -> None:
        ints[0], ints[1], ints[2], ints[3] = t.kind, int(t.time_out), len(t.ids), t.row
        row[4], row[5], ints[6] = t.p0, t.p1, t.i0

    def column(self, t: TermSpec) -> str:
        return str(bool(t.cfg.time_out))


class EnvTerminations(M.DeviceState):
    """The terminations side of a DirectRLEnv: the device tables and the manager's buffers."""

    STATE_PREFIX = "termination_"

    def __init__(self, cfg, env, n: int, device):
        self.n, self.device = n, device
        self._env = env
        self.spec = TerminationTerms(cfg.terminations, env._terminations_context())
        self.reset_envs = bool(getattr(cfg, "terminations_reset", False))
        T = len(self.spec.terms)
        z = lambda *shape: torch.zeros(*shape, dtype=torch.uint8, device=device)  # noqa: E731
        self.desc = torch.as_tensor(self.spec.rows.copy(), device=device)
        self.table = torch.as_tensor(self.spec.table.copy(), device=device)
        self.term_dones = z(T, n)
        self.time_outs, self.terminated, self.dones = z(n), z(n), z(n)
        self.last_episode_dones = z(T, n)
        self.reset_request = z(n)
        if self.reset_envs:  # the masked reset's observation rows, and the flags the step then returns
            self.reset_obs = torch.zeros(n, int(cfg.observation_space), dtype=torch.float32, device=device)
            self.step_terminated = torch.zeros(n, dtype=torch.bool, device=device)
            self.step_truncated = torch.zeros(n, dtype=torch.bool, device=device)
        self.launches = 0

    @staticmethod
    def wanted(cfg) -> bool:
        return getattr(cfg, "terminations", None) is not None

    # ---- launches
    def compute(self, terminated=None, truncated=None) -> torch.Tensor:
        """One launch: every term on the env's state as it stands.  terminated / truncated: the step's own flags
        ((n,) bool / uint8; None: no env was reset by the step).  Returns dones (n,) uint8."""
        env, spec = self._env, self.spec
        tensors = env._terminations_sources(net=spec.uses("illegal_contact"))
        tensors["step_terminated"], tensors["step_truncated"] = u8(terminated), u8(truncated)
        src = _native.make_termination_sources(tensors, env.physics_dt)
        _native.terminations_step(self.desc, self.table, spec.kinds, src, self.term_dones, self.time_outs,
                                  self.terminated, self.dones, self.last_episode_dones, self.reset_request,
                                  stream=env._noise_stream())
        self.launches += 1
        return self.dones

    def apply(self, out: tuple) -> tuple:
        """The manager's part of ``step``: the launch on the step's result ``out``; with cfg.terminations_reset also
        the masked reset of the envs the manager ends, whose observation rows and flags join the step's."""
        self.compute(out[2], out[3])
        if not self.reset_envs:
            return out
        env = self._env
        env._terminations_reset_mask(self.reset_request, self.reset_obs)
        policy = torch.where(self.reset_request.bool().unsqueeze(1), self.reset_obs, out[0]["policy"])
        torch.logical_or(out[2], self.terminated.bool(), out=self.step_terminated)
        torch.logical_or(out[3], self.time_outs.bool(), out=self.step_truncated)
        obs = dict(out[0], policy=policy)
        env.obs_buf = obs
        return (obs, out[1], self.step_terminated, self.step_truncated, *out[4:])

    def set_term_cfg(self, term_name: str, cfg) -> None:
        self.spec.replace(term_name, cfg, self.desc, self.table)

    # ---- state (get_state / set_state of the envs)
    def tensors(self) -> dict:
        return {"termination_term_dones": self.term_dones, "termination_time_outs": self.time_outs,
                "termination_terminated": self.terminated, "termination_dones": self.dones,
                "termination_last_episode_dones": self.last_episode_dones,
                "termination_reset_request": self.reset_request}


class TerminationManagerView:
    """``env.termination_manager``: the caller-visible surface of the reference's ``TerminationManager``
    (termination_manager.py:22-267) over the device state.  The flags are bool views of the kernel's bytes."""

    def __init__(self, term: EnvTerminations):
        self._t = term

    active_terms = property(lambda self: list(self._t.spec.names))
    dones = property(lambda self: self._t.dones.view(torch.bool))
    time_outs = property(lambda self: self._t.time_outs.view(torch.bool))
    terminated = property(lambda self: self._t.terminated.view(torch.bool))
    reset_request = property(lambda self: self._t.reset_request.view(torch.bool))

    @property
    def _term_dones(self) -> dict:
        """{term: (N,) bool view} of the terms' flags of the last launch."""
        return {name: self._t.term_dones[k].view(torch.bool) for k, name in enumerate(self._t.spec.names)}

    @property
    def last_episode_dones(self) -> dict:
        """{term: (N,) bool view} the terms' flags in the step that last ended the env's episode -- what the
        reference's reset counts, as a captured step serves it."""
        return {name: self._t.last_episode_dones[k].view(torch.bool) for k, name in enumerate(self._t.spec.names)}

    def compute(self) -> torch.Tensor:
        """TerminationManager.compute() on the env's state as it stands: one launch; no env counts as reset by the
        step, so time_out is the episode-length comparison alone."""
        return self._t.compute().view(torch.bool)

    def get_term(self, name: str) -> torch.Tensor:
        return self._t.term_dones[self._t.spec.index(name)].view(torch.bool)

    def reset(self, env_ids=None) -> dict:
        """TerminationManager.reset(env_ids): ``Episode_Termination/<term>`` = the number of ``env_ids`` whose flag
        of the term is set (a host read; by hand only -- the step does not call it)."""
        t = self._t
        sel = slice(None) if env_ids is None else torch.as_tensor(env_ids, device=t.device).long()
        return {f"Episode_Termination/{name}": torch.count_nonzero(t.term_dones[k][sel]).item()
                for k, name in enumerate(t.spec.names)}

    def set_term_cfg(self, term_name: str, cfg) -> None:
        """Replace a term's cfg.  The new descriptor is written into device memory in place, so it holds from the
        next launch on, in a captured graph too; a cfg with another term function is refused."""
        self._t.set_term_cfg(term_name, cfg)

    def get_term_cfg(self, term_name: str):
        return self._t.spec.terms[self._t.spec.index(term_name)].cfg

    def get_active_iterable_terms(self, env_idx: int) -> list:
        flags = self._t.term_dones[:, env_idx].float().cpu()
        return [(name, [flags[k].item()]) for k, name in enumerate(self._t.spec.names)]

    def __str__(self) -> str:
        return self._t.spec.table_str()
