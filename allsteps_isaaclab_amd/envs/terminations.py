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

import numpy as np
import torch

from .. import _native
from ..utils import terminations as TM
from ..utils.observations import resolve_joint_ids
from ..utils.rewards import resolve_body_ids

_KIND = {name: k for k, name in enumerate(_native.TERMINATION_KINDS)}
_FUNCS = {getattr(TM, name): name for name in TM.SERVED}
_REFUSED = {getattr(TM, name): name for name in TM.REFUSED}
STATE_PREFIX = "termination_"


def _unsupported(term: str | None, detail: str) -> "_native.NativeError":
    where = "cfg.terminations" + ("" if term is None else f" term {term!r}")
    return _native.NativeError(f"{where}: {detail}.  The terminations are computed in a HIP kernel (no host fallback); "
                               f"supported: {TM.SUPPORTED}")


def _is_number(x) -> bool:
    return isinstance(x, (int, float, np.floating, np.integer)) and not isinstance(x, bool)


@dataclass
class SensorInfo:
    """A contact sensor as the terms address it: its bodies' names, and per body the row of the net forces."""

    body_names: list
    net_bodies: list  # body b of the sensor -> body row of the contact report's net impulses


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


def _params(params: dict, required: tuple, optional: tuple, t: str) -> None:
    extra = sorted(set(params) - set(required) - set(optional))
    if extra:
        raise _unsupported(t, f"params {extra} are not parameters of the term function (it takes "
                              f"{list(required + optional)})")
    missing = [k for k in required if k not in params]
    if missing:
        raise _unsupported(t, f"the term function needs params {missing}")


def _number(x, key: str, t: str) -> np.float32:
    """A Python scalar as torch takes it in an operation with a float32 tensor."""
    if not _is_number(x):
        raise _unsupported(t, f"{key} = {x!r} is not a number")
    return np.float32(x)


def _robot_asset(params: dict, t: str):
    asset = params.get("asset_cfg", None)
    if asset is None:
        return TM.SceneEntityCfg("robot")
    if not hasattr(asset, "name"):
        raise _unsupported(t, f"params['asset_cfg'] = {asset!r} is not a SceneEntityCfg")
    if asset.name != "robot":
        raise _unsupported(t, f"asset_cfg.name = {asset.name!r} is not 'robot' (the env's articulation)")
    return asset


def _joints(params: dict, ctx: TermContext, t: str) -> list:
    asset = _robot_asset(params, t)
    try:
        ids = resolve_joint_ids(asset, ctx.joint_names, "asset_cfg")
    except ValueError as e:
        raise _unsupported(t, str(e)) from None
    ids = list(range(len(ctx.joint_names))) if ids is None else ids
    if not ids:
        raise _unsupported(t, "asset_cfg selects no joint")
    return ids


def _sensor_bodies(params: dict, ctx: TermContext, t: str) -> list:
    """The rows of the net forces that sensor_cfg's bodies read."""
    if not ctx.contact_forces:
        raise _unsupported(t, "the term reads the contact sensors' net forces: set cfg.contact_forces")
    sensor = params.get("sensor_cfg", None)
    sname = getattr(sensor, "name", None)
    if sname not in ctx.sensors:
        raise _unsupported(t, f"sensor_cfg names the sensor {sname!r}; the env has the contact sensors "
                              f"{sorted(ctx.sensors)}")
    info = ctx.sensors[sname]
    try:
        ids = resolve_body_ids(sensor, info.body_names, "sensor_cfg")
    except ValueError as e:
        raise _unsupported(t, str(e)) from None
    ids = list(range(len(info.body_names))) if ids is None else ids
    if not ids:
        raise _unsupported(t, "sensor_cfg selects no body")
    return [int(info.net_bodies[k]) for k in ids]


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


def _items(obj) -> list:
    """(name, value) of a cfg object in cfg order: a dict, or an object's attributes, then its classes' attributes
    that are TerminationTermCfg (the reference's configclass turns those into instance fields)."""
    if isinstance(obj, dict):
        return list(obj.items())
    items = [(k, v) for k, v in vars(obj).items() if not k.startswith("_")]
    seen = {k for k, _ in items}
    for klass in reversed(type(obj).__mro__[:-1]):
        for k, v in vars(klass).items():
            if k not in seen and not k.startswith("_") and isinstance(v, TM.TerminationTermCfg):
                items.append((k, v))
                seen.add(k)
    return items


class TerminationTerms:
    """The host side of cfg.terminations: the terms in cfg order, checked (no device needed), and the device tables
    as host arrays."""

    def __init__(self, terminations, ctx: TermContext):
        self.ctx = ctx
        self.terms: list[TermSpec] = []
        for name, cfg in _items(terminations):
            if cfg is None:  # (as the reference's _prepare_terms)
                continue
            self.terms.append(parse_term(name, cfg, ctx))
        if not self.terms:
            raise _unsupported(None, "there are no terms")
        if len(self.terms) > _native.MAX_TERMINATION_TERMS:
            raise _unsupported(None, f"{len(self.terms)} terms; the termination kernel takes at most "
                                     f"AS_MAX_TERMINATION_TERMS = {_native.MAX_TERMINATION_TERMS}")
        self.build()

    names = property(lambda self: [t.name for t in self.terms])

    def build(self) -> None:
        """The descriptor rows, the index table and the kinds mask from the term specs as they stand."""
        f32, i32 = np.float32, np.int32
        rows = np.zeros((len(self.terms), _native.TERMINATION_TERM_WORDS), f32)
        table = np.zeros((_native.TERMINATION_TABLE_ROWS, _native.MAX_TERMINATION_TERMS, _native.MAX_TERMINATION_IDS),
                         f32)
        for k, t in enumerate(self.terms):
            ints = rows[k].view(i32)
            ints[0], ints[1], ints[2], ints[3] = t.kind, int(t.time_out), len(t.ids), t.row
            rows[k, 4], rows[k, 5], ints[6] = t.p0, t.p1, t.i0
            table[0, k, :len(t.ids)] = np.asarray(t.ids, i32).view(f32)
            table[1, k, :len(t.a)] = t.a
            table[2, k, :len(t.b)] = t.b
        self.rows, self.table = rows, table
        self.kinds = 0
        for t in self.terms:
            self.kinds |= 1 << t.kind

    def index(self, term_name: str) -> int:
        if term_name not in self.names:
            raise ValueError(f"Termination term '{term_name}' not found.")
        return self.names.index(term_name)

    def uses(self, *kinds: str) -> bool:
        return any(_native.TERMINATION_KINDS[t.kind] in kinds for t in self.terms)

    def table_str(self) -> str:
        """TerminationManager.__str__ in the reference's form."""
        rows = [(str(i), t.name, str(bool(t.cfg.time_out))) for i, t in enumerate(self.terms)]
        head = ("Index", "Name", "Time Out")
        w = [max(len(r[j]) for r in rows + [head]) for j in range(3)]
        line = "+" + "+".join("-" * (x + 2) for x in w) + "+\n"
        total = len(line) - 3
        fmt = lambda r: "| " + " | ".join((r[0].center(w[0]), r[1].ljust(w[1]), r[2].center(w[2]))) + " |\n"  # noqa: E731
        msg = f"<TerminationManager> contains {len(rows)} active terms.\n"
        msg += "+" + "-" * total + "+\n" + "|" + "Active Termination Terms".center(total) + "|\n"
        msg += line + "| " + " | ".join(h.center(x) for h, x in zip(head, w)) + " |\n" + line
        return msg + "".join(fmt(r) for r in rows) + line


class EnvTerminations:
    """The terminations side of a DirectRLEnv: the device tables and the manager's buffers."""

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

    @staticmethod
    def is_state_key(k: str) -> bool:
        return k.startswith(STATE_PREFIX)

    # ---- launches
    def compute(self, terminated=None, truncated=None) -> torch.Tensor:
        """One launch: every term on the env's state as it stands.  terminated / truncated: the step's own flags
        ((n,) bool / uint8; None: no env was reset by the step).  Returns dones (n,) uint8."""
        env, spec = self._env, self.spec
        tensors = env._terminations_sources(net=spec.uses("illegal_contact"))
        tensors["step_terminated"], tensors["step_truncated"] = _u8(terminated), _u8(truncated)
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
        k = self.spec.index(term_name)
        new, old = parse_term(term_name, cfg, self.spec.ctx), self.spec.terms[k]
        if new.kind != old.kind:  # (the sources a launch is given, a captured one too, follow the kinds)
            kinds = _native.TERMINATION_KINDS
            raise _unsupported(term_name, f"the new cfg changes the term's function from {kinds[old.kind]} to "
                                          f"{kinds[new.kind]}; the terms' functions are fixed at construction (params "
                                          f"and time_out may change)")
        self.spec.terms[k] = new
        self.spec.build()
        self.desc.copy_(torch.as_tensor(self.spec.rows.copy()))
        self.table.copy_(torch.as_tensor(self.spec.table.copy()))

    # ---- state (get_state / set_state of the envs)
    def tensors(self) -> dict:
        return {STATE_PREFIX + "term_dones": self.term_dones, STATE_PREFIX + "time_outs": self.time_outs,
                STATE_PREFIX + "terminated": self.terminated, STATE_PREFIX + "dones": self.dones,
                STATE_PREFIX + "last_episode_dones": self.last_episode_dones,
                STATE_PREFIX + "reset_request": self.reset_request}

    def get_state(self) -> dict:
        return {k: v.clone() for k, v in self.tensors().items()}

    def set_state(self, state: dict) -> None:
        for k, v in self.tensors().items():
            if k in state:
                v.copy_(torch.as_tensor(state[k]).to(v.device, v.dtype).reshape(v.shape))


def _u8(x):
    if x is None:
        return None
    return x.view(torch.uint8) if x.dtype == torch.bool else x.to(torch.uint8)


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
