"""Device state of an env's reward manager (``cfg.rewards``) and the ``env.reward_manager`` view of it.

``DirectRLEnv`` builds an :class:`EnvRewards` once the subclass has its device state and launches ``as_rewards_step``
in ``step`` after the step and its in-kernel reset, the contact timers, the commands and the interval events, and
before the observation manager (csrc/reward_kernels.h; semantics and rounding order: csrc/allsteps_rewards.h).
Everything the kernel reads and writes -- the term descriptors, the index table, the reward, the episodic sums, the
per-step term values, the sums of the last episode and the previous actions -- lives in fixed device tensors, so a
step captured in a HIP graph replays, and ``set_term_cfg`` takes effect in a graph that is already captured.
"""

from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np
import torch

from .. import _native
from ..utils import rewards as RW
from ..utils.observations import resolve_joint_ids
from ..utils.rewards import resolve_body_ids

_KIND = {name: k for k, name in enumerate(_native.REW_KINDS)}
_FUNCS = {getattr(RW, name): name for name in RW.SERVED}
_REFUSED = {getattr(RW, name): name for name in RW.REFUSED}
STATE_PREFIX = "reward_"


def _unsupported(term: str | None, detail: str) -> "_native.NativeError":
    where = "cfg.rewards" + ("" if term is None else f" term {term!r}")
    return _native.NativeError(f"{where}: {detail}.  The rewards are computed in a HIP kernel (no host fallback); "
                               f"supported: {RW.SUPPORTED}")


def _is_number(x) -> bool:
    return isinstance(x, (int, float, np.floating, np.integer)) and not isinstance(x, bool)


@dataclass
class SensorInfo:
    """A contact sensor as the terms address it: its bodies' names, and per body the row of the net forces and of
    the timers it reads."""

    body_names: list
    net_bodies: list  # body b of the sensor -> body row of the contact report's net impulses
    timer_bodies: list  # body b of the sensor -> body row of the contact timers


@dataclass
class RewContext:
    """What the terms of an env can read -- the host facts the parser checks a cfg against (no device needed)."""

    joint_names: list
    default_joint_pos: np.ndarray  # (joints,) float32
    soft_joint_pos_limits: np.ndarray  # (joints, 2) float32
    action_cols: int
    step_dt: float
    command_names: list = field(default_factory=list)
    sensors: dict = field(default_factory=dict)  # name -> SensorInfo
    contact_forces: bool = False  # the contact report (cfg.contact_forces): net forces and qd_prev
    contact_air_time: bool = False  # the contact timers (cfg.contact_air_time)


@dataclass
class TermSpec:
    """One parsed term: what the descriptor row and the index table's row are made from."""

    name: str
    cfg: object
    kind: int
    weight: np.float32
    ids: list
    a: np.ndarray
    b: np.ndarray
    cmd_row: int = 0
    p0: np.float32 = np.float32(0.0)
    p1: np.float32 = np.float32(0.0)


def _params(params: dict, required: tuple, optional: tuple, t: str) -> None:
    extra = sorted(set(params) - set(required) - set(optional))
    if extra:
        raise _unsupported(t, f"params {extra} are not parameters of the term function (it takes "
                              f"{list(required + optional)})")
    missing = [k for k in required if k not in params]
    if missing:
        raise _unsupported(t, f"the term function needs params {missing}")


def _number(params: dict, key: str, t: str) -> np.float32:
    """A Python scalar as torch takes it in an operation with a float32 tensor."""
    x = params[key]
    if not _is_number(x):
        raise _unsupported(t, f"{key} = {x!r} is not a number")
    return np.float32(x)


def _robot_asset(params: dict, t: str):
    asset = params.get("asset_cfg", None)
    if asset is None:
        return RW.SceneEntityCfg("robot")
    if not hasattr(asset, "name"):
        raise _unsupported(t, f"params['asset_cfg'] = {asset!r} is not a SceneEntityCfg")
    if asset.name != "robot":
        raise _unsupported(t, f"asset_cfg.name = {asset.name!r} is not 'robot' (the env's articulation)")
    return asset


def _command(params: dict, ctx: RewContext, t: str) -> int:
    if not ctx.command_names:
        raise _unsupported(t, "the term reads a command, and the env has no command manager: set cfg.commands")
    cname = params.get("command_name", None)
    if cname not in ctx.command_names:
        raise _unsupported(t, f"command_name = {cname!r} names no command term of cfg.commands ({ctx.command_names})")
    return 3 * ctx.command_names.index(cname)


def _sensor_bodies(params: dict, ctx: RewContext, t: str, timers: bool) -> list:
    """The rows of the net forces (or of the timers) that sensor_cfg's bodies read."""
    if timers and not ctx.contact_air_time:
        raise _unsupported(t, "the term reads the contact sensors' air / contact timers: set cfg.contact_air_time")
    if not timers and not ctx.contact_forces:
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
    rows = info.timer_bodies if timers else info.net_bodies
    return [int(rows[k]) for k in ids]


def parse_term(t: str, cfg, ctx: RewContext) -> TermSpec:
    f32 = np.float32
    if not isinstance(cfg, RW.RewardTermCfg):
        raise TypeError(f"Configuration for the term '{t}' is not of type RewardTermCfg. Received: '{type(cfg)}'.")
    if not isinstance(cfg.weight, (float, int)):
        raise TypeError(f"Weight for the term '{t}' is not of type float or int. Received: '{type(cfg.weight)}'.")
    func = cfg.func
    name = getattr(func, "__name__", repr(func))
    if func is RW.MISSING or not callable(func):
        raise _unsupported(t, f"func = {func!r} is not callable")
    if not isinstance(cfg.params, dict):
        raise _unsupported(t, f"params = {cfg.params!r} is not a dict")
    p = cfg.params
    if func in _REFUSED or name in RW.REFUSED:
        raise _unsupported(t, f"{name}: {RW.REFUSED[name]}")
    if func not in _FUNCS:
        raise _unsupported(t, f"func = {name!r} is not a served term function")
    kname = _FUNCS[func]
    kind = _KIND[kname]
    z = np.zeros(0, f32)
    spec = TermSpec(t, cfg, kind, f32(cfg.weight), [], z, z)
    if kname in ("is_alive", "is_terminated", "action_l2", "action_rate_l2"):
        _params(p, (), (), t)
    elif kname in ("lin_vel_z_l2", "ang_vel_xy_l2", "flat_orientation_l2"):
        _params(p, (), ("asset_cfg",), t)
        _robot_asset(p, t)
    elif kname == "base_height_l2":
        _params(p, ("target_height",), ("asset_cfg", "sensor_cfg"), t)
        _robot_asset(p, t)
        if p.get("sensor_cfg", None) is not None:
            raise _unsupported(t, "base_height_l2 with a sensor_cfg (a target height adjusted by a ray caster) is "
                                  "not served")
        spec.p0 = _number(p, "target_height", t)
    elif kname.startswith("joint_"):
        _params(p, (), ("asset_cfg",), t)
        asset = _robot_asset(p, t)
        if kname == "joint_acc_l2" and not ctx.contact_forces:
            raise _unsupported(t, "joint_acc_l2 reads the contact report's qd_prev: set cfg.contact_forces")
        try:
            ids = resolve_joint_ids(asset, ctx.joint_names, "asset_cfg")
        except ValueError as e:
            raise _unsupported(t, str(e)) from None
        ids = list(range(len(ctx.joint_names))) if ids is None else ids
        if not ids:
            raise _unsupported(t, "asset_cfg selects no joint")
        spec.ids = ids
        if kname == "joint_deviation_l1":
            spec.a = ctx.default_joint_pos.astype(f32)[ids]
        elif kname == "joint_pos_limits":
            lim = ctx.soft_joint_pos_limits.astype(f32)
            spec.a, spec.b = lim[ids, 0], lim[ids, 1]
    elif kname in ("undesired_contacts", "contact_forces"):
        _params(p, ("threshold", "sensor_cfg"), (), t)
        spec.ids = _sensor_bodies(p, ctx, t, timers=False)
        spec.p0 = _number(p, "threshold", t)
    elif kname in ("feet_air_time", "feet_air_time_positive_biped"):
        _params(p, ("command_name", "sensor_cfg", "threshold"), (), t)
        spec.ids = _sensor_bodies(p, ctx, t, timers=True)
        spec.cmd_row = _command(p, ctx, t)
        spec.p0 = _number(p, "threshold", t)
        spec.p1 = f32(float(ctx.step_dt) + 1.0e-8)  # compute_first_contact(step_dt): dt + abs_tol in double
    else:  # the exp terms
        _params(p, ("std", "command_name"), ("asset_cfg",), t)
        _robot_asset(p, t)
        spec.cmd_row = _command(p, ctx, t)
        if not _is_number(p["std"]):
            raise _unsupported(t, f"std = {p['std']!r} is not a number")
        spec.p0 = f32(float(p["std"]) ** 2)  # std**2 in double, then torch's cast
    if len(spec.ids) > _native.MAX_REW_IDS:
        raise _unsupported(t, f"the term selects {len(spec.ids)} joints or bodies; the index table holds "
                              f"AS_MAX_REW_IDS = {_native.MAX_REW_IDS}")
    return spec


def _items(obj) -> list:
    """(name, value) of a cfg object in cfg order: a dict, or an object's attributes, then its classes' attributes
    that are RewardTermCfg (the reference's configclass turns those into instance fields)."""
    if isinstance(obj, dict):
        return list(obj.items())
    items = [(k, v) for k, v in vars(obj).items() if not k.startswith("_")]
    seen = {k for k, _ in items}
    for klass in reversed(type(obj).__mro__[:-1]):
        for k, v in vars(klass).items():
            if k not in seen and not k.startswith("_") and isinstance(v, RW.RewardTermCfg):
                items.append((k, v))
                seen.add(k)
    return items


class RewardTerms:
    """The host side of cfg.rewards: the terms in cfg order, checked (no device needed), and the device tables as
    host arrays."""

    def __init__(self, rewards, ctx: RewContext):
        self.ctx = ctx
        self.terms: list[TermSpec] = []
        for name, cfg in _items(rewards):
            if cfg is None:  # (as the reference's _prepare_terms)
                continue
            self.terms.append(parse_term(name, cfg, ctx))
        if not self.terms:
            raise _unsupported(None, "there are no terms")
        if len(self.terms) > _native.MAX_REW_TERMS:
            raise _unsupported(None, f"{len(self.terms)} terms; the reward kernel takes at most AS_MAX_REW_TERMS = "
                                     f"{_native.MAX_REW_TERMS}")
        self.build()

    names = property(lambda self: [t.name for t in self.terms])

    def build(self) -> None:
        """The descriptor rows, the index table and the kinds mask from the term specs as they stand."""
        f32, i32 = np.float32, np.int32
        rows = np.zeros((len(self.terms), _native.REW_TERM_WORDS), f32)
        table = np.zeros((_native.REW_TABLE_ROWS, _native.MAX_REW_TERMS, _native.MAX_REW_IDS), f32)
        for k, t in enumerate(self.terms):
            ints = rows[k].view(i32)
            ints[0], rows[k, 1], ints[2], ints[3], rows[k, 4], rows[k, 5] = (t.kind, t.weight, len(t.ids), t.cmd_row,
                                                                             t.p0, t.p1)
            m = len(t.ids)
            table[0, k, :m] = np.asarray(t.ids, i32).view(f32)
            table[1, k, :len(t.a)] = t.a
            table[2, k, :len(t.b)] = t.b
        self.rows, self.table = rows, table
        self.kinds = 0
        for t in self.terms:
            self.kinds |= 1 << t.kind

    def index(self, term_name: str) -> int:
        if term_name not in self.names:
            raise ValueError(f"Reward term '{term_name}' not found.")
        return self.names.index(term_name)

    def uses(self, *kinds: str) -> bool:
        return any(_native.REW_KINDS[t.kind] in kinds for t in self.terms)

    def table_str(self) -> str:
        """RewardManager.__str__ in the reference's form."""
        rows = [(str(i), t.name, str(t.cfg.weight)) for i, t in enumerate(self.terms)]
        head = ("Index", "Name", "Weight")
        w = [max(len(r[j]) for r in rows + [head]) for j in range(3)]
        line = "+" + "+".join("-" * (x + 2) for x in w) + "+\n"
        total = len(line) - 3
        fmt = lambda r: "| " + " | ".join((r[0].center(w[0]), r[1].ljust(w[1]), r[2].rjust(w[2]))) + " |\n"  # noqa: E731
        msg = f"<RewardManager> contains {len(rows)} active terms.\n"
        msg += "+" + "-" * total + "+\n" + "|" + "Active Reward Terms".center(total) + "|\n"
        msg += line + "| " + " | ".join(h.center(x) for h, x in zip(head, w)) + " |\n" + line
        return msg + "".join(fmt(r) for r in rows) + line


class EnvRewards:
    """The rewards side of a DirectRLEnv: the device tables and the manager's buffers."""

    def __init__(self, cfg, env, n: int, device):
        self.n, self.device = n, device
        self._env = env
        self.spec = RewardTerms(cfg.rewards, env._rewards_context())
        self.replace_task_reward = bool(getattr(cfg, "rewards_replace_task_reward", False))
        T, A = len(self.spec.terms), int(self.spec.ctx.action_cols)
        z = lambda *shape: torch.zeros(*shape, dtype=torch.float32, device=device)  # noqa: E731
        self.desc = torch.as_tensor(self.spec.rows.copy(), device=device)
        self.table = torch.as_tensor(self.spec.table.copy(), device=device)
        self.reward = z(n)
        self.episode_sums = z(T, n)
        self.step_reward = z(T, n)
        self.last_episode_sums = z(T, n)
        self.prev_actions = z(n, A)
        self.launches = 0

    @staticmethod
    def wanted(cfg) -> bool:
        return getattr(cfg, "rewards", None) is not None

    @staticmethod
    def is_state_key(k: str) -> bool:
        return k.startswith(STATE_PREFIX)

    # ---- launches
    def compute(self, dt: float, terminated=None, reset=None, reset2=None) -> torch.Tensor:
        """One launch: every term on the env's state as it stands.  terminated: the step's flags ((n,) bool / uint8,
        None: the env's reset_terminated); reset / reset2: the step's dones (None: no env is done)."""
        env, spec = self._env, self.spec
        tensors = env._rewards_sources(net=spec.uses("undesired_contacts", "contact_forces"))
        tensors["terminated"] = _u8(env.reset_terminated if terminated is None else terminated)
        src = _native.make_reward_sources(tensors, env.physics_dt, env._actions_clamped)
        _native.rewards_step(self.desc, self.table, spec.kinds, src, self.reward, self.episode_sums,
                             self.step_reward, self.last_episode_sums, self.prev_actions, reset=_u8(reset),
                             reset2=_u8(reset2), dt=float(dt), stream=env._noise_stream())
        self.launches += 1
        return self.reward

    def reset(self, mask) -> None:
        """RewardManager.reset(env_ids) for the envs of a uint8 / bool mask (None: all): the sums and prev_actions
        become 0; nothing is logged here (``RewardManagerView.reset`` returns the extras)."""
        if mask is not None:
            mask = _u8(mask.to(self.device).reshape(self.n))
        _native.rewards_reset(self.episode_sums, self.prev_actions, mask=mask, stream=self._env._noise_stream())
        self.launches += 1

    def set_term_cfg(self, term_name: str, cfg) -> None:
        k = self.spec.index(term_name)
        new, old = parse_term(term_name, cfg, self.spec.ctx), self.spec.terms[k]
        if new.kind != old.kind:  # (the sources a launch is given, a captured one too, follow the kinds)
            raise _unsupported(term_name, f"the new cfg changes the term's function from "
                                          f"{_native.REW_KINDS[old.kind]} to {_native.REW_KINDS[new.kind]}; the terms' "
                                          f"functions are fixed at construction (weight and params may change)")
        self.spec.terms[k] = new
        self.spec.build()
        self.desc.copy_(torch.as_tensor(self.spec.rows.copy()))
        self.table.copy_(torch.as_tensor(self.spec.table.copy()))

    # ---- state (get_state / set_state of the envs)
    def tensors(self) -> dict:
        return {STATE_PREFIX + "episode_sums": self.episode_sums, STATE_PREFIX + "step": self.step_reward,
                STATE_PREFIX + "last_episode_sums": self.last_episode_sums,
                STATE_PREFIX + "prev_actions": self.prev_actions}

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


class RewardManagerView:
    """``env.reward_manager``: the caller-visible surface of the reference's ``RewardManager``
    (reward_manager.py:23-246) over the device state."""

    def __init__(self, rew: EnvRewards):
        self._r = rew

    active_terms = property(lambda self: list(self._r.spec.names))
    reward_buf = property(lambda self: self._r.reward)
    _reward_buf = reward_buf
    prev_actions = property(lambda self: self._r.prev_actions)

    @property
    def _episode_sums(self) -> dict:
        """{term: (N,) view} of the running episodic sums."""
        return {name: self._r.episode_sums[k] for k, name in enumerate(self._r.spec.names)}

    @property
    def last_episode_sums(self) -> dict:
        """{term: (N,)} the sums an env had when the step last reset it -- what the reference's reset logs, as a
        captured step serves it."""
        return {name: self._r.last_episode_sums[k] for k, name in enumerate(self._r.spec.names)}

    @property
    def _step_reward(self) -> torch.Tensor:
        """(N, T) the terms' values of the last launch (weighted, per second): a transposed view."""
        return self._r.step_reward.T

    def compute(self, dt: float) -> torch.Tensor:
        """RewardManager.compute(dt) on the env's state as it stands: one launch, no env counts as done."""
        return self._r.compute(dt)

    def reset(self, env_ids=None) -> dict:
        """RewardManager.reset(env_ids): ``Episode_Reward/<term>`` = mean of the sums over ``env_ids`` /
        max_episode_length_s (a host read), then the reset of those envs, one launch."""
        r = self._r
        sel = slice(None) if env_ids is None else torch.as_tensor(env_ids, device=r.device).long()
        extras = {f"Episode_Reward/{name}": (torch.mean(r.episode_sums[k][sel]) / r._env.max_episode_length_s).item()
                  for k, name in enumerate(r.spec.names)}
        mask = None
        if env_ids is not None:
            mask = torch.zeros(r.n, dtype=torch.uint8, device=r.device)
            mask[sel] = 1
        r.reset(mask)
        return extras

    def set_term_cfg(self, term_name: str, cfg) -> None:
        """Replace a term's cfg.  The new descriptor is written into device memory in place, so it holds from the
        next launch on, in a captured graph too; a cfg with another term function is refused."""
        self._r.set_term_cfg(term_name, cfg)

    def get_term_cfg(self, term_name: str):
        return self._r.spec.terms[self._r.spec.index(term_name)].cfg

    def get_active_iterable_terms(self, env_idx: int) -> list:
        step = self._r.step_reward[:, env_idx].cpu()
        return [(name, [step[k].item()]) for k, name in enumerate(self._r.spec.names)]

    def __str__(self) -> str:
        return self._r.spec.table_str()
