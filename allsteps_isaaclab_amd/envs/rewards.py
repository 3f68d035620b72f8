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
from functools import partial

import numpy as np
import torch

from .. import _native
from ..utils import rewards as RW
from . import _manager as M
from ._manager import SensorInfo, u8  # noqa: F401  (SensorInfo: re-exported)

_KIND = {name: k for k, name in enumerate(_native.REW_KINDS)}
_FUNCS = {getattr(RW, name): name for name in RW.SERVED}
_REFUSED = {getattr(RW, name): name for name in RW.REFUSED}


def _unsupported(term: str | None, detail: str) -> "_native.NativeError":
    where = "cfg.rewards" + ("" if term is None else f" term {term!r}")
    return _native.NativeError(f"{where}: {detail}.  The rewards are computed in a HIP kernel (no host fallback); "
                               f"supported: {RW.SUPPORTED}")


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


_params = partial(M.check_params, _unsupported)
_number = partial(M.number, _unsupported)
_robot_asset = partial(M.robot_asset, _unsupported)
_sensor_bodies = partial(M.sensor_bodies, _unsupported)


def _command(params: dict, ctx: RewContext, t: str) -> int:
    if not ctx.command_names:
        raise _unsupported(t, "the term reads a command, and the env has no command manager: set cfg.commands")
    cname = params.get("command_name", None)
    if cname not in ctx.command_names:
        raise _unsupported(t, f"command_name = {cname!r} names no command term of cfg.commands ({ctx.command_names})")
    return 3 * ctx.command_names.index(cname)


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
        spec.p0 = _number(p["target_height"], "target_height", t)
    elif kname.startswith("joint_"):
        _params(p, (), ("asset_cfg",), t)
        asset = _robot_asset(p, t)
        if kname == "joint_acc_l2" and not ctx.contact_forces:
            raise _unsupported(t, "joint_acc_l2 reads the contact report's qd_prev: set cfg.contact_forces")
        spec.ids = ids = M.joint_ids(_unsupported, asset, ctx.joint_names, t)
        if kname == "joint_deviation_l1":
            spec.a = ctx.default_joint_pos.astype(f32)[ids]
        elif kname == "joint_pos_limits":
            lim = ctx.soft_joint_pos_limits.astype(f32)
            spec.a, spec.b = lim[ids, 0], lim[ids, 1]
    elif kname in ("undesired_contacts", "contact_forces"):
        _params(p, ("threshold", "sensor_cfg"), (), t)
        spec.ids = _sensor_bodies(p, ctx, t, timers=False)
        spec.p0 = _number(p["threshold"], "threshold", t)
    elif kname in ("feet_air_time", "feet_air_time_positive_biped"):
        _params(p, ("command_name", "sensor_cfg", "threshold"), (), t)
        spec.ids = _sensor_bodies(p, ctx, t, timers=True)
        spec.cmd_row = _command(p, ctx, t)
        spec.p0 = _number(p["threshold"], "threshold", t)
        spec.p1 = f32(float(ctx.step_dt) + 1.0e-8)  # compute_first_contact(step_dt): dt + abs_tol in double
    else:  # the exp terms
        _params(p, ("std", "command_name"), ("asset_cfg",), t)
        _robot_asset(p, t)
        spec.cmd_row = _command(p, ctx, t)
        _number(p["std"], "std", t)
        spec.p0 = f32(float(p["std"]) ** 2)  # std**2 in double, then torch's cast
    if len(spec.ids) > _native.MAX_REW_IDS:
        raise _unsupported(t, f"the term selects {len(spec.ids)} joints or bodies; the index table holds "
                              f"AS_MAX_REW_IDS = {_native.MAX_REW_IDS}")
    return spec


class RewardTerms(M.TermTable):
    """The host side of cfg.rewards: the terms in cfg order, checked (no device needed), and the device tables as
    host arrays."""

    NOUN, TERM_TYPE, KINDS = "Reward", RW.RewardTermCfg, _native.REW_KINDS
    WORDS, TABLE = _native.REW_TERM_WORDS, (_native.REW_TABLE_ROWS, _native.MAX_REW_TERMS, _native.MAX_REW_IDS)
    LIMIT, COLUMN, MAY_CHANGE = "AS_MAX_REW_TERMS", ("Weight", str.rjust), "weight and params"
    parse_term, unsupported = staticmethod(parse_term), staticmethod(_unsupported)

    def pack(self, row, ints, t: TermSpec) -> None:
        ints[0], row[1], ints[2], ints[3], row[4], row[5] = t.kind, t.weight, len(t.ids), t.cmd_row, t.p0, t.p1

    def column(self, t: TermSpec) -> str:
        return str(t.cfg.weight)


class EnvRewards(M.DeviceState):
    """The rewards side of a DirectRLEnv: the device tables and the manager's buffers."""

    STATE_PREFIX = "reward_"

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

    # ---- launches
    def compute(self, dt: float, terminated=None, reset=None, reset2=None) -> torch.Tensor:
        """One launch: every term on the env's state as it stands.  terminated: the step's flags ((n,) bool / uint8,
        None: the env's reset_terminated); reset / reset2: the step's dones (None: no env is done)."""
        env, spec = self._env, self.spec
        tensors = env._rewards_sources(net=spec.uses("undesired_contacts", "contact_forces"))
        tensors["terminated"] = u8(env.reset_terminated if terminated is None else terminated)
        src = _native.make_reward_sources(tensors, env.physics_dt, env._actions_clamped)
        _native.rewards_step(self.desc, self.table, spec.kinds, src, self.reward, self.episode_sums,
                             self.step_reward, self.last_episode_sums, self.prev_actions, reset=u8(reset),
                             reset2=u8(reset2), dt=float(dt), stream=env._noise_stream())
        self.launches += 1
        return self.reward

    def reset(self, mask) -> None:
        """RewardManager.reset(env_ids) for the envs of a uint8 / bool mask (None: all): the sums and prev_actions
        become 0; nothing is logged here (``RewardManagerView.reset`` returns the extras)."""
        if mask is not None:
            mask = u8(mask.to(self.device).reshape(self.n))
        _native.rewards_reset(self.episode_sums, self.prev_actions, mask=mask, stream=self._env._noise_stream())
        self.launches += 1

    def set_term_cfg(self, term_name: str, cfg) -> None:
        self.spec.replace(term_name, cfg, self.desc, self.table)

    # ---- state (get_state / set_state of the envs)
    def tensors(self) -> dict:
        return {"reward_episode_sums": self.episode_sums, "reward_step": self.step_reward,
                "reward_last_episode_sums": self.last_episode_sums, "reward_prev_actions": self.prev_actions}


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
