"""The action manager of the envs (``cfg.actions``): parsing of the reference's joint action term cfgs into the device
column table, the manager's buffers, and ``env.action_manager``.

``cfg.actions`` is a dict or a cfg object whose entries are ``utils.actions`` term cfgs, in cfg order (None entries are
skipped).  A column is one (term, joint) pair.  ``k_actions_process`` (csrc/action_kernels.h) runs once per ``step``
after the action noise model and before the physics: prev_action <- action, action <- input, processed, the EMA
columns' prev_applied, and the joint command buffer ``cmd`` (N, joints), which the physics reads through
``as_set_joint_commands`` in place of the actuator's own action formula.  ``k_actions_reset`` is
``ActionManager.reset`` over a device mask.  Semantics and rounding: csrc/allsteps_actions.h.

Anything the kernels do not serve raises ``NativeError`` at construction, naming the term and the reason; the
reference's own ``ValueError``s (names that match nothing or twice, an ``alpha`` outside [0, 1], a scale of a wrong
type, ``cfg.action_space`` != the terms' total) are kept as they are.
"""

from __future__ import annotations

from dataclasses import dataclass

import numpy as np
import torch

from .. import _native
from ..utils import actions as AC
from ._manager import DeviceState, cfg_items, u8

KIND_POSITION, KIND_EFFORT, KIND_TO_LIMITS, KIND_EMA = range(4)  # AS_ACTION_*
_POSITION_KINDS = (KIND_POSITION, KIND_TO_LIMITS, KIND_EMA)
# words of as_action_column_t
_W_JOINT, _W_KIND, _W_RESCALE, _W_TERM, _W_SCALE, _W_OFFSET, _W_CLIP_LO, _W_CLIP_HI, _W_LIM_LO, _W_LIM_HI, _W_ALPHA, \
    _W_OMA = range(12)


def _unsupported(term: str, detail: str) -> "_native.NativeError":
    return _native.NativeError(f"cfg.actions term {term!r}: {detail}.  The action terms run in a HIP kernel (no host "
                               f"fallback); supported: {AC.SUPPORTED}")


@dataclass
class ActContext:
    """What the terms of an env can resolve against."""

    joint_names: list
    default_joint_pos: np.ndarray       # (joints,)
    soft_joint_pos_limits: np.ndarray   # (joints, 2)
    actuator: int = _native.ACT_TORQUE  # _native.ACT_TORQUE / ACT_DC_MOTOR: what the physics does with a command
    action_space: int | None = None     # cfg.action_space, or None: not checked


@dataclass
class ActionTerm:
    name: str
    cfg: object
    kind: int
    joint_ids: list
    joint_names: list
    rows: np.ndarray  # (action_dim, 12) uint32 words of as_action_column_t (term and joint filled by ActionTerms)

    @property
    def action_dim(self) -> int:
        return len(self.joint_ids)


def named_terms(actions) -> list:
    """[(name, cfg)] of a dict or cfg object, in its order, without the None entries.  Unlike the other managers'
    walks this one has never read a class's attributes or passed over names that begin with ``_``; it is kept so."""
    return list(cfg_items(actions, AC.ActionTermCfg, private="keep", class_attrs=False))


def _f32(x) -> np.float32:
    """A Python number as torch takes it against a float32 tensor."""
    return np.float32(float(x))


def _per_joint(name: str, what: str, value, names: list, default: float) -> np.ndarray:
    """A float or a regex dict over the term's joints as float32 per joint (joint_actions.py:79-98)."""
    if isinstance(value, (float, int)):
        return np.full(len(names), _f32(value), np.float32)
    if isinstance(value, dict):
        out = np.full(len(names), default, np.float32)
        ids, _, vals = AC.resolve_matching_names_values(value, names)
        out[ids] = np.asarray([float(v) for v in vals], np.float64).astype(np.float32)
        return out
    raise ValueError(f"Unsupported {what} type: {type(value)}. Supported types are float and dict.")


def _clip(cfg, names: list) -> np.ndarray:
    out = np.empty((len(names), 2), np.float32)
    out[:, 0], out[:, 1] = -np.inf, np.inf
    if cfg.clip is None:
        return out
    if not isinstance(cfg.clip, dict):
        raise ValueError(f"Unsupported clip type: {type(cfg.clip)}. Supported types are dict.")
    ids, _, vals = AC.resolve_matching_names_values(cfg.clip, names)
    out[ids] = np.asarray([[float(v[0]), float(v[1])] for v in vals], np.float64).astype(np.float32).reshape(-1, 2)
    return out


def _alpha(cfg, names: list):
    """(alpha, 1 - alpha) per joint as the reference's process_actions multiplies them (:208-213): a float alpha
    enters both products as a Python scalar (1.0 - alpha formed in double), a dict as a float32 tensor."""
    a = cfg.alpha
    if isinstance(a, float):
        if not 0.0 <= a <= 1.0:
            raise ValueError(f"Moving average weight must be in the range [0, 1]. Got {a}.")
        return np.full(len(names), _f32(a), np.float32), np.full(len(names), _f32(1.0 - a), np.float32)
    if isinstance(a, dict):
        out = np.ones(len(names), np.float32)
        ids, hit, vals = AC.resolve_matching_names_values(a, names)
        for n_, v in zip(hit, vals):
            if not 0.0 <= v <= 1.0:
                raise ValueError(f"Moving average weight must be in the range [0, 1]. Got {v} for joint {n_}.")
        out[ids] = np.asarray([float(v) for v in vals], np.float64).astype(np.float32)
        return out, (np.float32(1.0) - out).astype(np.float32)
    raise ValueError(f"Unsupported moving average weight type: {type(a)}. Supported types are float and dict.")


def parse_term(name: str, cfg, ctx: ActContext) -> ActionTerm:
    for cls in type(cfg).__mro__:
        if cls.__name__ in AC.REFUSED and cls.__module__ == AC.__name__:
            raise _unsupported(name, f"{cls.__name__} is not served: {AC.REFUSED[cls.__name__]}")
    if isinstance(cfg, AC.EMAJointPositionToLimitsActionCfg):
        kind = KIND_EMA
    elif isinstance(cfg, AC.JointPositionToLimitsActionCfg):
        kind = KIND_TO_LIMITS
    elif isinstance(cfg, AC.JointPositionActionCfg):
        kind = KIND_POSITION
    elif isinstance(cfg, AC.JointEffortActionCfg):
        kind = KIND_EFFORT
    else:
        raise _unsupported(name, f"{type(cfg).__name__} is not one of the served term cfgs (a custom term class "
                                 f"cannot run in the kernel)")
    if cfg.debug_vis:
        raise _unsupported(name, "debug_vis = True: there is no visualisation")
    if cfg.asset_name != "robot":
        raise _unsupported(name, f"asset_name = {cfg.asset_name!r} is not 'robot' (the env's articulation)")
    if kind in _POSITION_KINDS and ctx.actuator != _native.ACT_DC_MOTOR:
        raise _unsupported(name, "a joint position term needs the DC-motor actuator (AS_ACT_DC_MOTOR, the quadruped); "
                                 "this env's torque actuator has kp = kd = 0, so a position target would do nothing")
    if kind == KIND_EFFORT and ctx.actuator != _native.ACT_TORQUE:
        raise _unsupported(name, "a joint effort term needs the torque actuator (AS_ACT_TORQUE, the walker); this "
                                 "env's DC motor takes position targets")
    names_all = list(ctx.joint_names)
    if kind in (KIND_POSITION, KIND_EFFORT):
        ids, names = AC.resolve_matching_names(cfg.joint_names, names_all, bool(cfg.preserve_order))
    else:
        ids, names = AC.resolve_matching_names(cfg.joint_names, names_all)
    k = len(ids)
    rows = np.zeros((k, _native.ACTION_COLUMN_WORDS), np.uint32)
    fl = rows.view(np.float32)
    rows.view(np.int32)[:, _W_KIND] = kind
    fl[:, _W_SCALE] = _per_joint(name, "scale", cfg.scale, names, 1.0)
    if kind in (KIND_POSITION, KIND_EFFORT):
        fl[:, _W_OFFSET] = _per_joint(name, "offset", cfg.offset, names, 0.0)
        if kind == KIND_POSITION and cfg.use_default_offset:
            fl[:, _W_OFFSET] = np.asarray(ctx.default_joint_pos, np.float32)[ids]
    clip = _clip(cfg, names)
    if np.isnan(clip).any():
        raise _unsupported(name, "a clip bound is NaN")
    fl[:, _W_CLIP_LO], fl[:, _W_CLIP_HI] = clip[:, 0], clip[:, 1]
    lim = np.asarray(ctx.soft_joint_pos_limits, np.float32)[ids]
    fl[:, _W_LIM_LO], fl[:, _W_LIM_HI] = lim[:, 0], lim[:, 1]
    fl[:, _W_ALPHA], fl[:, _W_OMA] = 1.0, 0.0
    if kind in (KIND_TO_LIMITS, KIND_EMA):
        rows.view(np.int32)[:, _W_RESCALE] = int(bool(cfg.rescale_to_limits))
    if kind == KIND_EMA:
        fl[:, _W_ALPHA], fl[:, _W_OMA] = _alpha(cfg, names)
    rows.view(np.int32)[:, _W_JOINT] = ids
    return ActionTerm(name, cfg, kind, list(ids), list(names), rows)


class ActionTerms:
    """The parsed cfg.actions: the terms in cfg order and the column table."""

    def __init__(self, actions, ctx: ActContext):
        self.ctx = ctx
        self.terms = [parse_term(k, c, ctx) for k, c in named_terms(actions)]
        self.names = [t.name for t in self.terms]
        self.dims = [t.action_dim for t in self.terms]
        self.total = sum(self.dims)
        if self.total > _native.ACT_DIM:
            raise _native.NativeError(f"cfg.actions has {self.total} columns ({dict(zip(self.names, self.dims))}); the "
                                      f"action kernel takes at most AS_ACT_DIM = {_native.ACT_DIM}")
        count = np.zeros(len(ctx.joint_names), np.int64)
        for t in self.terms:
            np.add.at(count, t.joint_ids, 1)
        missing = [n for n, c in zip(ctx.joint_names, count) if c == 0]
        twice = [n for n, c in zip(ctx.joint_names, count) if c > 1]
        if missing or twice:
            raise _native.NativeError(
                f"cfg.actions must command every joint of the robot exactly once: not commanded {missing}, commanded "
                f"more than once {twice}.  What an uncommanded joint's target would be depends on scene reset code "
                f"this project does not have; supported: {AC.SUPPORTED}")
        if ctx.action_space is not None and int(ctx.action_space) != self.total:
            raise ValueError(f"cfg.action_space = {ctx.action_space} but the terms of cfg.actions take "
                             f"{self.total} columns ({dict(zip(self.names, self.dims))})")
        for k, t in enumerate(self.terms):
            t.rows.view(np.int32)[:, _W_TERM] = k
        self.rows = np.concatenate([t.rows for t in self.terms]).view(np.float32)  # (total, 12) words
        self.starts = [int(x) for x in np.cumsum([0] + self.dims[:-1])]
        self.column_joints = [j for t in self.terms for j in t.joint_ids]

    def index(self, name: str) -> int:
        if name not in self.names:
            raise KeyError(f"action term {name!r} not found; active terms: {self.names}")
        return self.names.index(name)

    def table_str(self) -> str:
        """ActionManager.__str__ in the reference's form (a title wider than the columns widens them, the last one
        taking the remainder, as the reference's table does)."""
        rows = [(str(i), t.name, str(t.action_dim)) for i, t in enumerate(self.terms)]
        head = ("Index", "Name", "Dimension")
        title = f"Active Action Terms (shape: {self.total})"
        w = [max(len(r[j]) for r in rows + [head]) for j in range(3)]
        need = len(title) + 4 - (3 * 2 + 4)  # content width under which the title does not fit
        if sum(w) < need:
            scale = need / sum(w)
            w = [int(x * scale) for x in w]
            w[-1] += need - sum(w)
        line = "+" + "+".join("-" * (x + 2) for x in w) + "+\n"
        total = len(line) - 3
        fmt = lambda r: "| " + " | ".join((r[0].center(w[0]), r[1].ljust(w[1]), r[2].rjust(w[2]))) + " |\n"  # noqa: E731
        msg = f"<ActionManager> contains {len(rows)} active terms.\n"
        msg += "+" + "-" * total + "+\n" + "|" + title.center(total) + "|\n"
        msg += line + fmt(head) + line  # (a header is aligned as its column)
        return msg + "".join(fmt(r) for r in rows) + line


class EnvActions(DeviceState):
    """The actions side of a DirectRLEnv: the device column table, the manager's buffers and the command buffer."""

    STATE_KEYS = ("action_action", "action_prev_action", "action_processed", "action_prev_applied", "action_commands")

    def __init__(self, cfg, env, n: int, device):
        self.n, self.device = n, device
        self._env = env
        self.spec = ActionTerms(cfg.actions, env._actions_context())
        D, J = self.spec.total, len(self.spec.ctx.joint_names)
        z = lambda cols: torch.zeros(n, cols, dtype=torch.float32, device=device)  # noqa: E731
        self.cols = torch.as_tensor(self.spec.rows.copy(), device=device)
        self.action, self.prev_action, self.processed, self.prev_applied = z(D), z(D), z(D), z(D)
        self.cmd = z(J)
        self.launches = 0

    @staticmethod
    def wanted(cfg) -> bool:
        return getattr(cfg, "actions", None) is not None

    # ---- launches
    def process(self, action: torch.Tensor) -> torch.Tensor:
        """ActionManager.process_action: one launch.  Returns the action as the launch read it (float32,
        contiguous, on the device)."""
        if action.dim() != 2 or self.spec.total != action.shape[1]:
            got = action.shape[1] if action.dim() == 2 else tuple(action.shape)
            raise ValueError(f"Invalid action shape, expected: {self.spec.total}, received: {got}.")
        if action.shape[0] != self.n:
            raise ValueError(f"Invalid action shape, expected {self.n} envs, received: {action.shape[0]}.")
        a = action.to(self.device)
        if a.dtype != torch.float32 or not a.is_contiguous():
            a = a.float().contiguous()
        _native.actions_step(self.cols, a, self.action, self.prev_action, self.processed, self.prev_applied,
                             self.cmd, stream=self._env._noise_stream())
        self.launches += 1
        return a

    def reset(self, mask=None, mask2=None) -> None:
        """ActionManager.reset over the envs of mask | mask2 ((n,) uint8 / bool device tensors; neither: all): one
        stream-ordered launch, no host read."""
        q = self._env._actions_joint_pos()
        _native.actions_reset(self.cols, self.action, self.prev_action, self.prev_applied, q, u8(mask), u8(mask2),
                              stream=self._env._noise_stream())
        self.launches += 1

    # ---- state (get_state / set_state of the envs)
    def tensors(self) -> dict:
        return dict(zip(self.STATE_KEYS, (self.action, self.prev_action, self.processed, self.prev_applied,
                                          self.cmd)))


class ActionTermView:
    """``env.action_manager.get_term(name)``: one term of the reference's ``ActionTerm`` surface over the manager's
    device buffers."""

    def __init__(self, act: EnvActions, k: int):
        self._a, self._k = act, k
        t = act.spec.terms[k]
        self.cfg = t.cfg
        self._lo, self._hi = act.spec.starts[k], act.spec.starts[k] + t.action_dim
        self._joint_ids, self._joint_names = list(t.joint_ids), list(t.joint_names)

    action_dim = property(lambda self: self._hi - self._lo)

    @property
    def raw_actions(self) -> torch.Tensor:
        """(N, action_dim) the term's columns of the manager's ``action``: a view -- the two are equal in the
        reference at every point (process_action stores both, reset zeroes both)."""
        return self._a.action[:, self._lo:self._hi]

    @property
    def processed_actions(self) -> torch.Tensor:
        return self._a.processed[:, self._lo:self._hi]

    @property
    def prev_applied_actions(self) -> torch.Tensor:
        """(N, action_dim) the EMA term's previous applied targets (zeros for the other terms)."""
        return self._a.prev_applied[:, self._lo:self._hi]

    def apply_actions(self) -> None:
        """Nothing to do: the physics reads the command buffer in every substep of the step."""


class ActionManagerView:
    """``env.action_manager``: the caller-visible surface of the reference's ``ActionManager``
    (action_manager.py:164-394) over the device state."""

    def __init__(self, act: EnvActions):
        self._a = act
        self._terms = {name: ActionTermView(act, k) for k, name in enumerate(act.spec.names)}

    action = property(lambda self: self._a.action)
    prev_action = property(lambda self: self._a.prev_action)
    total_action_dim = property(lambda self: self._a.spec.total)
    active_terms = property(lambda self: list(self._a.spec.names))
    action_term_dim = property(lambda self: list(self._a.spec.dims))
    joint_commands = property(lambda self: self._a.cmd, doc="(N, joints) the command buffer the physics reads")
    has_debug_vis_implementation = False

    def get_term(self, name: str) -> ActionTermView:
        return self._terms[name]

    def process_action(self, action: torch.Tensor) -> None:
        """ActionManager.process_action by hand: one launch on the manager's buffers (``step`` calls it itself)."""
        self._a.process(action)

    def apply_action(self) -> None:
        """Nothing to do: the step consumes the command buffer in every physics substep."""

    def reset(self, env_ids=None) -> dict:
        a = self._a
        if env_ids is None:
            a.reset(None)
        else:
            ids = torch.as_tensor(env_ids, device=a.device)
            if ids.dtype == torch.bool:
                mask = ids.to(torch.uint8)
            else:
                mask = torch.zeros(a.n, dtype=torch.uint8, device=a.device)
                mask[ids.long().reshape(-1)] = 1
            a.reset(mask)
        return {}

    def set_debug_vis(self, debug_vis: bool) -> bool:
        return False

    def get_active_iterable_terms(self, env_idx: int) -> list:
        row = self._a.action[env_idx].cpu()
        return [(name, row[t._lo:t._hi].tolist()) for name, t in self._terms.items()]

    def __str__(self) -> str:
        return self._a.spec.table_str()
