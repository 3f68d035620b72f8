"""Device state of an env's command manager (``cfg.commands``) and the ``env.command_manager`` view of it.

``DirectRLEnv`` builds an :class:`EnvCommands` at construction when ``cfg.commands`` is set and launches
``as_commands_step`` after the step -- after its in-kernel reset and before the interval events, the reference's
order (manager_based_rl_env.py:220-239) -- on the env's stream (csrc/command_kernels.h; semantics and Philox
stream: csrc/allsteps_commands.h).  Everything the kernel reads and writes -- commands, heading targets, masks,
timers, counters, metrics, the per-env stream counter ``t``, the term descriptors -- lives in fixed device tensors,
so a step captured in a HIP graph replays with fresh draws, and ``set_term_cfg`` or a range edit followed by
``refresh()`` takes effect in a graph that is already captured.
"""

from __future__ import annotations

import math
import warnings

import numpy as np
import torch

from .. import _native
from ..utils import commands as CM
from ._manager import DeviceState, RowTerms, is_number, u8

METRIC_NAMES = ("error_vel_xy", "error_vel_yaw")


def _unsupported(term: str, detail: str) -> "_native.NativeError":
    return _native.NativeError(f"cfg.commands term {term!r}: {detail}.  The commands run in a HIP kernel (no host "
                               f"fallback); supported: {CM.SUPPORTED}")


def _tuple(x, k: int, term: str, what: str) -> tuple:
    try:
        vals = tuple(x)
    except TypeError:
        raise _unsupported(term, f"{what} = {x!r} is not a tuple of {k} numbers") from None
    if len(vals) != k or not all(is_number(v) for v in vals):
        raise _unsupported(term, f"{what} = {x!r} is not a tuple of {k} numbers")
    return tuple(float(v) for v in vals)


def _range(x, term: str, what: str) -> tuple[float, float]:
    lo, hi = _tuple(x, 2, term, what)
    if hi < lo:
        raise _unsupported(term, f"{what} = {x!r} has hi < lo")
    return lo, hi


def _prob(x, term: str, what: str) -> np.float32:
    if not is_number(x):
        raise _unsupported(term, f"{what} = {x!r} is not a number")
    return np.float32(x)


def term_row(name: str, cfg, step_dt: float) -> np.ndarray:
    """The as_command_term_t of a term as 21 float32 words (the first two hold int32 bits: kind, heading); raises
    NativeError, naming the term and the reason, for a term the kernel does not serve, and ValueError / a warning
    for the reference's two constructor checks (velocity_command.py:62-71).

    Every constant is formed as the reference forms it: a range reaches ``uniform_`` as two Python floats that
    torch rounds to float32 before it subtracts them; ``max_command_step`` is a Python double division, rounded to
    float32 where it meets the tensor; a probability, the stiffness and the clip bounds are rounded to float32 by
    the comparison, the multiply and the clip they enter."""
    f = np.float32
    if isinstance(cfg, CM.NullCommandCfg):
        raise _unsupported(name, "NullCommandCfg has no command to serve and never resamples (its resampling_time_range "
                                 "is infinite): leave the entry out or set it to None")
    if not isinstance(cfg, CM.UniformVelocityCommandCfg):
        raise _unsupported(name, f"{type(cfg).__name__} is not a served command term (the pose commands need env "
                                 f"origins or a body target)")
    normal = isinstance(cfg, CM.NormalVelocityCommandCfg)
    ranges = cfg.ranges
    if ranges is CM.MISSING or ranges is None:
        raise _unsupported(name, "ranges is not set")
    if not normal:
        heading = getattr(ranges, "heading", None)
        if cfg.heading_command and heading is None:  # velocity_command.py:62-66
            raise ValueError("The velocity command has heading commands active (heading_command=True) but the "
                             "`ranges.heading` parameter is set to None.")
        if heading and not cfg.heading_command:  # velocity_command.py:67-71
            warnings.warn(f"The velocity command has the 'ranges.heading' attribute set to '{heading}' but the "
                          f"heading command is not active. Consider setting the flag for the heading command to True.")
    if cfg.asset_name != "robot":
        raise _unsupported(name, f"asset_name = {cfg.asset_name!r} is not 'robot' (the command reads the root state "
                                 f"of the env's articulation)")
    rt = cfg.resampling_time_range
    if rt is CM.MISSING:
        raise _unsupported(name, "resampling_time_range is not set")
    t_lo, t_hi = _range(rt, name, "resampling_time_range")
    if not (math.isfinite(t_lo) and math.isfinite(t_hi)):
        raise _unsupported(name, f"resampling_time_range = {rt!r} is not finite (the reference's uniform_ gives NaN "
                                 f"timers for it)")
    row = np.zeros(_native.COMMAND_TERM_WORDS, f)
    ints = row[:2].view(np.int32)
    ints[0] = _native.COMMAND_NORMAL if normal else _native.COMMAND_UNIFORM
    row[2] = f(t_lo)
    row[3] = f(t_hi) - f(t_lo)
    if normal:
        mean = _tuple(getattr(ranges, "mean_vel", None), 3, name, "ranges.mean_vel")
        std = _tuple(getattr(ranges, "std_vel", None), 3, name, "ranges.std_vel")
        zero = _tuple(getattr(ranges, "zero_prob", None), 3, name, "ranges.zero_prob")
        if min(std) < 0:
            raise _unsupported(name, f"ranges.std_vel = {std!r} has a negative entry")
        row[4:7], row[8:11], row[17:20] = mean, std, zero
    else:
        keys = ("lin_vel_x", "lin_vel_y", "ang_vel_z") + (("heading",) if cfg.heading_command else ())
        for k, key in enumerate(keys):
            lo, hi = _range(getattr(ranges, key, None), name, f"ranges.{key}")
            row[4 + k] = f(lo)
            row[8 + k] = f(hi) - f(lo)
        ints[1] = 1 if cfg.heading_command else 0
        row[12], row[13] = (f(v) for v in _range(ranges.ang_vel_z, name, "ranges.ang_vel_z"))
        if not is_number(cfg.heading_control_stiffness):
            raise _unsupported(name, f"heading_control_stiffness = {cfg.heading_control_stiffness!r} is not a number")
        row[14] = f(cfg.heading_control_stiffness)
        row[15] = _prob(cfg.rel_heading_envs, name, "rel_heading_envs")
    row[16] = _prob(cfg.rel_standing_envs, name, "rel_standing_envs")
    with np.errstate(divide="ignore"):
        row[20] = f(np.float64(t_hi) / np.float64(step_dt))  # _update_metrics: a Python division, then float32
    if not np.isfinite(row[2:20]).all():
        raise _unsupported(name, "a range is not finite in float32")
    return row


class CommandTerms(RowTerms):
    """The host side of cfg.commands: names, cfgs and descriptor rows, checked (no device needed).  None entries
    are skipped (command_manager.py:409-410)."""

    NOUN, TERM_TYPE, WORDS = "command", CM.CommandTermCfg, _native.COMMAND_TERM_WORDS
    LIMIT = ("AS_MAX_COMMAND_TERMS", _native.MAX_COMMAND_TERMS)

    def __init__(self, commands, step_dt: float):
        self.step_dt = float(step_dt)
        super().__init__(commands)

    def row(self, name: str, cfg) -> np.ndarray:
        return term_row(name, cfg, self.step_dt)


class EnvCommands(DeviceState):
    """The commands side of a DirectRLEnv: term descriptors, the terms' per-env state and the stream counter."""

    STATE_KEYS = ("command_t", "command_time_left", "command_vel_b", "command_heading_target", "command_flags",
                  "command_counter", "command_metrics", "command_last_metrics")

    def __init__(self, cfg, n: int, device, seed: int, step_dt: float):
        self.n, self.device, self.seed = n, device, int(seed)
        self.dt = float(np.float32(step_dt))
        self.terms = CommandTerms(cfg.commands, step_dt)
        k = len(self.terms.names)
        z = lambda *shape, dtype=torch.float32: torch.zeros(*shape, dtype=dtype, device=device)  # noqa: E731
        self.desc = torch.as_tensor(self.terms.rows.copy(), device=device)
        self.vel = z(k, 3, n)
        self.heading_target = z(k, n)
        self.flags = z(k, _native.COMMAND_FLAG_ROWS, n, dtype=torch.uint8)
        self.time_left = z(k, n)
        self.counter = z(k, n, dtype=torch.int32)
        self.metrics = z(k, _native.COMMAND_METRIC_ROWS, n)
        self.last_metrics = z(k, _native.COMMAND_METRIC_ROWS, n)
        self.t = z(n, dtype=torch.int32)

    @staticmethod
    def wanted(cfg) -> bool:
        return getattr(cfg, "commands", None) is not None

    def _state_args(self):
        return (self.vel, self.heading_target, self.flags, self.time_left, self.counter, self.metrics,
                self.last_metrics, self.t)

    def apply(self, root_quat, root_lin, root_ang, terminated, truncated, env_offset: int, stream, dt=None) -> None:
        """The reset of the envs the step reset, then CommandManager.compute(dt), one launch."""
        if not len(self.terms.names):
            return
        _native.commands_step(self.desc, root_quat, root_lin, root_ang, *self._state_args(),
                              self.dt if dt is None else float(np.float32(dt)), reset=terminated, reset2=truncated,
                              seed=self.seed, env_offset=env_offset, stream=stream)

    def reset(self, mask, env_offset: int, stream) -> None:
        """CommandManager.reset(env_ids) without the logged means, for the envs of a uint8 / bool mask (None: all)."""
        if not len(self.terms.names):
            return
        if mask is not None:
            mask = u8(mask.to(self.device).reshape(self.n))
        _native.commands_reset(self.desc, *self._state_args(), mask=mask, seed=self.seed, env_offset=env_offset,
                               stream=stream)

    def set_term_cfg(self, term_name: str, cfg) -> None:
        k = self.terms.set(term_name, cfg)
        self.desc[k].copy_(torch.as_tensor(self.terms.rows[k].copy()))

    def refresh(self) -> None:
        """Rebuild every descriptor from the cfgs as they now stand (after an in-place range edit)."""
        for name, cfg in zip(self.terms.names, self.terms.cfgs):
            self.set_term_cfg(name, cfg)

    # ---- state (get_state / set_state of the envs)
    def tensors(self) -> dict:
        return dict(zip(self.STATE_KEYS, (self.t, self.time_left, self.vel, self.heading_target, self.flags,
                                          self.counter, self.metrics, self.last_metrics)))


class CommandTermView:
    """A term of ``env.command_manager``: the caller-visible attributes of the reference's velocity command terms
    over the device rows.  ``command`` / ``vel_command_b`` is the (N, 3) transposed view of the term's field-major
    (3, N) rows -- the same storage, not contiguous; the masks are bool views; ``command_counter`` is int32 (the
    reference's is int64)."""

    def __init__(self, cmds: EnvCommands, k: int):
        self._c, self._k = cmds, k

    cfg = property(lambda self: self._c.terms.cfgs[self._k])
    vel_command_b = property(lambda self: self._c.vel[self._k].T)
    command = vel_command_b
    heading_target = property(lambda self: self._c.heading_target[self._k])
    is_heading_env = property(lambda self: self._c.flags[self._k, 0].view(torch.bool))
    is_standing_env = property(lambda self: self._c.flags[self._k, 1].view(torch.bool))
    is_zero_vel_x_env = property(lambda self: self._c.flags[self._k, 2].view(torch.bool))
    is_zero_vel_y_env = property(lambda self: self._c.flags[self._k, 3].view(torch.bool))
    is_zero_vel_yaw_env = property(lambda self: self._c.flags[self._k, 4].view(torch.bool))
    time_left = property(lambda self: self._c.time_left[self._k])
    command_counter = property(lambda self: self._c.counter[self._k])

    @property
    def metrics(self) -> dict[str, torch.Tensor]:
        return {m: self._c.metrics[self._k, j] for j, m in enumerate(METRIC_NAMES)}

    @property
    def last_episode_metrics(self) -> dict[str, torch.Tensor]:
        """Per env, the metrics its last reset took a snapshot of (the reference logs their mean over the reset
        envs into extras; a captured step cannot, so the rows are the served form)."""
        return {m: self._c.last_metrics[self._k, j] for j, m in enumerate(METRIC_NAMES)}

    def __str__(self) -> str:
        cfg = self.cfg
        normal = isinstance(cfg, CM.NormalVelocityCommandCfg)
        msg = f"{'Normal' if normal else 'Uniform'}VelocityCommand:\n"
        msg += f"\tCommand dimension: {tuple(self.command.shape[1:])}\n"
        msg += f"\tResampling time range: {cfg.resampling_time_range}\n"
        if not normal:
            msg += f"\tHeading command: {cfg.heading_command}\n"
            if cfg.heading_command:
                msg += f"\tHeading probability: {cfg.rel_heading_envs}\n"
        msg += f"\tStanding probability: {cfg.rel_standing_envs}"
        return msg


class CommandManagerView:
    """``env.command_manager``: the caller-visible surface of the reference's ``CommandManager``
    (command_manager.py:225-394) over the device state."""

    def __init__(self, cmds: EnvCommands, env):
        self._c, self._env = cmds, env
        self._terms = {name: CommandTermView(cmds, k) for k, name in enumerate(cmds.terms.names)}

    @property
    def active_terms(self) -> list[str]:
        return list(self._terms)

    def get_term(self, name: str) -> CommandTermView:
        return self._terms[name]

    def get_command(self, name: str) -> torch.Tensor:
        return self._terms[name].command

    def get_term_cfg(self, name: str):
        return self._terms[name].cfg

    def set_term_cfg(self, name: str, cfg) -> None:
        """Replace a term's cfg.  The new constants are written into the device descriptors, so they hold from the
        next launch on, in a captured graph too; the running commands and timers are kept."""
        self._c.set_term_cfg(name, cfg)

    def refresh(self) -> None:
        """Take over in-place edits of the terms' cfgs (a curriculum widening ``cfg.ranges.lin_vel_x``, say): the
        reference reads the cfg at every resample, the kernel reads the descriptors this rewrites."""
        self._c.refresh()

    def compute(self, dt: float) -> None:
        """CommandManager.compute(dt) on the env's root state as it stands: one launch, no reset."""
        s = self._env.state
        self._c.apply(s["root_quat"], s["root_lin"], s["root_ang"], None, None, self._env._noise_offset(),
                      self._env._noise_stream(), dt=dt)

    def reset(self, env_ids=None) -> dict[str, float]:
        """CommandManager.reset(env_ids): the means of the terms' metrics over ``env_ids`` under
        ``Metrics/<term>/<metric>`` (a host read), then the reset of those envs, one launch."""
        c = self._c
        sel = slice(None) if env_ids is None else torch.as_tensor(env_ids, device=c.device).long()
        extras = {f"Metrics/{name}/{m}": torch.mean(c.metrics[k, j][sel]).item()
                  for k, name in enumerate(c.terms.names) for j, m in enumerate(METRIC_NAMES)}
        mask = None
        if env_ids is not None:
            mask = torch.zeros(c.n, dtype=torch.uint8, device=c.device)
            mask[sel] = 1
        c.reset(mask, self._env._noise_offset(), self._env._noise_stream())
        return extras

    def __str__(self) -> str:
        names = self.active_terms
        msg = f"<CommandManager> contains {len(names)} active terms.\n"
        rows = [(str(i), k, "NormalVelocityCommand" if isinstance(t.cfg, CM.NormalVelocityCommandCfg)
                 else "UniformVelocityCommand") for i, (k, t) in enumerate(self._terms.items())]
        head = ("Index", "Name", "Type")
        w = [max(len(r[j]) for r in rows + [head]) for j in range(3)]
        line = "+" + "+".join("-" * (x + 2) for x in w) + "+\n"
        total = len(line) - 3
        fmt = lambda r: "| " + " | ".join((r[0].center(w[0]), r[1].ljust(w[1]), r[2].center(w[2]))) + " |\n"  # noqa: E731
        msg += "+" + "-" * total + "+\n" + "|" + "Active Command Terms".center(total) + "|\n"
        msg += line + fmt(head) + line + "".join(fmt(r) for r in rows) + line
        return msg
