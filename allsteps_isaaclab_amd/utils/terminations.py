"""Termination configuration -- ``TerminationTermCfg`` of ``isaaclab.managers`` and the termination functions of
``isaaclab.envs.mdp``, same names, fields and defaults, for ``cfg.terminations`` of the envs.

The done flags themselves are computed on the device (``k_terminations_step``, csrc/termination_kernels.h): a term's
``func`` names which of the built-in term functions it asks for, and the env raises at construction for anything it
does not serve.  Each function below is also an ordinary callable: it returns the torch expression over the env's
views, the composition the kernel replaces, on the same values the kernel reads.
"""

from __future__ import annotations

from dataclasses import dataclass, field
from typing import Callable

import torch

from .events import SceneEntityCfg
from .noise import MISSING
from .observations import _joint_ids, _robot
from .rewards import _body_ids, _sensor


@dataclass
class TerminationTermCfg:
    """manager_term_cfg.py ``TerminationTermCfg`` (with ``ManagerTermBaseCfg``'s ``func`` / ``params``)."""

    func: Callable = MISSING
    params: dict = field(default_factory=dict)
    time_out: bool = False


_ROBOT = SceneEntityCfg("robot")


# ---- MDP terminations
def time_out(env):
    """terminations.py ``time_out``: the episode length reached the maximum.  The step resets such an env in-kernel
    and its counter is 0 again when this is read, so the step's own truncated flag -- the same comparison, made
    before that reset -- is part of it."""
    return env.reset_time_outs | (env.episode_length_buf >= env.max_episode_length)


def command_resample(env, command_name: str, num_resamples: int = 1):
    command = env.command_manager.get_term(command_name)
    return torch.logical_and(command.time_left <= env.step_dt, command.command_counter == num_resamples)


# ---- root terminations
def bad_orientation(env, limit_angle: float, asset_cfg: SceneEntityCfg = _ROBOT):
    return torch.acos(-_robot(env).projected_gravity_b[:, 2]).abs() > limit_angle


def root_height_below_minimum(env, minimum_height: float, asset_cfg: SceneEntityCfg = _ROBOT):
    return _robot(env).root_pos_w[:, 2] < minimum_height


# ---- joint terminations
def joint_pos_out_of_limit(env, asset_cfg: SceneEntityCfg = _ROBOT):
    """terminations.py ``joint_pos_out_of_limit`` as documented: any of the selected joints outside its soft limits.
    (The reference's body reduces over all joints and then indexes the (N,) result with ``[:, joint_ids]``, which
    raises for every input.)"""
    ids = _joint_ids(env, asset_cfg)
    d = _robot(env)
    q, lim = d.joint_pos[:, ids], d.soft_joint_pos_limits[:, ids]
    return torch.logical_or(torch.any(q > lim[..., 1], dim=1), torch.any(q < lim[..., 0], dim=1))


def joint_pos_out_of_manual_limit(env, bounds: tuple, asset_cfg: SceneEntityCfg = _ROBOT):
    q = _robot(env).joint_pos[:, _joint_ids(env, asset_cfg)]
    return torch.logical_or(torch.any(q > bounds[1], dim=1), torch.any(q < bounds[0], dim=1))


def joint_vel_out_of_manual_limit(env, max_velocity: float, asset_cfg: SceneEntityCfg = _ROBOT):
    return torch.any(torch.abs(_robot(env).joint_vel[:, _joint_ids(env, asset_cfg)]) > max_velocity, dim=1)


# ---- contact sensor
def illegal_contact(env, threshold: float, sensor_cfg: SceneEntityCfg):
    sensor = _sensor(env, sensor_cfg)
    f = sensor.data.net_forces_w_history
    return torch.any(torch.max(torch.norm(f[:, :, _body_ids(sensor, sensor_cfg)], dim=-1), dim=1)[0] > threshold,
                     dim=1)


def _refused(name: str, why: str):
    def fn(env, *args, **kwargs):
        raise NotImplementedError(f"{name} is not served: {why}")

    fn.__name__ = fn.__qualname__ = name
    fn.__doc__ = f"terminations.py ``{name}``: refused in cfg.terminations ({why})."
    return fn


REFUSED = {
    "joint_effort_out_of_limit": "the step keeps no applied torque",
    "joint_vel_out_of_limit": "the views have no soft joint velocity limits",
}
joint_effort_out_of_limit = _refused("joint_effort_out_of_limit", REFUSED["joint_effort_out_of_limit"])
joint_vel_out_of_limit = _refused("joint_vel_out_of_limit", REFUSED["joint_vel_out_of_limit"])

SERVED = ("time_out", "command_resample", "bad_orientation", "root_height_below_minimum", "joint_pos_out_of_limit",
          "joint_pos_out_of_manual_limit", "joint_vel_out_of_manual_limit", "illegal_contact")
SUPPORTED = ", ".join(SERVED) + "; time_out a bool"
