"""Reward configuration -- ``RewardTermCfg`` of ``isaaclab.managers`` and the reward functions of
``isaaclab.envs.mdp`` and of the velocity task's ``mdp``, same names, fields and defaults, for ``cfg.rewards`` of the
envs.

The weighted sum itself is computed on the device (``k_rewards_step``, csrc/reward_kernels.h): a term's ``func``
names which of the built-in term functions it asks for, and the env raises at construction for anything it does not
serve.  Each function below is also an ordinary callable: it returns the torch expression over the env's views, the
composition the kernel replaces, on the same values the kernel reads.
"""

from __future__ import annotations

import re
from dataclasses import dataclass, field
from typing import Callable

import torch

from .events import SceneEntityCfg
from .noise import MISSING
from .observations import _joint_ids, _robot


@dataclass
class RewardTermCfg:
    """manager_term_cfg.py ``RewardTermCfg`` (with ``ManagerTermBaseCfg``'s ``func`` / ``params``)."""

    func: Callable = MISSING
    params: dict = field(default_factory=dict)
    weight: float = MISSING


_ROBOT = SceneEntityCfg("robot")


def resolve_body_ids(sensor_cfg, body_names: list, what: str):
    """The bodies of a sensor a cfg selects, as a list of indices into the sensor's bodies -- None: all of them.
    ``body_names`` are regular expressions matched against the whole name, in body order (``preserve_order``: in the
    order given)."""
    names = getattr(sensor_cfg, "body_names", None)
    ids = getattr(sensor_cfg, "body_ids", slice(None))
    if names is not None:
        names = [names] if isinstance(names, str) else list(names)
        hit = [[k for k, bn in enumerate(body_names) if re.fullmatch(p, bn)] for p in names]
        missing = [p for p, h in zip(names, hit) if not h]
        if missing:
            raise ValueError(f"{what}: body_names {missing} match no body of {body_names}")
        flat = [k for h in hit for k in h]
        return flat if getattr(sensor_cfg, "preserve_order", False) else sorted(set(flat))
    if isinstance(ids, slice):
        return None if ids == slice(None) else list(range(len(body_names)))[ids]
    ids = [int(k) for k in (ids.tolist() if hasattr(ids, "tolist") else ids)]
    if any(k < 0 or k >= len(body_names) for k in ids):
        raise ValueError(f"{what}: body_ids {ids} outside [0, {len(body_names)})")
    return ids


def _sensor(env, sensor_cfg):
    """The contact sensor a cfg names: a sensor of the scene, or the env's own foot sensor of that name."""
    name = sensor_cfg.name
    s = env.scene.sensors.get(name) if hasattr(env.scene, "sensors") else None
    s = getattr(env, name, None) if s is None else s
    if s is None or not hasattr(s, "body_names"):
        raise KeyError(f"sensor_cfg names the sensor {name!r}, which the env does not have")
    return s


def _body_ids(sensor, sensor_cfg):
    ids = resolve_body_ids(sensor_cfg, sensor.body_names, "body selection")
    return slice(None) if ids is None else ids


def _action(env):
    return env.actions


# ---- general
def is_alive(env):
    """rewards.py ``is_alive``: 1 for an env the step did not terminate."""
    return (~env.reset_terminated).float()


def is_terminated(env):
    """rewards.py ``is_terminated``: 1 for an env the step terminated (time-outs are not terminations)."""
    return env.reset_terminated.float()


# ---- root penalties
def lin_vel_z_l2(env, asset_cfg: SceneEntityCfg = _ROBOT):
    return torch.square(_robot(env).root_lin_vel_b[:, 2])


def ang_vel_xy_l2(env, asset_cfg: SceneEntityCfg = _ROBOT):
    return torch.sum(torch.square(_robot(env).root_ang_vel_b[:, :2]), dim=1)


def flat_orientation_l2(env, asset_cfg: SceneEntityCfg = _ROBOT):
    return torch.sum(torch.square(_robot(env).projected_gravity_b[:, :2]), dim=1)


def base_height_l2(env, target_height: float, asset_cfg: SceneEntityCfg = _ROBOT, sensor_cfg=None):
    if sensor_cfg is not None:
        raise NotImplementedError("base_height_l2 with a sensor_cfg is not served")
    return torch.square(_robot(env).root_pos_w[:, 2] - target_height)


# ---- joint penalties
def joint_vel_l1(env, asset_cfg: SceneEntityCfg = _ROBOT):
    return torch.sum(torch.abs(_robot(env).joint_vel[:, _joint_ids(env, asset_cfg)]), dim=1)


def joint_vel_l2(env, asset_cfg: SceneEntityCfg = _ROBOT):
    return torch.sum(torch.square(_robot(env).joint_vel[:, _joint_ids(env, asset_cfg)]), dim=1)


def joint_acc_l2(env, asset_cfg: SceneEntityCfg = _ROBOT):
    return torch.sum(torch.square(_robot(env).joint_acc[:, _joint_ids(env, asset_cfg)]), dim=1)


def joint_deviation_l1(env, asset_cfg: SceneEntityCfg = _ROBOT):
    ids = _joint_ids(env, asset_cfg)
    return torch.sum(torch.abs(_robot(env).joint_pos[:, ids] - _robot(env).default_joint_pos[:, ids]), dim=1)


def joint_pos_limits(env, asset_cfg: SceneEntityCfg = _ROBOT):
    ids = _joint_ids(env, asset_cfg)
    d = _robot(env)
    out = -(d.joint_pos[:, ids] - d.soft_joint_pos_limits[:, ids, 0]).clip(max=0.0)
    out += (d.joint_pos[:, ids] - d.soft_joint_pos_limits[:, ids, 1]).clip(min=0.0)
    return torch.sum(out, dim=1)


# ---- action penalties
def action_rate_l2(env):
    """rewards.py ``action_rate_l2``: against the reward manager's ``prev_actions`` (the action of the env's last
    step, 0 after its reset)."""
    return torch.sum(torch.square(_action(env) - env.reward_manager.prev_actions), dim=1)


def action_l2(env):
    return torch.sum(torch.square(_action(env)), dim=1)


# ---- contact sensor
def undesired_contacts(env, threshold: float, sensor_cfg: SceneEntityCfg):
    sensor = _sensor(env, sensor_cfg)
    f = sensor.data.net_forces_w_history
    is_contact = torch.max(torch.norm(f[:, :, _body_ids(sensor, sensor_cfg)], dim=-1), dim=1)[0] > threshold
    return torch.sum(is_contact, dim=1)


def contact_forces(env, threshold: float, sensor_cfg: SceneEntityCfg):
    sensor = _sensor(env, sensor_cfg)
    f = sensor.data.net_forces_w_history
    violation = torch.max(torch.norm(f[:, :, _body_ids(sensor, sensor_cfg)], dim=-1), dim=1)[0] - threshold
    return torch.sum(violation.clip(min=0.0), dim=1)


# ---- the velocity task's terms
def feet_air_time(env, command_name: str, sensor_cfg: SceneEntityCfg, threshold: float):
    sensor = _sensor(env, sensor_cfg)
    ids = _body_ids(sensor, sensor_cfg)
    first_contact = sensor.compute_first_contact(env.step_dt)[:, ids]
    last_air_time = sensor.data.last_air_time[:, ids]
    reward = torch.sum((last_air_time - threshold) * first_contact, dim=1)
    reward *= torch.norm(env.command_manager.get_command(command_name)[:, :2], dim=1) > 0.1
    return reward


def feet_air_time_positive_biped(env, command_name: str, threshold: float, sensor_cfg: SceneEntityCfg):
    sensor = _sensor(env, sensor_cfg)
    ids = _body_ids(sensor, sensor_cfg)
    air_time = sensor.data.current_air_time[:, ids]
    contact_time = sensor.data.current_contact_time[:, ids]
    in_contact = contact_time > 0.0
    in_mode_time = torch.where(in_contact, contact_time, air_time)
    single_stance = torch.sum(in_contact.int(), dim=1) == 1
    reward = torch.min(torch.where(single_stance.unsqueeze(-1), in_mode_time, 0.0), dim=1)[0]
    reward = torch.clamp(reward, max=threshold)
    reward *= torch.norm(env.command_manager.get_command(command_name)[:, :2], dim=1) > 0.1
    return reward


def track_lin_vel_xy_exp(env, std: float, command_name: str, asset_cfg: SceneEntityCfg = _ROBOT):
    err = torch.sum(torch.square(env.command_manager.get_command(command_name)[:, :2]
                                 - _robot(env).root_lin_vel_b[:, :2]), dim=1)
    return torch.exp(-err / std**2)


def track_ang_vel_z_exp(env, std: float, command_name: str, asset_cfg: SceneEntityCfg = _ROBOT):
    err = torch.square(env.command_manager.get_command(command_name)[:, 2] - _robot(env).root_ang_vel_b[:, 2])
    return torch.exp(-err / std**2)


def track_ang_vel_z_world_exp(env, command_name: str, std: float, asset_cfg: SceneEntityCfg = _ROBOT):
    err = torch.square(env.command_manager.get_command(command_name)[:, 2] - _robot(env).root_ang_vel_w[:, 2])
    return torch.exp(-err / std**2)


def _yaw_quat(quat):
    """math.py ``yaw_quat``: the yaw component of (w, x, y, z) quaternions, normalised."""
    qw, qx, qy, qz = quat[:, 0], quat[:, 1], quat[:, 2], quat[:, 3]
    yaw = torch.atan2(2 * (qw * qz + qx * qy), 1 - 2 * (qy * qy + qz * qz))
    out = torch.zeros_like(quat)
    out[:, 3] = torch.sin(yaw / 2)
    out[:, 0] = torch.cos(yaw / 2)
    return out / out.norm(p=2, dim=-1).clamp(min=1e-9, max=None).unsqueeze(-1)


def track_lin_vel_xy_yaw_frame_exp(env, std: float, command_name: str, asset_cfg: SceneEntityCfg = _ROBOT):
    d = _robot(env)
    vel_yaw = d._rotate_inverse(_yaw_quat(d.root_quat_w), d.root_lin_vel_w[:, :3])
    err = torch.sum(torch.square(env.command_manager.get_command(command_name)[:, :2] - vel_yaw[:, :2]), dim=1)
    return torch.exp(-err / std**2)


def _refused(name: str, why: str):
    def fn(env, *args, **kwargs):
        raise NotImplementedError(f"{name} is not served: {why}")

    fn.__name__ = fn.__qualname__ = name
    fn.__doc__ = f"rewards.py ``{name}``: refused in cfg.rewards ({why})."
    return fn


REFUSED = {
    "joint_torques_l2": "the step keeps no applied torque",
    "applied_torque_limits": "the step keeps no applied torque",
    "joint_vel_limits": "the views have no soft joint velocity limits",
    "body_lin_acc_l2": "the step keeps no body accelerations",
    "feet_slide": "the body velocities are computed on demand, not kept by the step",
    "is_terminated_term": "there is no termination manager",
}
joint_torques_l2 = _refused("joint_torques_l2", REFUSED["joint_torques_l2"])
applied_torque_limits = _refused("applied_torque_limits", REFUSED["applied_torque_limits"])
joint_vel_limits = _refused("joint_vel_limits", REFUSED["joint_vel_limits"])
body_lin_acc_l2 = _refused("body_lin_acc_l2", REFUSED["body_lin_acc_l2"])
feet_slide = _refused("feet_slide", REFUSED["feet_slide"])
is_terminated_term = _refused("is_terminated_term", REFUSED["is_terminated_term"])

SERVED = ("is_alive", "is_terminated", "lin_vel_z_l2", "ang_vel_xy_l2", "flat_orientation_l2", "base_height_l2",
          "joint_vel_l1", "joint_vel_l2", "joint_deviation_l1", "joint_pos_limits", "joint_acc_l2", "action_l2",
          "action_rate_l2", "undesired_contacts", "contact_forces", "feet_air_time", "feet_air_time_positive_biped",
          "track_lin_vel_xy_exp", "track_ang_vel_z_exp", "track_ang_vel_z_world_exp",
          "track_lin_vel_xy_yaw_frame_exp")
SUPPORTED = ", ".join(SERVED) + "; weight a float or an int"
