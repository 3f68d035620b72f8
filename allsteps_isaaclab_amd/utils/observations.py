"""Observation configuration -- ``ObservationTermCfg`` / ``ObservationGroupCfg`` of ``isaaclab.managers`` and the
observation functions of ``isaaclab.envs.mdp``, same names, fields and defaults, for ``cfg.observations`` of the envs.

The groups themselves are assembled on the device (``k_observations``, csrc/observation_kernels.h): a term's
``func`` names which of the built-in term functions it asks for, and the env raises at construction for anything it
does not serve.  Each function below is also an ordinary callable: it returns the torch expression over the env's
views, the same values the kernel reads (``generated_commands``, ``height_scan`` and the ``imu_*`` functions live in
``utils/commands.py`` and ``utils/sensors.py``).
"""

from __future__ import annotations

import re
from dataclasses import dataclass, field
from typing import Any, Callable

from .events import SceneEntityCfg
from .noise import MISSING


@dataclass
class ObservationTermCfg:
    """manager_term_cfg.py ``ObservationTermCfg`` (with ``ManagerTermBaseCfg``'s ``func`` / ``params``)."""

    func: Callable = MISSING
    params: dict = field(default_factory=dict)
    modifiers: Any = None
    noise: Any = None
    clip: Any = None  # (lo, hi)
    scale: Any = None  # float, or a tuple of the term's width
    history_length: int = 0
    flatten_history_dim: bool = True


@dataclass
class ObservationGroupCfg:
    """manager_term_cfg.py ``ObservationGroupCfg``: the terms are the other attributes of an instance or of a
    subclass (or the entries of a dict with these four keys beside them)."""

    concatenate_terms: bool = True
    enable_corruption: bool = False
    history_length: Any = None  # int | None: set, it overrides the terms'
    flatten_history_dim: bool = True


GROUP_SETTINGS = ("concatenate_terms", "enable_corruption", "history_length", "flatten_history_dim")

_ROBOT = SceneEntityCfg("robot")


def resolve_joint_ids(asset_cfg, joint_names: list, what: str):
    """The joints an asset cfg selects, as a list of indices -- None: all of them.  ``joint_names`` are regular
    expressions matched against the whole name, in joint order (``preserve_order``: in the order given)."""
    names = getattr(asset_cfg, "joint_names", None)
    ids = getattr(asset_cfg, "joint_ids", slice(None))
    if names is not None:
        names = [names] if isinstance(names, str) else list(names)
        hit = [[k for k, jn in enumerate(joint_names) if re.fullmatch(p, jn)] for p in names]
        missing = [p for p, h in zip(names, hit) if not h]
        if missing:
            raise ValueError(f"{what}: joint_names {missing} match no joint of {joint_names}")
        flat = [k for h in hit for k in h]
        return flat if getattr(asset_cfg, "preserve_order", False) else sorted(set(flat))
    if isinstance(ids, slice):
        return None if ids == slice(None) else list(range(len(joint_names)))[ids]
    ids = [int(k) for k in (ids.tolist() if hasattr(ids, "tolist") else ids)]
    if any(k < 0 or k >= len(joint_names) for k in ids):
        raise ValueError(f"{what}: joint_ids {ids} outside [0, {len(joint_names)})")
    return ids


def _robot(env):
    return env.robot.data


def _joint_ids(env, asset_cfg):
    """The joint selection of an asset cfg as something that indexes a (N, joints) view."""
    ids = resolve_joint_ids(asset_cfg, _robot(env).joint_names, "joint selection")
    return slice(None) if ids is None else ids


def base_pos_z(env, asset_cfg: SceneEntityCfg = _ROBOT):
    """observations.py ``base_pos_z``: root height in the simulation world frame -- (N, 1)."""
    return _robot(env).root_pos_w[:, 2].unsqueeze(-1)


def base_lin_vel(env, asset_cfg: SceneEntityCfg = _ROBOT):
    """observations.py ``base_lin_vel``: root linear velocity in the root frame -- (N, 3)."""
    return _robot(env).root_lin_vel_b


def base_ang_vel(env, asset_cfg: SceneEntityCfg = _ROBOT):
    """observations.py ``base_ang_vel``: root angular velocity in the root frame -- (N, 3)."""
    return _robot(env).root_ang_vel_b


def projected_gravity(env, asset_cfg: SceneEntityCfg = _ROBOT):
    """observations.py ``projected_gravity``: the gravity direction in the root frame -- (N, 3)."""
    return _robot(env).projected_gravity_b


def root_pos_w(env, asset_cfg: SceneEntityCfg = _ROBOT):
    """observations.py ``root_pos_w``: root position relative to the env's origin -- (N, 3).  The envs' state is
    env-local already, so this is ``robot.data.root_pos_w`` as it is."""
    return _robot(env).root_pos_w


def root_quat_w(env, make_quat_unique: bool = False, asset_cfg: SceneEntityCfg = _ROBOT):
    """observations.py ``root_quat_w``: root orientation (w, x, y, z), with a non-negative real part when
    ``make_quat_unique`` -- (N, 4)."""
    import torch

    q = _robot(env).root_quat_w
    return torch.where(q[..., 0:1] < 0, -q, q) if make_quat_unique else q


def root_lin_vel_w(env, asset_cfg: SceneEntityCfg = _ROBOT):
    """observations.py ``root_lin_vel_w`` -- (N, 3)."""
    return _robot(env).root_lin_vel_w


def root_ang_vel_w(env, asset_cfg: SceneEntityCfg = _ROBOT):
    """observations.py ``root_ang_vel_w`` -- (N, 3)."""
    return _robot(env).root_ang_vel_w


def joint_pos(env, asset_cfg: SceneEntityCfg = _ROBOT):
    """observations.py ``joint_pos``: the selected joints' positions -- (N, joints)."""
    return _robot(env).joint_pos[:, _joint_ids(env, asset_cfg)]


def joint_pos_rel(env, asset_cfg: SceneEntityCfg = _ROBOT):
    """observations.py ``joint_pos_rel``: the positions relative to the default joint positions."""
    ids = _joint_ids(env, asset_cfg)
    return _robot(env).joint_pos[:, ids] - _robot(env).default_joint_pos[:, ids]


def joint_pos_limit_normalized(env, asset_cfg: SceneEntityCfg = _ROBOT):
    """observations.py ``joint_pos_limit_normalized``: ``scale_transform`` of the positions by the soft limits."""
    ids = _joint_ids(env, asset_cfg)
    lim = _robot(env).soft_joint_pos_limits
    lower, upper = lim[:, ids, 0], lim[:, ids, 1]
    offset = (lower + upper) * 0.5
    return 2 * (_robot(env).joint_pos[:, ids] - offset) / (upper - lower)


def joint_vel(env, asset_cfg: SceneEntityCfg = _ROBOT):
    """observations.py ``joint_vel``: the selected joints' velocities -- (N, joints)."""
    return _robot(env).joint_vel[:, _joint_ids(env, asset_cfg)]


def joint_vel_rel(env, asset_cfg: SceneEntityCfg = _ROBOT):
    """observations.py ``joint_vel_rel``: the velocities relative to the default joint velocities."""
    ids = _joint_ids(env, asset_cfg)
    return _robot(env).joint_vel[:, ids] - _robot(env).default_joint_vel[:, ids]


def last_action(env, action_name: Any = None):
    """observations.py ``last_action``: the last action as ``env.actions`` has it (after the action noise model)
    -- (N, actions).  In a group the kernel reads 0 for an env the step reset, as ``action_manager.reset`` leaves
    it."""
    if action_name is not None:
        raise NotImplementedError("last_action: the direct-workflow envs have one action term (action_name=None)")
    return env.actions


def _refused(name: str, why: str):
    def fn(env, *args, **kwargs):
        raise NotImplementedError(f"{name} is not served: {why}")

    fn.__name__ = fn.__qualname__ = name
    fn.__doc__ = f"observations.py ``{name}``: refused in cfg.observations ({why})."
    return fn


body_incoming_wrench = _refused("body_incoming_wrench", "the step keeps no joint reaction wrenches")
image_features = _refused("image_features", "a pretrained network on the host is no device term")

SUPPORTED = ("base_pos_z, base_lin_vel, base_ang_vel, projected_gravity, root_pos_w, root_quat_w, root_lin_vel_w, "
             "root_ang_vel_w, joint_pos, joint_pos_rel, joint_pos_limit_normalized, joint_vel, joint_vel_rel, "
             "last_action, generated_commands, height_scan, imu_orientation, imu_ang_vel, imu_lin_acc; noise a "
             "ConstantNoiseCfg / UniformNoiseCfg / GaussianNoiseCfg; clip (lo, hi); scale a float or a tuple")
