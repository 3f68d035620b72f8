"""Command configuration -- ``CommandTermCfg`` of ``isaaclab.managers`` and ``UniformVelocityCommandCfg`` /
``NormalVelocityCommandCfg`` / ``NullCommandCfg`` of ``isaaclab.envs.mdp``, same names, fields and defaults, for
``cfg.commands`` of the envs, and the observation term ``generated_commands``.

The commands themselves run on the device (``k_commands_step``, csrc/command_kernels.h): a cfg's class names which
of the built-in command terms an entry asks for, and the env raises at construction for anything it does not
serve.  ``class_type`` is carried for code that reads it; there is no host implementation behind it.  The marker /
debug-visualisation fields are accepted and ignored (there is no viewport).
"""

from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Any

from .noise import MISSING


@dataclass
class CommandTermCfg:
    """manager_term_cfg.py ``CommandTermCfg``."""

    class_type: Any = MISSING
    resampling_time_range: tuple = MISSING
    debug_vis: bool = False


@dataclass
class NullCommandCfg(CommandTermCfg):
    """commands_cfg.py ``NullCommandCfg``: a term without a command, never resampled."""

    class_type: Any = "NullCommand"

    def __post_init__(self):
        self.resampling_time_range = (math.inf, math.inf)


@dataclass
class UniformVelocityCommandCfg(CommandTermCfg):
    """commands_cfg.py ``UniformVelocityCommandCfg``."""

    @dataclass
    class Ranges:
        lin_vel_x: tuple = MISSING
        lin_vel_y: tuple = MISSING
        ang_vel_z: tuple = MISSING
        heading: tuple | None = None

    class_type: Any = "UniformVelocityCommand"
    asset_name: str = MISSING
    heading_command: bool = False
    heading_control_stiffness: float = 1.0
    rel_standing_envs: float = 0.0
    rel_heading_envs: float = 1.0
    ranges: Any = MISSING
    goal_vel_visualizer_cfg: Any = None
    current_vel_visualizer_cfg: Any = None


@dataclass
class NormalVelocityCommandCfg(UniformVelocityCommandCfg):
    """commands_cfg.py ``NormalVelocityCommandCfg`` (no heading command)."""

    @dataclass
    class Ranges:
        mean_vel: tuple = MISSING
        std_vel: tuple = MISSING
        zero_prob: tuple = MISSING

    class_type: Any = "NormalVelocityCommand"
    heading_command: bool = False


def generated_commands(env, command_name: str):
    """observations.py ``generated_commands``: the command of the term ``command_name`` -- the same storage as
    ``env.command_manager.get_command(command_name)``, an (N, 3) view of the device rows."""
    return env.command_manager.get_command(command_name)


SUPPORTED = ("UniformVelocityCommandCfg(asset_name='robot', resampling_time_range=(lo, hi), ranges=Ranges(lin_vel_x, "
             "lin_vel_y, ang_vel_z[, heading]), heading_command, heading_control_stiffness, rel_heading_envs, "
             "rel_standing_envs) and NormalVelocityCommandCfg(asset_name='robot', resampling_time_range=(lo, hi), "
             "ranges=Ranges(mean_vel, std_vel, zero_prob), rel_standing_envs)")
