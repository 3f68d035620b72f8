"""Sensor configuration -- ``RayCasterCfg`` and ``patterns`` of ``isaaclab.sensors`` and the observation function
``height_scan`` of ``isaaclab.envs.mdp``, same names, fields and defaults, for ``cfg.height_scanner`` of the envs.

The rays are cast on the device (``k_ray_cast``, csrc/ray_caster_kernels.h) against the ground plane and the env's
stones; the env raises at construction for what that kernel does not serve (envs/ray_caster.py).
"""

from __future__ import annotations

from dataclasses import dataclass, field
from typing import Any

from . import patterns  # noqa: F401  (isaaclab.sensors.patterns)
from .noise import MISSING


@dataclass
class RayCasterCfg:
    """ray_caster_cfg.py ``RayCasterCfg`` with ``SensorBaseCfg``'s fields (sensor_base_cfg.py)."""

    @dataclass
    class OffsetCfg:
        """The sensor frame's pose in the frame of the body it is attached to."""

        pos: tuple = (0.0, 0.0, 0.0)
        rot: tuple = (1.0, 0.0, 0.0, 0.0)  # (w, x, y, z)

    prim_path: str = MISSING
    update_period: float = 0.0
    history_length: int = 0
    debug_vis: bool = False
    mesh_prim_paths: Any = MISSING  # list[str]
    offset: OffsetCfg = field(default_factory=OffsetCfg)
    attach_yaw_only: bool = MISSING
    pattern_cfg: Any = MISSING  # a patterns.PatternBaseCfg
    max_distance: float = 1e6
    drift_range: tuple = (0.0, 0.0)


def height_scan(env, sensor_cfg, offset: float = 0.5):
    """observations.py ``height_scan``: the sensor's height over every hit point, less ``offset`` -- (N, R)."""
    sensor = env.scene.sensors[sensor_cfg.name]
    return sensor.data.pos_w[:, 2].unsqueeze(1) - sensor.data.ray_hits_w[..., 2] - offset
