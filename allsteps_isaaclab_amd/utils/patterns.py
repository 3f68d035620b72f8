"""Ray patterns of the ray-caster sensor -- ``isaaclab.sensors.patterns``: ``GridPatternCfg`` and ``grid_pattern``,
same names, fields, defaults and results (``ray_caster/patterns/patterns.py:16-58``, ``patterns_cfg.py``).

A pattern cfg's ``func(cfg, device)`` returns the local ray starts and directions, two ``(R, 3)`` tensors: the
reference's protocol, so any pattern cfg written for it can be handed to ``RayCasterCfg.pattern_cfg``.  Only the
grid ships; the camera, lidar and bpearl patterns are out of scope.
"""

from __future__ import annotations

from dataclasses import dataclass
from typing import Any, Callable

import torch

from .noise import MISSING


def grid_pattern(cfg: "GridPatternCfg", device) -> tuple[torch.Tensor, torch.Tensor]:
    """Parallel rays on a regular 2-D grid from ``-size / 2`` to ``size / 2`` in steps of ``resolution``.  The
    coordinates come from the same torch calls as the reference's (an ``arange`` whose end is ``size / 2 + 1e-9``,
    a ``meshgrid`` indexed by the ordering), so the rays are bit-equal to its."""
    if cfg.ordering not in ["xy", "yx"]:
        raise ValueError(f"Ordering must be 'xy' or 'yx'. Received: '{cfg.ordering}'.")
    if cfg.resolution <= 0:
        raise ValueError(f"Resolution must be greater than 0. Received: '{cfg.resolution}'.")
    axes = [torch.arange(start=-s / 2, end=s / 2 + 1.0e-9, step=cfg.resolution, device=device) for s in cfg.size[:2]]
    gx, gy = torch.meshgrid(axes[0], axes[1], indexing="xy" if cfg.ordering == "xy" else "ij")
    starts = torch.zeros(gx.numel(), 3, device=device)
    starts[:, 0] = gx.flatten()
    starts[:, 1] = gy.flatten()
    directions = torch.zeros_like(starts)
    directions[..., :] = torch.tensor(list(cfg.direction), device=device)
    return starts, directions


@dataclass
class PatternBaseCfg:
    """patterns_cfg.py ``PatternBaseCfg``: ``func(cfg, device) -> (starts (R, 3), directions (R, 3))``."""

    func: Callable = MISSING


@dataclass
class GridPatternCfg(PatternBaseCfg):
    """patterns_cfg.py ``GridPatternCfg``."""

    func: Callable = grid_pattern
    resolution: float = MISSING
    size: Any = MISSING  # (length, width)
    direction: tuple = (0.0, 0.0, -1.0)
    ordering: str = "xy"  # "xy" | "yx": which grid index runs fastest
