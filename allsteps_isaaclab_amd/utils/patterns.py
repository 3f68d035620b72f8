"""Ray patterns of the ray-caster sensors -- ``isaaclab.sensors.patterns``: ``GridPatternCfg`` / ``grid_pattern`` and
``PinholeCameraPatternCfg`` / ``pinhole_camera_pattern``, same names, fields, defaults and results
(``ray_caster/patterns/patterns.py``, ``patterns_cfg.py``).

A pattern cfg's ``func(cfg, device)`` returns the local ray starts and directions, two ``(R, 3)`` tensors: the
reference's protocol, so any pattern cfg written for it can be handed to ``RayCasterCfg.pattern_cfg``.  The pinhole
pattern's ``func(cfg, intrinsic_matrices, device)`` takes the cameras' intrinsics as well and returns ``(N, R, 3)``
tensors, as the reference's does (``RayCasterCameraCfg.pattern_cfg``).  The lidar and bpearl patterns are out of
scope.
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


def pinhole_camera_pattern(cfg: "PinholeCameraPatternCfg", intrinsic_matrices: torch.Tensor,
                           device) -> tuple[torch.Tensor, torch.Tensor]:
    """One ray through the centre of every pixel of a ``cfg.height`` x ``cfg.width`` image, for cameras with the
    intrinsic matrices ``(N, 3, 3)``: starts (all zero) and unit directions, ``(N, H * W, 3)`` each.  Pixel (row v,
    column u) is ray ``v * W + u``.  A pixel centre ``(u + 0.5, v + 0.5, 1)`` is taken through the inverse intrinsic
    matrix into the optical frame (x right, y down, z forward) and from there into the sensor frame of the ray
    caster (x forward, y left, z up): ``(z, -x, -y)``, normalised."""
    k = torch.as_tensor(intrinsic_matrices, device=device)
    if k.ndim != 3 or k.shape[1:] != (3, 3):
        raise ValueError(f"intrinsic_matrices must have the shape (N, 3, 3). Received: {tuple(k.shape)}.")
    if not k.is_floating_point():
        k = k.to(torch.float32)
    inv = torch.linalg.inv(k)  # (N, 3, 3)
    u = (torch.arange(cfg.width, device=device, dtype=k.dtype) + 0.5).repeat(cfg.height)  # (R,) the column runs fastest
    v = (torch.arange(cfg.height, device=device, dtype=k.dtype) + 0.5).repeat_interleave(cfg.width)
    # optical-frame coordinates of every pixel centre, (N, 3, R): inv[:, :, 0] u + inv[:, :, 1] v + inv[:, :, 2]
    optical = (inv[:, :, 0:1] * u + inv[:, :, 1:2] * v) + inv[:, :, 2:3]
    x, y, z = optical[:, 0], optical[:, 1], optical[:, 2]
    directions = torch.stack([z, -x, -y], dim=-1)  # (N, R, 3)
    directions = directions / torch.sqrt((z * z + x * x) + y * y).unsqueeze(-1)
    return torch.zeros_like(directions), directions


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


@dataclass
class PinholeCameraPatternCfg(PatternBaseCfg):
    """patterns_cfg.py ``PinholeCameraPatternCfg``.  Focal length, apertures and their offsets are in tenths of the
    world unit (cm for a world in metres), as a USD camera's are."""

    func: Callable = pinhole_camera_pattern
    focal_length: float = 24.0
    horizontal_aperture: float = 20.955
    vertical_aperture: Any = None  # None: horizontal_aperture * height / width (square pixels)
    horizontal_aperture_offset: float = 0.0
    vertical_aperture_offset: float = 0.0
    width: int = MISSING
    height: int = MISSING

    @classmethod
    def from_intrinsic_matrix(cls, intrinsic_matrix, width: int, height: int,
                              focal_length: float = 24.0) -> "PinholeCameraPatternCfg":
        """The cfg of a camera with the row-major intrinsic matrix ``[f_x, 0, c_x, 0, f_y, c_y, 0, 0, 1]``: the
        apertures that give these focal lengths in pixels at ``focal_length``, the offsets that put the principal
        point at ``(c_x, c_y)``."""
        f_x, c_x, f_y, c_y = (intrinsic_matrix[i] for i in (0, 2, 4, 5))
        return cls(focal_length=focal_length, horizontal_aperture=width * focal_length / f_x,
                   vertical_aperture=height * focal_length / f_y,
                   horizontal_aperture_offset=(c_x - width / 2) / f_x,
                   vertical_aperture_offset=(c_y - height / 2) / f_y, width=width, height=height)
