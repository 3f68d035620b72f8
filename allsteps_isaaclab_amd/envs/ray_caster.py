"""The host side of ``cfg.height_scanner``: a ``RayCasterCfg`` checked against what the device kernel serves and
turned into the call's constants and local rays (no device needed).  ``views._RayCaster`` holds the device buffers.

The reference's ray caster casts against one static warp mesh; here the surfaces are the ground plane and the
env's stones, closed-form in ``k_ray_cast`` (csrc/allsteps_ray_caster.h), so ``mesh_prim_paths`` may name either or
both.  Everything the kernel does not serve is refused here with a ``NativeError`` that names the field.
"""

from __future__ import annotations

import math
import re

import torch

from .. import _native

GROUND_PATH = "/World/ground"
STONES_PATH = "/World/envs/env_.*/step_.*"
GROUND_Z = 0.0  # the plane terrain of the envs (envs/scene.py)


def _refuse(field: str, detail: str) -> "_native.NativeError":
    return _native.NativeError(f"cfg.height_scanner.{field}: {detail}.  The rays are cast by a HIP kernel against "
                               f"the ground plane and the stones (no host fallback)")


def quat_apply(quat: torch.Tensor, vec: torch.Tensor) -> torch.Tensor:
    """``isaaclab.utils.math.quat_apply`` (math.py:545-564) on (R, 4) and (R, 3): t = 2 (xyz x v), v + w t + xyz x t."""
    w, u = quat[:, :1], quat[:, 1:]
    t = torch.linalg.cross(u, vec, dim=-1) * 2
    return (vec + w * t) + torch.linalg.cross(u, t, dim=-1)


class RayCasterSpec:
    """A checked ``RayCasterCfg``: ``surfaces`` (AS_RAY_* bits), ``num_rays``, ``max_distance``, ``attach_yaw_only``
    and ``rays`` -- float32 (6, R) on the host, local start xyz | direction xyz after the cfg's offset."""

    def __init__(self, cfg, *, root_body: str, step_dt: float, step_paths=()):
        self.cfg = cfg
        path = getattr(cfg, "prim_path", None)
        if not isinstance(path, str) or not path:
            raise _refuse("prim_path", f"{path!r} is not a prim path")
        leaf = path.split("/")[-1]
        if re.match(r"^[a-zA-Z0-9/_]+$", leaf) is None:  # the reference's own refusal (ray_caster.py:61-67)
            raise RuntimeError(f"Invalid prim path for the ray-caster sensor: {path}."
                               "\n\tHint: Please ensure that the prim path does not contain any regex patterns in the "
                               "leaf.")
        if leaf != root_body:
            raise _refuse("prim_path", f"{path!r} attaches the sensor to {leaf!r}; only the robot's root body "
                                       f"{root_body!r} is served (its pose is the state's root_pos / root_quat)")
        meshes = getattr(cfg, "mesh_prim_paths", None)
        if not isinstance(meshes, (list, tuple)) or len(meshes) == 0:
            raise _refuse("mesh_prim_paths", f"{meshes!r} is not a non-empty list of prim paths")
        stones = {STONES_PATH, *step_paths}
        self.surfaces = 0
        for m in meshes:
            if m == GROUND_PATH:
                self.surfaces |= _native.RAY_GROUND
            elif m in stones:
                self.surfaces |= _native.RAY_STONES  # any of the stones' paths selects all of the env's stones
            else:
                raise _refuse("mesh_prim_paths", f"{m!r} is neither the ground plane {GROUND_PATH!r} nor the stones "
                                                 f"({STONES_PATH!r} or an entry of cfg.step_paths)")
        drift = tuple(getattr(cfg, "drift_range", (0.0, 0.0)))
        if len(drift) != 2 or any(float(x) != 0.0 for x in drift):
            raise _refuse("drift_range", f"{drift!r} is not (0.0, 0.0): the sensor carries no state and draws nothing")
        period = float(getattr(cfg, "update_period", 0.0))
        if not period <= step_dt:
            raise _refuse("update_period", f"{period!r} s is longer than the env step ({step_dt!r} s): the data would "
                                           f"have to go stale across steps, and the sensor keeps no timestamp")
        if getattr(cfg, "debug_vis", False):
            raise _refuse("debug_vis", "True asks for visualization markers, which a headless env has not")
        yaw = getattr(cfg, "attach_yaw_only", None)
        if not isinstance(yaw, bool):
            raise _refuse("attach_yaw_only", f"{yaw!r} is not a bool")
        self.attach_yaw_only = yaw
        self.max_distance = float(getattr(cfg, "max_distance", 1e6))
        if not math.isfinite(self.max_distance) or self.max_distance <= 0.0:
            raise _refuse("max_distance", f"{self.max_distance!r} is not a finite positive distance")
        pattern = getattr(cfg, "pattern_cfg", None)
        if pattern is None or not callable(getattr(pattern, "func", None)):
            raise _refuse("pattern_cfg", f"{pattern!r} has no func(cfg, device)")
        # RayCaster._initialize_rays_impl (ray_caster.py:201-209), on the host in float32
        starts, directions = pattern.func(pattern, "cpu")
        starts, directions = torch.as_tensor(starts), torch.as_tensor(directions)
        if starts.ndim != 2 or starts.shape[1] != 3 or directions.shape != starts.shape or len(starts) == 0:
            raise _refuse("pattern_cfg", f"func returned shapes {tuple(starts.shape)} and {tuple(directions.shape)}, "
                                         f"not (R, 3) and (R, 3)")
        self.num_rays = len(directions)
        if self.num_rays > _native.MAX_RAYS:
            raise _refuse("pattern_cfg", f"{self.num_rays} rays; the kernel takes at most AS_MAX_RAYS = "
                                         f"{_native.MAX_RAYS}")
        offset = getattr(cfg, "offset", None)
        pos, rot = list(getattr(offset, "pos", ())), list(getattr(offset, "rot", ()))
        if len(pos) != 3 or len(rot) != 4 or not all(math.isfinite(float(x)) for x in pos + rot):
            raise _refuse("offset", f"pos {pos!r} / rot {rot!r} is not a finite position and quaternion")
        starts, directions = starts.to(torch.float32).clone(), directions.to(torch.float32)
        offset_pos, offset_quat = torch.tensor(pos), torch.tensor(rot)
        directions = quat_apply(offset_quat.repeat(len(directions), 1), directions)
        starts += offset_pos
        self.rays = torch.cat([starts.T, directions.T]).contiguous()
        if not bool(torch.isfinite(self.rays).all()):
            raise _refuse("pattern_cfg", "a ray start or direction is not finite in float32")

    def native_cfg(self) -> "_native.AsRayCaster":
        c = _native.AsRayCaster()
        c.num_rays, c.attach_yaw_only, c.surfaces = self.num_rays, int(self.attach_yaw_only), self.surfaces
        c.max_distance, c.ground_z = self.max_distance, GROUND_Z
        return c

    def surface_names(self) -> list:
        return [name for bit, name in ((_native.RAY_GROUND, "ground"), (_native.RAY_STONES, "stones"))
                if self.surfaces & bit]
