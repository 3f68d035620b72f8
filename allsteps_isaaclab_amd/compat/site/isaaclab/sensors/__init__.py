"""Shim of ``isaaclab.sensors``: the ray-caster cfg classes, served by the device ray-cast kernels
(``cfg.height_scanner`` and ``cfg.camera`` of the envs), and ``ImuCfg``, served by the device IMU kernel
(``cfg.imu``)."""

from allsteps_isaaclab_amd.utils.sensors import ImuCfg, RayCasterCameraCfg, RayCasterCfg  # noqa: F401

from . import patterns  # noqa: F401

__all__ = ["ImuCfg", "RayCasterCameraCfg", "RayCasterCfg", "patterns"]
