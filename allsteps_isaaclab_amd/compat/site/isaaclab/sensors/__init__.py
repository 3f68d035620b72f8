"""Shim of ``isaaclab.sensors``: the ray-caster cfg classes, served by the device ray-cast kernels
(``cfg.height_scanner`` and ``cfg.camera`` of the envs), ``ImuCfg``, served by the device IMU kernel
(``cfg.imu``), and ``FrameTransformerCfg`` / ``OffsetCfg``, served by the device frame-transformer kernel
(``cfg.frame_transformer``)."""

from allsteps_isaaclab_amd.utils.sensors import (  # noqa: F401
    FrameTransformerCfg,
    ImuCfg,
    OffsetCfg,
    RayCasterCameraCfg,
    RayCasterCfg,
)

from . import patterns  # noqa: F401

__all__ = ["FrameTransformerCfg", "ImuCfg", "OffsetCfg", "RayCasterCameraCfg", "RayCasterCfg", "patterns"]
