"""Shim of ``isaaclab.sensors.patterns``: the grid pattern of the ray-caster sensor and the pinhole pattern of the
ray-cast camera."""

from allsteps_isaaclab_amd.utils.patterns import (  # noqa: F401
    GridPatternCfg, PatternBaseCfg, PinholeCameraPatternCfg, grid_pattern, pinhole_camera_pattern)

__all__ = ["GridPatternCfg", "PatternBaseCfg", "PinholeCameraPatternCfg", "grid_pattern", "pinhole_camera_pattern"]
