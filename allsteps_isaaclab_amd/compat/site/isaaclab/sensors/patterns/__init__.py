"""Shim of ``isaaclab.sensors.patterns``: the grid pattern of the ray-caster sensor."""

from allsteps_isaaclab_amd.utils.patterns import GridPatternCfg, PatternBaseCfg, grid_pattern  # noqa: F401

__all__ = ["GridPatternCfg", "PatternBaseCfg", "grid_pattern"]
