"""Shim of ``isaaclab.sensors``: the ray-caster cfg classes, served by the device ray-cast kernel
(``cfg.height_scanner`` of the envs)."""

from allsteps_isaaclab_amd.utils.sensors import RayCasterCfg  # noqa: F401

from . import patterns  # noqa: F401

__all__ = ["RayCasterCfg", "patterns"]
