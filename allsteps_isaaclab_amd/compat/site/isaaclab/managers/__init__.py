"""Shim of ``isaaclab.managers``: the event cfg classes, served by the device event kernel.  The manager-based
workflow itself is out of scope."""

from allsteps_isaaclab_amd.utils.events import EventTermCfg, SceneEntityCfg  # noqa: F401

__all__ = ["EventTermCfg", "SceneEntityCfg"]
