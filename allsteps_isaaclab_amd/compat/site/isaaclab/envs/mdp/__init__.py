"""Shim of ``isaaclab.envs.mdp``: the event function the device event kernel serves and the height-scan
observation over the device ray caster."""

from allsteps_isaaclab_amd.utils.events import push_by_setting_velocity  # noqa: F401
from allsteps_isaaclab_amd.utils.sensors import height_scan  # noqa: F401

__all__ = ["push_by_setting_velocity", "height_scan"]
