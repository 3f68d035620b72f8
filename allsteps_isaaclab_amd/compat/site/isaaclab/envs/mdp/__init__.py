"""Shim of ``isaaclab.envs.mdp``: the event function the device event kernel serves."""

from allsteps_isaaclab_amd.utils.events import push_by_setting_velocity  # noqa: F401

__all__ = ["push_by_setting_velocity"]
