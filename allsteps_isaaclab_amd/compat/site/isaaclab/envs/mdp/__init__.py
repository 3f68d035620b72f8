"""Shim of ``isaaclab.envs.mdp``: the event function the device event kernel serves, the height-scan
observation over the device ray caster, the image observation over the device ray-cast camera, the IMU
observations over the device IMU kernel, and the velocity command cfgs and ``generated_commands`` over the device
command kernel."""

from allsteps_isaaclab_amd.utils.commands import (  # noqa: F401
    NormalVelocityCommandCfg, NullCommandCfg, UniformVelocityCommandCfg, generated_commands)
from allsteps_isaaclab_amd.utils.events import push_by_setting_velocity  # noqa: F401
from allsteps_isaaclab_amd.utils.sensors import (  # noqa: F401
    height_scan, image, imu_ang_vel, imu_lin_acc, imu_orientation)

__all__ = ["push_by_setting_velocity", "height_scan", "image", "imu_orientation", "imu_ang_vel", "imu_lin_acc",
           "UniformVelocityCommandCfg", "NormalVelocityCommandCfg", "NullCommandCfg", "generated_commands"]
