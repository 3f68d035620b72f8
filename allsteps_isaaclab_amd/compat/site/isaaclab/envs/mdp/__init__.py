"""Shim of ``isaaclab.envs.mdp``: the event function the device event kernel serves, the height-scan
observation over the device ray caster and the IMU observations over the device IMU kernel."""

from allsteps_isaaclab_amd.utils.events import push_by_setting_velocity  # noqa: F401
from allsteps_isaaclab_amd.utils.sensors import height_scan, imu_ang_vel, imu_lin_acc, imu_orientation  # noqa: F401

__all__ = ["push_by_setting_velocity", "height_scan", "imu_orientation", "imu_ang_vel", "imu_lin_acc"]
