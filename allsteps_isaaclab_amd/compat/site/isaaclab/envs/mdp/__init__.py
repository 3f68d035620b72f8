"""Shim of ``isaaclab.envs.mdp``: the event function the device event kernel serves, the height-scan
observation over the device ray caster, the image observation over the device ray-cast camera, the IMU
observations over the device IMU kernel, the velocity command cfgs and ``generated_commands`` over the device
command kernel, the observation functions the device observation kernel serves, the reward functions the device
reward kernel serves (those of the velocity task's ``mdp`` among them), the termination functions the device
termination kernel serves, and the action term cfgs of ``isaaclab.envs.mdp.actions``: the joint terms the device
action kernels serve, and the others, which import and are refused by the envs with their reason."""

from allsteps_isaaclab_amd.utils.actions import (  # noqa: F401
    JointActionCfg, JointPositionActionCfg, JointEffortActionCfg, JointPositionToLimitsActionCfg,
    EMAJointPositionToLimitsActionCfg, RelativeJointPositionActionCfg, JointVelocityActionCfg, BinaryJointActionCfg,
    BinaryJointPositionActionCfg, BinaryJointVelocityActionCfg, NonHolonomicActionCfg,
    DifferentialInverseKinematicsActionCfg, OperationalSpaceControllerActionCfg)
from allsteps_isaaclab_amd.utils.commands import (  # noqa: F401
    NormalVelocityCommandCfg, NullCommandCfg, UniformVelocityCommandCfg, generated_commands)
from allsteps_isaaclab_amd.utils.events import push_by_setting_velocity  # noqa: F401
from allsteps_isaaclab_amd.utils.observations import (  # noqa: F401
    base_ang_vel, base_lin_vel, base_pos_z, body_incoming_wrench, image_features, joint_pos,
    joint_pos_limit_normalized, joint_pos_rel, joint_vel, joint_vel_rel, last_action, projected_gravity, root_ang_vel_w,
    root_lin_vel_w, root_pos_w, root_quat_w)
from allsteps_isaaclab_amd.utils.rewards import (  # noqa: F401
    is_alive, is_terminated, is_terminated_term, lin_vel_z_l2, ang_vel_xy_l2, flat_orientation_l2, base_height_l2,
    body_lin_acc_l2, joint_torques_l2, joint_vel_l1, joint_vel_l2, joint_acc_l2, joint_deviation_l1,
    joint_pos_limits, joint_vel_limits, applied_torque_limits, action_rate_l2, action_l2, undesired_contacts,
    contact_forces, track_lin_vel_xy_exp, track_ang_vel_z_exp, feet_air_time, feet_air_time_positive_biped,
    feet_slide, track_lin_vel_xy_yaw_frame_exp, track_ang_vel_z_world_exp)
from allsteps_isaaclab_amd.utils.terminations import (  # noqa: F401
    time_out, command_resample, bad_orientation, root_height_below_minimum, joint_pos_out_of_limit,
    joint_pos_out_of_manual_limit, joint_vel_out_of_limit, joint_vel_out_of_manual_limit, joint_effort_out_of_limit,
    illegal_contact)
from allsteps_isaaclab_amd.utils.sensors import (  # noqa: F401
    height_scan, image, imu_ang_vel, imu_lin_acc, imu_orientation)

__all__ = ["push_by_setting_velocity", "height_scan", "image", "imu_orientation", "imu_ang_vel", "imu_lin_acc",
           "UniformVelocityCommandCfg", "NormalVelocityCommandCfg", "NullCommandCfg", "generated_commands",
           "base_pos_z", "base_lin_vel", "base_ang_vel", "projected_gravity", "root_pos_w", "root_quat_w",
           "root_lin_vel_w", "root_ang_vel_w", "joint_pos", "joint_pos_rel", "joint_pos_limit_normalized", "joint_vel",
           "joint_vel_rel", "last_action", "body_incoming_wrench", "image_features",
           "is_alive", "is_terminated", "is_terminated_term", "lin_vel_z_l2", "ang_vel_xy_l2",
           "flat_orientation_l2", "base_height_l2", "body_lin_acc_l2", "joint_torques_l2", "joint_vel_l1",
           "joint_vel_l2", "joint_acc_l2", "joint_deviation_l1", "joint_pos_limits", "joint_vel_limits",
           "applied_torque_limits", "action_rate_l2", "action_l2", "undesired_contacts", "contact_forces",
           "track_lin_vel_xy_exp", "track_ang_vel_z_exp", "feet_air_time", "feet_air_time_positive_biped",
           "feet_slide", "track_lin_vel_xy_yaw_frame_exp", "track_ang_vel_z_world_exp",
           "time_out", "command_resample", "bad_orientation", "root_height_below_minimum", "joint_pos_out_of_limit",
           "joint_pos_out_of_manual_limit", "joint_vel_out_of_limit", "joint_vel_out_of_manual_limit",
           "joint_effort_out_of_limit", "illegal_contact",
           "JointActionCfg", "JointPositionActionCfg", "JointEffortActionCfg", "JointPositionToLimitsActionCfg",
           "EMAJointPositionToLimitsActionCfg", "RelativeJointPositionActionCfg", "JointVelocityActionCfg",
           "BinaryJointActionCfg", "BinaryJointPositionActionCfg", "BinaryJointVelocityActionCfg",
           "NonHolonomicActionCfg", "DifferentialInverseKinematicsActionCfg", "OperationalSpaceControllerActionCfg"]
