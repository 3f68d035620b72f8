"""``AllstepsEnvCfg`` -- the configuration surface of the reference task, MI355X-native backend.

Mirrors ``isaaclab_tasks/direct/allsteps/allsteps_env_cfg.py:51-235`` field for field where the
field means something without Omniverse (env counts, timing, reward scales, names, reset ranges),
plus the physics constants that replace the PhysX scene/articulation settings
(``simulation_cfg.py``, ``walker3d.py:21-46``).  USD/visual fields (markers, lights, materials,
prim paths) have no meaning here and are not carried.
"""

from __future__ import annotations

import dataclasses
import math
from dataclasses import dataclass, field


@dataclass
class SimulationCfg:
    """Physics constants (``isaaclab/sim/simulation_cfg.py``; ``walker3d.py:21-46``)."""

    dt: float = 1.0 / 240.0                 # allsteps_env_cfg.py:62
    render_interval: int = 4
    device: str = "cuda:0"
    gravity: tuple = (0.0, 0.0, -9.81)      # simulation_cfg.py gravity
    # Contact / solver settings replacing PhysX TGS (walker3d.py:26-32: 4 position iterations,
    # max_depenetration_velocity 10).  Friction: "average" combine of the MJCF geom friction 1.2
    # and the PhysX default material 0.5 (simulation_cfg.py default material) -> 0.85.
    friction: float = 0.85
    contact_margin: float = 0.01
    baumgarte: float = 0.2
    slop: float = 0.002
    max_depenetration_velocity: float = 10.0
    solver_position_iteration_count: int = 4
    max_joint_velocity: float = 100.0


@dataclass
class InteractiveSceneCfg:
    num_envs: int = 4096                    # allsteps_env_cfg.py:78
    env_spacing: float = 4.0
    replicate_physics: bool = True


@dataclass
class AllstepsEnvCfg:
    # env (allsteps_env_cfg.py:53-59)
    episode_length_s: float = 15.0
    decimation: int = 4
    action_scale: float = 1.0
    action_space: int = 21
    observation_space: int = 59
    state_space: int = 0
    seed: int | None = 42
    is_finite_horizon: bool = False          # direct_rl_env_cfg.py:59

    sim: SimulationCfg = field(default_factory=SimulationCfg)
    scene: InteractiveSceneCfg = field(default_factory=InteractiveSceneCfg)

    # steps (allsteps_env_cfg.py:90-97)
    num_steps: int = 20
    step_size: tuple = (0.5, 0.8, 0.225)
    step_radius: float = 0.25
    camera_pos: tuple = (1.5, -4.0, 1.5)
    # Curriculum level the stones are generated at.  The reference generates them once at level 0
    # (allsteps_env.py:71) and never regenerates; C3 uses 9 as an init knob.
    initial_stone_curriculum: int = 0
    # The reference never regenerates stones (its _reset_idx resets curr_target_index before testing
    # it, allsteps_env.py:492-500).  True = the intended behaviour: a reset env
    # whose target index was past half the stones gets a new course at the current curriculum level.
    regenerate_footsteps: bool = False
    # The opt-in contact report: with True the step also stores the contacts its solver kept in each of the
    # last `decimation` substeps, and the env serves real sensor*.data.force_matrix_w / net_forces_w /
    # net_forces_w_history (contact_sensor.py:329-343, history_length = 4: allsteps_env_cfg.py:119-130) and
    # robot.data.joint_acc (articulation_data.py:547-556).  False: the step and its outputs as ever.
    contact_forces: bool = False
    # The contact sensors' air / contact timers (ContactSensorCfg.track_air_time and force_threshold,
    # contact_sensor_cfg.py:23-30): with True sensor*.data.current_air_time / last_air_time / current_contact_time /
    # last_contact_time and sensor*.compute_first_contact / compute_first_air, advanced on the device by one HIP
    # kernel after the step (csrc/contact_timer_kernels.h: `decimation` sensor updates per step, one launch more);
    # a foot is in contact where the norm of its net contact force exceeds contact_force_threshold (N).  It
    # builds the contact report itself, so the contact_forces views work too.  False: the step as ever.
    contact_air_time: bool = False
    contact_force_threshold: float = 1.0
    # A ray-caster height scanner on the robot's root body (the reference's RayCasterCfg, e.g. velocity_env_cfg.py:
    # 66-73): a utils.sensors.RayCasterCfg, or None.  env.height_scanner / env.scene.sensors["height_scanner"] then
    # cast the cfg's ray pattern against the ground plane and / or the env's stones in one HIP kernel
    # (csrc/ray_caster_kernels.h) whenever the data is read after the scene changed; mdp.height_scan reads it.  The
    # step, its observation and the state are as ever either way.  None: nothing allocated, nothing launched.
    height_scanner: object = None
    # IMU sensors on any of the robot's bodies (the reference's ImuCfg): a utils.sensors.ImuCfg -- then env.imu,
    # env.scene.sensors["imu"] and the defaults of mdp.imu_orientation / imu_ang_vel / imu_lin_acc -- or a dict of
    # name -> ImuCfg (at most 8), or None.  One HIP kernel (csrc/imu_kernels.h) updates every sensor of the envs that
    # are outdated -- all of them after a step or a reset, the envs of a masked reset -- whenever a sensor's data is
    # read.  The step, its observation and the state are as ever either way.  None: nothing allocated or launched.
    imu: object = None
    # Frame transformers over the robot's bodies and the env's stones (the reference's FrameTransformerCfg): a
    # utils.sensors.FrameTransformerCfg -- then env.frame_transformer and env.scene.sensors["frame_transformer"] --
    # or a dict of name -> FrameTransformerCfg (at most 4, 32 target frames in all), or None.  One HIP kernel
    # (csrc/frame_transformer_kernels.h) forms every target frame in the world and in its source frame whenever a
    # sensor's data is read after the scene changed.  The step, its observation and the state are as ever either
    # way.  None: nothing allocated or launched.
    frame_transformer: object = None
    # ray-cast depth cameras on the root body (the reference's RayCasterCameraCfg): a utils.sensors.RayCasterCameraCfg
    # -- then env.camera and env.scene.sensors["camera"] -- or a dict of name -> cfg (at most 4), or None.  One HIP
    # kernel (csrc/ray_camera_kernels.h) casts a camera's pixels against the ground and the stones whenever its data
    # is read after the scene changed; mdp.image reads it.  The default step launches nothing for it.
    camera: object = None
    # Noise models of DirectRLEnvCfg (direct_rl_env_cfg.py:171, 208): a utils.noise NoiseModelCfg /
    # NoiseModelWithAdditiveBiasCfg (the reference's isaaclab.utils.noise classes) or None.  The action model
    # perturbs the action before the step, the observation model the policy observation after it, a bias model's
    # per-env bias is re-drawn for every env that resets -- in HIP kernels around the step (csrc/noise_kernels.h),
    # one launch more per step for an observation model, two with an action model; None: the step as ever.
    action_noise_model: object = None
    observation_noise_model: object = None
    # Events of DirectRLEnvCfg (direct_rl_env_cfg.py `events`): a dict or cfg object of utils.events EventTermCfg
    # (the reference's isaaclab.managers class) or None.  Served: push_by_setting_velocity in "interval" mode --
    # per-env timers, the push added to the root velocity -- in one HIP kernel after the step
    # (csrc/event_kernels.h), one launch more per step; anything else raises at construction.  None: the step as
    # ever.
    events: object = None
    # Command manager (the reference's ManagerBasedRLEnvCfg `commands`): a dict or cfg object of utils.commands
    # UniformVelocityCommandCfg / NormalVelocityCommandCfg terms, or None.  Served on the device by k_commands_step
    # (csrc/command_kernels.h), one launch more per step, as env.command_manager; the task's observation and reward
    # do not read it.  Anything else raises at construction.  None: nothing is allocated or launched.
    commands: object = None
    # Observation manager (the reference's ManagerBasedEnvCfg `observations`): a dict or cfg object whose entries are
    # utils.observations ObservationGroupCfg groups of ObservationTermCfg terms, or None.  Each group is assembled on
    # the device by k_observations (csrc/observation_kernels.h), one launch per group last in the step, as
    # env.observation_manager and under its name in the returned observation dict; "policy" stays the task's own.
    # Anything not served raises at construction.  None: nothing is allocated or launched.
    observations: object = None
    # Reward manager (the reference's ManagerBasedRLEnvCfg `rewards`): a dict or cfg object whose entries are
    # utils.rewards RewardTermCfg terms (None entries are skipped), or None.  The weighted sum, the episodic sums and
    # the per-step term values are computed on the device by k_rewards_step (csrc/reward_kernels.h), one launch per
    # step, as env.reward_manager.  step() returns the task's own reward unless rewards_replace_task_reward, which
    # makes it the manager's.  Anything not served raises at construction.  None: nothing is allocated or launched.
    rewards: object = None
    rewards_replace_task_reward: bool = False
    # Termination manager (the reference's ManagerBasedRLEnvCfg `terminations`): a dict or cfg object whose entries
    # are utils.terminations TerminationTermCfg terms (None entries are skipped), or None.  The terms' flags,
    # time_outs, terminated and dones are computed on the device by k_terminations_step
    # (csrc/termination_kernels.h), one launch per step directly after the step, as env.termination_manager.
    # step() returns the task's own dones and resets only what the task resets unless terminations_reset (the
    # walker only), which also ends and resets the envs the manager's dones name.  Anything not served raises at
    # construction.  None: nothing is allocated or launched.
    terminations: object = None
    terminations_reset: bool = False
    # Action manager (the reference's ManagerBasedEnvCfg `actions`): a dict or cfg object whose entries are
    # utils.actions term cfgs, in cfg order (None entries are skipped), or None.  The walker's torque actuator
    # serves JointEffortActionCfg terms that together command every joint exactly once: the processed action is
    # the applied effort itself -- the hard-wired gain_curriculum * gear * clip(a) is not applied, so the
    # curriculum gain does not act on an effort term.  The terms are processed on the device by k_actions_process
    # (csrc/action_kernels.h), one launch per step ahead of the physics, as env.action_manager; action_space must
    # equal the terms' total dimension.  Anything not served raises at construction.  None: nothing is allocated
    # or launched and the step applies its own formula.
    actions: object = None

    # joint gears, cfg/PhysX dof order (allsteps_env_cfg.py:133-155)
    joint_gears: list = field(default_factory=lambda: [
        60, 80, 60, 50, 60, 60, 50, 60, 60, 60, 60, 80, 100, 60, 80, 100, 60, 90, 90, 60, 60])
    force_scale: float = 1.5

    torso_name: str = "torso"
    foot_names: list = field(default_factory=lambda: ["right_foot", "left_foot"])
    hip_y_names: list = field(default_factory=lambda: ["right_hip_y", "left_hip_y"])
    right_body_names: list = field(default_factory=lambda: [
        "right_shoulder_x", "right_shoulder_y", "right_shoulder_z", "right_elbow", "right_hip_x",
        "right_hip_y", "right_hip_z", "right_knee", "right_ankle"])
    left_body_names: list = field(default_factory=lambda: [
        "left_shoulder_x", "left_shoulder_y", "left_shoulder_z", "left_elbow", "left_hip_x",
        "left_hip_y", "left_hip_z", "left_knee", "left_ankle"])
    negation_body_names: list = field(default_factory=lambda: ["abdomen_z", "abdomen_x"])

    # reward scales (allsteps_env_cfg.py:222-234)
    energy_cost_scale: float = 0.009
    actions_cost_scale: float = 0.01
    alive_reward_scale: float = 2.0
    dof_vel_scale: float = 0.1
    joint_at_limit_cost_scale: float = 0.1
    death_cost: float = -1.0
    termination_height_absolute: float = 0.4
    angular_velocity_scale: float = 0.25
    initial_joint_angle_range: list = field(default_factory=lambda: [-0.1, 0.1])
    initial_joint_angle_clip_range: list = field(default_factory=lambda: [-0.95, 0.95])

    # task constants hard-coded in allsteps_env.py:29-60
    epsilon: float = 1e-4
    stop_frames: int = 2
    max_curriculum: int = 9
    curriculum_progress_threshold: int = 12
    init_root_pos: tuple = (0.2, 0.0, 1.5)   # walker3d.py:37

    def replace(self, **kw) -> "AllstepsEnvCfg":
        return dataclasses.replace(self, **kw)

    @property
    def step_dt(self) -> float:
        return self.sim.dt * self.decimation

    @property
    def max_episode_length(self) -> int:
        # direct_rl_env.py:247-250
        return math.ceil(self.episode_length_s / (self.sim.dt * self.decimation))


def running_start_pose() -> list:
    """allsteps_env.py:505-511: running-start joint pose, cfg dof order."""
    q = [0.0] * 21
    q[12] = q[17] = -math.pi / 8
    q[15] = math.pi / 10
    q[2] = q[5] = math.pi / 3
    q[4] = -math.pi / 6
    q[7] = math.pi / 6
    q[9] = q[10] = math.pi / 3
    return q
