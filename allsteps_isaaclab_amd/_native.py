"""ctypes binding of ``liballsteps_hip.so`` (the C ABI of ``include/allsteps.h``).

The product path has no fallback: if the HIP library is missing or no gfx950 device is present the
calls raise :class:`NativeError` -- nothing silently runs on the CPU.
"""

from __future__ import annotations

import ctypes as C
import os

import numpy as np

PKG = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(PKG, "liballsteps_hip.so")
PPO_LIB_PATH = os.path.join(PKG, "libppo_hip.so")
CSRC = os.path.join(PKG, "csrc")
INCLUDE = os.path.join(os.path.dirname(PKG), "include")

MAXL, MAXG, MAXSP = 32, 32, 256
ABI_VERSION = 6

EXPORTED_SYMBOLS = [
    "as_create", "as_destroy", "as_reset_all", "as_step", "as_physics_step", "as_generate_stones",
    "as_step_counters", "as_get_curriculum_host", "as_abi_version", "as_last_error", "as_task_step",
    "as_set_seed", "as_profile", "as_profile_read", "as_debug_stamps", "as_reset_mask", "as_set_graph_safe",
    "as_profile_sampled", "as_hbm_copy", "as_set_actuator", "as_set_quad_task", "as_quad_step", "as_quad_reset_all",
    "as_build_id", "as_step_counters_host", "as_body_state", "as_sweep_plan", "as_set_contact_report",
    "as_contact_forces", "as_noise_actions", "as_noise_post", "as_events_init", "as_events_interval",
    "as_contact_timers", "as_ray_cast", "as_imu", "as_ray_camera",
    "as_frame_transformer", "as_commands_step", "as_commands_reset", "as_observations_step",
    "as_observations_reset", "as_rewards_step", "as_rewards_reset", "as_terminations_step",
    "as_actions_step", "as_actions_reset", "as_set_joint_commands", "as_quad_reset_mask",
]
MAXB = 32  # AS_MAX_BODIES
MAXC = 10  # AS_MAX_CONTACTS
REPORT_WORDS = 8  # AS_REPORT_WORDS: lambda_n n (3) | contact point (3) | separation | packed ids
REPORT_FEET = 4  # AS_REPORT_FEET
NUM_STONES = 20  # AS_NUM_STONES
TIMER_ROWS = 4  # as_contact_timers rows: current_air, last_air, current_contact, last_contact
MAX_RAYS = 1024  # AS_MAX_RAYS
RAY_GROUND, RAY_STONES = 1, 2  # AS_RAY_GROUND, AS_RAY_STONES (as_ray_caster_t.surfaces)
RAY_HIT_GROUND, RAY_MISS = -1, -2  # AS_RAY_HIT_GROUND, AS_RAY_MISS (as_ray_cast's surface)
MAX_CAMERA_RAYS = 16384  # AS_MAX_CAMERA_RAYS (128 x 128)
CAM_CLIP_NONE, CAM_CLIP_MAX, CAM_CLIP_ZERO = 0, 1, 2  # AS_CAM_CLIP_* (as_ray_camera_t.clipping)
MAX_IMUS = 8  # AS_MAX_IMUS
IMU_DATA_ROWS = 19  # as_imu data rows: pos 3 | quat 4 | lin_vel_b 3 | ang_vel_b 3 | lin_acc_b 3 | ang_acc_b 3
IMU_PREV_ROWS = 6  # as_imu prev rows: world linear | angular velocity of the previous update
MAX_FRAME_TRANSFORMERS = 4  # AS_MAX_FRAME_TRANSFORMERS
MAX_FRAMES = 32  # AS_MAX_FRAMES
FRAME_SOURCE_ROWS = 7  # as_frame_transformer source rows: pos 3 | quat 4
FRAME_TARGET_ROWS = 14  # as_frame_transformer target rows: pos_w 3 | quat_w 4 | pos_source 3 | quat_source 4
BODY_STATE_ROWS = 16  # AS_BODY_STATE_ROWS: pos 3 | quat 4 | frame lin vel 3 | ang vel 3 | COM lin vel 3


class NativeError(RuntimeError):
    pass


class AsBodyTable(C.Structure):
    """as_body_table_t (include/allsteps.h): the model's bodies for as_body_state."""
    _fields_ = [("num_bodies", C.c_int32), ("link", C.c_int32 * MAXB), ("offset_pos", (C.c_float * 3) * MAXB),
                ("offset_quat", (C.c_float * 4) * MAXB), ("com", (C.c_float * 3) * MAXB)]


class AsRayCaster(C.Structure):
    """as_ray_caster_t (include/allsteps.h): what one as_ray_cast call casts against and how far."""
    _fields_ = [("num_rays", C.c_int32), ("attach_yaw_only", C.c_int32), ("surfaces", C.c_int32),
                ("max_distance", C.c_float), ("ground_z", C.c_float)]


class AsRayCamera(C.Structure):
    """as_ray_camera_t (include/allsteps.h): the image, what one as_ray_camera call casts against and the clipping."""
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("surfaces", C.c_int32), ("clipping", C.c_int32),
                ("max_distance", C.c_float), ("ground_z", C.c_float)]


class AsImuTable(C.Structure):
    """as_imu_table_t (include/allsteps.h): the sensors of one as_imu call, each on a body of the model."""
    _fields_ = [("num_sensors", C.c_int32), ("link", C.c_int32 * MAX_IMUS),
                ("body_offset_pos", (C.c_float * 3) * MAX_IMUS), ("body_offset_quat", (C.c_float * 4) * MAX_IMUS),
                ("com", (C.c_float * 3) * MAX_IMUS), ("offset_pos", (C.c_float * 3) * MAX_IMUS),
                ("offset_rot", (C.c_float * 4) * MAX_IMUS), ("gravity_bias", (C.c_float * 3) * MAX_IMUS)]


class AsFrameBody(C.Structure):
    """as_frame_body_t (include/allsteps.h): the body (link >= 0) or stone (link < 0) a frame sits on, and its offset."""
    _fields_ = [("link", C.c_int32), ("stone", C.c_int32), ("body_offset_pos", C.c_float * 3),
                ("body_offset_quat", C.c_float * 4), ("offset_pos", C.c_float * 3), ("offset_rot", C.c_float * 4)]


class AsFrameTable(C.Structure):
    """as_frame_table_t (include/allsteps.h): the sensors and target frames of one as_frame_transformer call."""
    _fields_ = [("num_sensors", C.c_int32), ("num_frames", C.c_int32),
                ("apply_source_offset", C.c_int32 * MAX_FRAME_TRANSFORMERS),
                ("apply_target_offset", C.c_int32 * MAX_FRAME_TRANSFORMERS),
                ("source", AsFrameBody * MAX_FRAME_TRANSFORMERS), ("target", AsFrameBody * MAX_FRAMES),
                ("sensor", C.c_int32 * MAX_FRAMES)]


class AsContactReport(C.Structure):
    """as_contact_report_t (include/allsteps.h): caller-owned device buffers of the opt-in contact report."""
    _fields_ = [("depth", C.c_int32), ("count", C.c_void_p), ("records", C.c_void_p), ("qd_prev", C.c_void_p)]


class AsNoiseModel(C.Structure):
    """as_noise_model_t (include/allsteps.h): a noise term, its parameter vectors and the optional per-env bias."""
    _fields_ = [("kind", C.c_int32), ("op", C.c_int32), ("p0", C.c_void_p), ("p1", C.c_void_p),
                ("bias_kind", C.c_int32), ("bias_op", C.c_int32), ("bias_p0", C.c_float), ("bias_p1", C.c_float),
                ("bias", C.c_void_p)]


NOISE_NONE, NOISE_CONSTANT, NOISE_UNIFORM, NOISE_GAUSSIAN = 0, 1, 2, 3  # AS_NOISE_*
NOISE_OPS = {"add": 0, "scale": 1, "abs": 2}  # AS_NOISE_ADD / SCALE / ABS
NOISE_MAX_COLS = 256
# Philox tags of the noise streams (csrc/allsteps_noise.h): action term, observation term, action bias,
# observation bias
NOISE_TAGS = (0x4E416374, 0x4E4F6273, 0x4E416269, 0x4E4F6269)


def _ptr(t):
    return None if t is None else t.data_ptr()


def noise_actions(model: AsNoiseModel, src, out, t, draws=None, seed: int = 0, env_offset: int = 0, stream=None):
    """as_noise_actions: out (n, cols) = model(src), on `stream`; draws (n, cols) injected or None (Philox)."""
    n, cols = src.shape
    check(load().as_noise_actions(C.byref(model), src.data_ptr(), out.data_ptr(), n, cols, t.data_ptr(), _ptr(draws),
                                  seed & 0xFFFFFFFFFFFFFFFF, env_offset, stream), "as_noise_actions")


def noise_post(action_model, obs_model, obs, t, reset=None, reset2=None, obs_draws=None, action_bias_draws=None,
               obs_bias_draws=None, seed: int = 0, env_offset: int = 0, stream=None):
    """as_noise_post: re-draw the biases of the envs in reset | reset2 (None: all), noise obs (n, cols) in
    place (None: skip), advance t (n,)."""
    n = t.shape[0]
    cols = 0 if obs is None else obs.shape[1]
    check(load().as_noise_post(None if action_model is None else C.byref(action_model),
                               None if obs_model is None else C.byref(obs_model), _ptr(obs), n, cols, t.data_ptr(),
                               _ptr(reset), _ptr(reset2), _ptr(obs_draws), _ptr(action_bias_draws),
                               _ptr(obs_bias_draws), seed & 0xFFFFFFFFFFFFFFFF, env_offset, stream), "as_noise_post")


MAX_EVENT_TERMS = 4  # AS_MAX_EVENT_TERMS
EVENT_TERM_FLOATS = 14  # as_event_term_t: interval_lo, interval_w, vel_lo[6], vel_w[6]
# Philox tags of the event streams (csrc/allsteps_events.h): interval resamples, pushes
EVENT_TAGS = (0x45764976, 0x45765075)


def events_init(terms, time_left, t, interval_draws=None, seed: int = 0, env_offset: int = 0, stream=None):
    """as_events_init: time_left (terms, n) = the initial timers, t (n,) = 1.  terms: (terms, 14) float32 device
    rows of as_event_term_t; interval_draws (terms, n) injected or None (Philox at counter 0)."""
    k, n = time_left.shape
    check(load().as_events_init(terms.data_ptr(), k, time_left.data_ptr(), t.data_ptr(), n, _ptr(interval_draws),
                                seed & 0xFFFFFFFFFFFFFFFF, env_offset, stream), "as_events_init")


def events_interval(terms, root_lin, root_ang, time_left, t, dt: float, fired=None, interval_draws=None,
                    push_draws=None, seed: int = 0, env_offset: int = 0, stream=None):
    """as_events_interval: one env step of the interval terms on root_lin / root_ang (3, n), time_left
    (terms, n), t (n,); fired (terms, n) uint8 or None; interval_draws (terms, n), push_draws (terms, 6, n)
    injected or None (Philox)."""
    k, n = time_left.shape
    check(load().as_events_interval(terms.data_ptr(), k, root_lin.data_ptr(), root_ang.data_ptr(),
                                    time_left.data_ptr(), t.data_ptr(), _ptr(fired), n, dt, _ptr(interval_draws),
                                    _ptr(push_draws), seed & 0xFFFFFFFFFFFFFFFF, env_offset, stream),
          "as_events_interval")


MAX_COMMAND_TERMS = 4  # AS_MAX_COMMAND_TERMS
COMMAND_DRAWS = 11  # AS_COMMAND_DRAWS: draws a term consumes per resample at most
COMMAND_UNIFORM, COMMAND_NORMAL = 0, 1  # AS_COMMAND_UNIFORM / AS_COMMAND_NORMAL
COMMAND_FLAG_ROWS = 5  # is_heading, is_standing, is_zero_vel_x / y / yaw
COMMAND_METRIC_ROWS = 2  # error_vel_xy, error_vel_yaw
# as_command_term_t as 21 32-bit words: kind, heading (int32) | time_lo, time_w | lo[4] | w[4] | clip_lo, clip_hi |
# stiffness | p_heading | p_standing | p_zero[3] | max_command_step (float32)
COMMAND_TERM_WORDS = 21
# Philox tags of the command streams (csrc/allsteps_commands.h): the reset's resample, the compute's
COMMAND_TAGS = (0x436D5273, 0x436D4370)


def commands_step(terms, root_quat, root_lin, root_ang, vel, heading_target, flags, time_left, counter, metrics,
                  last_metrics, t, dt: float, reset=None, reset2=None, draws=None, seed: int = 0, env_offset: int = 0,
                  stream=None):
    """as_commands_step: the reset of the envs in reset | reset2 ((n,) uint8 / bool, None: none), then
    CommandTerm.compute(dt) of every env, every term.  terms: (terms, 21) float32 device rows of as_command_term_t;
    root_quat (4, n), root_lin / root_ang (3, n); vel (terms, 3, n), heading_target (terms, n), flags (terms, 5, n)
    uint8, time_left (terms, n), counter (terms, n) int32, metrics / last_metrics (terms, 2, n) (last_metrics may
    be None), t (n,); draws (2, terms, 11, n) injected or None (Philox)."""
    k, n = time_left.shape
    check(load().as_commands_step(terms.data_ptr(), k, root_quat.data_ptr(), root_lin.data_ptr(),
                                  root_ang.data_ptr(), vel.data_ptr(), heading_target.data_ptr(), flags.data_ptr(),
                                  time_left.data_ptr(), counter.data_ptr(), metrics.data_ptr(), _ptr(last_metrics),
                                  t.data_ptr(), _ptr(reset), _ptr(reset2), n, dt, _ptr(draws),
                                  seed & 0xFFFFFFFFFFFFFFFF, env_offset, stream), "as_commands_step")


def commands_reset(terms, vel, heading_target, flags, time_left, counter, metrics, last_metrics, t, mask=None,
                   draws=None, seed: int = 0, env_offset: int = 0, stream=None):
    """as_commands_reset: CommandTerm.reset of the envs in mask ((n,) uint8 / bool, None: all), no compute; draws
    (terms, 11, n) injected or None (Philox)."""
    k, n = time_left.shape
    check(load().as_commands_reset(terms.data_ptr(), k, vel.data_ptr(), heading_target.data_ptr(), flags.data_ptr(),
                                   time_left.data_ptr(), counter.data_ptr(), metrics.data_ptr(), _ptr(last_metrics),
                                   t.data_ptr(), _ptr(mask), n, _ptr(draws), seed & 0xFFFFFFFFFFFFFFFF, env_offset,
                                   stream), "as_commands_reset")


MAX_OBS_GROUPS = 4  # AS_MAX_OBS_GROUPS
MAX_OBS_TERMS = 16  # AS_MAX_OBS_TERMS: terms of a group
MAX_OBS_COLS = 256  # AS_MAX_OBS_COLS: columns of a group before the history
MAX_OBS_OUT_COLS = 1280  # AS_MAX_OBS_OUT_COLS: columns of a group's output, history included
OBS_COL_ROWS = 6  # AS_OBS_COL_ROWS: source row (int32) | a | b | noise p0 | noise p1 | scale
OBS_GATHER, OBS_LIMIT_NORM, OBS_QUAT_UNIQUE, OBS_ROTATE_INVERSE, OBS_HEIGHT_SCAN, OBS_LAST_ACTION = range(6)  # AS_OBS_*
OBS_SOURCES = ("root_pos", "root_quat", "root_lin", "root_ang", "q", "qd", "commands", "imu", "ray_hits", "ray_pose",
               "actions", "gravity")  # AS_OBS_SRC_*, in order
# as_observation_term_t as 12 32-bit words: kind, source, width, col, out_col, history, noise_kind, noise_op, clip
# (int32) | clip_lo, clip_hi (float32) | flags (int32)
OBS_TERM_WORDS = 12
OBS_TAG = 0x4F62734D  # Philox tag of the observation streams (csrc/allsteps_observations.h)


class AsObservationSources(C.Structure):
    """as_observation_sources_t (include/allsteps.h): the device rows the terms of a group read."""
    _fields_ = [("ptr", C.c_void_p * len(OBS_SOURCES)), ("rows", C.c_int32 * len(OBS_SOURCES))]


def make_observation_sources(tensors: dict) -> AsObservationSources:
    """as_observation_sources_t over {source name: tensor}: field-major (rows, ..., n) tensors, the actions (n, A)."""
    S = AsObservationSources()
    for k, name in enumerate(OBS_SOURCES):
        t = tensors.get(name)
        if t is None:
            continue
        S.ptr[k] = t.data_ptr()
        S.rows[k] = t.shape[1] if name == "actions" else t.numel() // t.shape[-1]
    return S


def observations_step(terms, cols, omap, d0: int, out_cols: int, group: int, sources: AsObservationSources, out,
                      count, t, reset=None, reset2=None, draws=None, seed: int = 0, env_offset: int = 0, stream=None):
    """as_observations_step: one group, one launch.  terms (num_terms, 12) float32 device rows of
    as_observation_term_t, cols (6, 256) float32 words, omap (out_cols,) int32; out (n, out_cols), count (n,) int32,
    t (n,) int32; reset / reset2 (n,) uint8 / bool or None; draws (d0, n) injected or None (Philox)."""
    n = out.shape[0]
    check(load().as_observations_step(terms.data_ptr(), terms.shape[0], cols.data_ptr(), omap.data_ptr(), d0,
                                      out_cols, group, C.byref(sources), out.data_ptr(), count.data_ptr(),
                                      t.data_ptr(), _ptr(reset), _ptr(reset2), n, _ptr(draws),
                                      seed & 0xFFFFFFFFFFFFFFFF, env_offset, stream), "as_observations_step")


def observations_reset(out, count, mask=None, stream=None):
    """as_observations_reset: the push count and the output row of the envs in mask ((n,) uint8 / bool, None: all)
    become 0."""
    n, out_cols = out.shape
    check(load().as_observations_reset(out.data_ptr(), out_cols, count.data_ptr(), _ptr(mask), n, stream),
          "as_observations_reset")


MAX_REW_TERMS = 32  # AS_MAX_REW_TERMS
MAX_REW_IDS = 32  # AS_MAX_REW_IDS: entries of a term's row of the index table
REW_TABLE_ROWS = 3  # AS_REW_TABLE_ROWS: id (int32) | a | b
REW_KINDS = ("is_alive", "is_terminated", "lin_vel_z_l2", "ang_vel_xy_l2", "flat_orientation_l2", "base_height_l2",
             "joint_vel_l1", "joint_vel_l2", "joint_deviation_l1", "joint_pos_limits", "joint_acc_l2", "action_l2",
             "action_rate_l2", "undesired_contacts", "contact_forces", "feet_air_time",
             "feet_air_time_positive_biped", "track_lin_vel_xy_exp", "track_ang_vel_z_exp",
             "track_ang_vel_z_world_exp", "track_lin_vel_xy_yaw_frame_exp")  # AS_REW_*, in order
# as_reward_term_t as 8 32-bit words: kind (int32) | weight (float32) | num_ids, cmd_row (int32) | p0, p1 (float32)
# | two reserved words
REW_TERM_WORDS = 8


class AsRewardSources(C.Structure):
    """as_reward_sources_t (include/allsteps.h): the device rows the reward terms read."""
    _fields_ = [(k, C.c_void_p) for k in ("root_pos", "root_quat", "root_lin", "root_ang", "q", "qd", "qd_prev",
                                          "commands", "net", "timers", "actions", "terminated")] + \
               [(k, C.c_int32) for k in ("joint_rows", "qd_prev_rows", "command_rows", "depth", "bodies",
                                         "timer_bodies", "action_cols", "clamp_actions")] + [("sim_dt", C.c_float)]


def make_reward_sources(tensors: dict, sim_dt: float, clamp_actions: bool = False) -> AsRewardSources:
    """as_reward_sources_t over {name: tensor or None}: root_pos / root_quat / root_lin / root_ang / q / qd / qd_prev
    / commands (rows, n), net (depth, bodies, 3, n), timers (4, bodies, n), actions (n, A), terminated (n,) uint8."""
    S = AsRewardSources()
    for name, _ in AsRewardSources._fields_[:12]:
        t = tensors.get(name)
        if t is not None:
            setattr(S, name, t.data_ptr())
    rows = lambda name, dim=0: 0 if tensors.get(name) is None else int(tensors[name].shape[dim])  # noqa: E731
    S.joint_rows = min(rows("q"), rows("qd"))
    S.qd_prev_rows, S.command_rows = rows("qd_prev"), rows("commands")
    S.depth, S.bodies, S.timer_bodies = rows("net"), rows("net", 1), rows("timers", 1)
    S.action_cols, S.clamp_actions, S.sim_dt = rows("actions", 1), int(bool(clamp_actions)), float(sim_dt)
    return S


def rewards_step(terms, table, kinds: int, sources: AsRewardSources, reward, episode_sums, step_reward,
                 last_episode_sums=None, prev_actions=None, reset=None, reset2=None, dt: float = 0.0, stream=None):
    """as_rewards_step: every term of cfg.rewards in one launch.  terms (num_terms, 8) float32 device rows of
    as_reward_term_t, table (3, 32, 32) float32 words, kinds the bitmask of the kinds the descriptors hold; reward
    (n,), episode_sums / step_reward / last_episode_sums (num_terms, n), prev_actions (n, A); reset / reset2 (n,)
    uint8 / bool or None."""
    check(load().as_rewards_step(terms.data_ptr(), terms.shape[0], table.data_ptr(), kinds, C.byref(sources),
                                 reward.data_ptr(), episode_sums.data_ptr(), step_reward.data_ptr(),
                                 _ptr(last_episode_sums), _ptr(prev_actions), _ptr(reset), _ptr(reset2),
                                 reward.shape[0], dt, stream), "as_rewards_step")


def rewards_reset(episode_sums, prev_actions=None, mask=None, stream=None):
    """as_rewards_reset: the episodic sums (num_terms, n) and prev_actions (n, A) of the envs in mask ((n,) uint8 /
    bool, None: all) become 0."""
    k, n = episode_sums.shape
    check(load().as_rewards_reset(episode_sums.data_ptr(), k, _ptr(prev_actions),
                                  0 if prev_actions is None else prev_actions.shape[1], _ptr(mask), n, stream),
          "as_rewards_reset")


MAX_TERMINATION_TERMS = 16  # AS_MAX_TERMINATION_TERMS
MAX_TERMINATION_IDS = 32  # AS_MAX_TERMINATION_IDS: entries of a term's row of the index table
TERMINATION_TABLE_ROWS = 3  # AS_TERMINATION_TABLE_ROWS: id (int32) | a | b
TERMINATION_KINDS = ("time_out", "command_resample", "bad_orientation", "root_height_below_minimum",
                     "joint_pos_out_of_limit", "joint_pos_out_of_manual_limit", "joint_vel_out_of_manual_limit",
                     "illegal_contact")  # AS_TERMINATION_*, in order
# as_termination_term_t as 8 32-bit words: kind, time_out, num_ids, row (int32) | p0, p1 (float32) | i0 (int32) | one
# reserved word
TERMINATION_TERM_WORDS = 8


class AsTerminationSources(C.Structure):
    """as_termination_sources_t (include/allsteps.h): the device rows the termination terms read."""
    _fields_ = [(k, C.c_void_p) for k in ("root_pos", "root_quat", "q", "qd", "time_left", "command_counter", "net",
                                          "ep_len", "step_terminated", "step_truncated")] + \
               [(k, C.c_int32) for k in ("joint_rows", "command_terms", "depth", "bodies")] + [("sim_dt", C.c_float)]


def make_termination_sources(tensors: dict, sim_dt: float) -> AsTerminationSources:
    """as_termination_sources_t over {name: tensor or None}: root_pos / root_quat / q / qd (rows, n), time_left
    (terms, n) float32 and command_counter (terms, n) int32, net (depth, bodies, 3, n), ep_len (n,) int32,
    step_terminated / step_truncated (n,) uint8."""
    S = AsTerminationSources()
    for name, _ in AsTerminationSources._fields_[:10]:
        t = tensors.get(name)
        if t is not None:
            setattr(S, name, t.data_ptr())
    rows = lambda name, dim=0: 0 if tensors.get(name) is None else int(tensors[name].shape[dim])  # noqa: E731
    # one row count serves a pair of sources: that of whichever is there, the smaller where both are (a source that
    # is not there is NULL and reads as 0)
    both = lambda a, b: min([r for r in (rows(a), rows(b)) if r] or [0])  # noqa: E731
    S.joint_rows = both("q", "qd")
    S.command_terms = both("time_left", "command_counter")
    S.depth, S.bodies, S.sim_dt = rows("net"), rows("net", 1), float(sim_dt)
    return S


def terminations_step(terms, table, kinds: int, sources: AsTerminationSources, term_dones, time_outs, terminated,
                      dones, last_episode_dones=None, reset_request=None, stream=None):
    """as_terminations_step: every term of cfg.terminations in one launch.  terms (num_terms, 8) float32 device rows
    of as_termination_term_t, table (3, 16, 32) float32 words, kinds the bitmask of the kinds the descriptors hold;
    term_dones / last_episode_dones (num_terms, n), time_outs / terminated / dones / reset_request (n,), all uint8."""
    check(load().as_terminations_step(terms.data_ptr(), terms.shape[0], table.data_ptr(), kinds, C.byref(sources),
                                      term_dones.data_ptr(), time_outs.data_ptr(), terminated.data_ptr(),
                                      dones.data_ptr(), _ptr(last_episode_dones), _ptr(reset_request),
                                      dones.shape[0], stream), "as_terminations_step")


ACT_DIM = 21  # AS_ACT_DIM: the most columns of cfg.actions, the most joints of a command row
ACTION_KINDS = ("joint_position", "joint_effort", "position_to_limits", "ema_position_to_limits")  # AS_ACTION_*
# as_action_column_t as 12 32-bit words: joint, kind, rescale, term (int32) | scale, offset, clip_lo, clip_hi, lim_lo,
# lim_hi, alpha, one_minus_alpha (float32)
ACTION_COLUMN_WORDS = 12


def actions_step(cols, inp, action, prev_action, processed, prev_applied, cmd, stream=None):
    """as_actions_step: process_action of every column of cfg.actions in one launch.  cols (num_cols, 12) float32
    device rows of as_action_column_t; inp / action / prev_action / processed / prev_applied (n, num_cols) and cmd
    (n, joints), float32, contiguous."""
    check(load().as_actions_step(cols.data_ptr(), cols.shape[0], inp.data_ptr(), action.data_ptr(),
                                 prev_action.data_ptr(), processed.data_ptr(), prev_applied.data_ptr(),
                                 cmd.data_ptr(), cmd.shape[1], action.shape[0], stream), "as_actions_step")


def actions_reset(cols, action, prev_action, prev_applied, q, mask=None, mask2=None, stream=None):
    """as_actions_reset: ActionManager.reset over the envs of mask | mask2 ((n,) uint8 / bool; neither: every env);
    q (joints, n) float32 the joint positions, cfg dof order."""
    check(load().as_actions_reset(cols.data_ptr(), cols.shape[0], action.data_ptr(), prev_action.data_ptr(),
                                  prev_applied.data_ptr(), q.data_ptr(), q.shape[0], _ptr(mask), _ptr(mask2),
                                  action.shape[0], stream), "as_actions_reset")


def unpack_report_ids(w):
    """(link, link2, stone, foot) of a record's ids word (int array or tensor); -1 = none."""
    return w & 0xFF, (w >> 8 & 0xFF) - 1, (w >> 16 & 0xFF) - 1, (w >> 24 & 0xFF) - 1


def make_body_table(m: dict) -> AsBodyTable:
    t = AsBodyTable()
    nb = int(m["num_bodies"])
    t.num_bodies = nb
    for k in range(nb):
        t.link[k] = int(m["body_link"][k])
        t.offset_pos[k][:] = [float(x) for x in m["body_offset_pos"][k]]
        t.offset_quat[k][:] = [float(x) for x in m["body_offset_quat"][k]]
        t.com[k][:] = [float(x) for x in m["body_com"][k]]
    return t


class AsModel(C.Structure):
    _fields_ = [
        ("num_links", C.c_int32), ("num_hinges", C.c_int32), ("parent", C.c_int32 * MAXL),
        ("offset_pos", (C.c_float * 3) * MAXL), ("offset_quat", (C.c_float * 4) * MAXL),
        ("axis", (C.c_float * 3) * MAXL), ("anchor", (C.c_float * 3) * MAXL), ("mass", C.c_float * MAXL),
        ("com", (C.c_float * 3) * MAXL), ("inertia", (C.c_float * 6) * MAXL), ("armature", C.c_float * MAXL),
        ("lower", C.c_float * MAXL), ("upper", C.c_float * MAXL), ("cfg_dof_link", C.c_int32 * MAXL),
        ("gear", C.c_float * MAXL), ("num_geoms", C.c_int32), ("geom_link", C.c_int32 * MAXG),
        ("geom_type", C.c_int32 * MAXG), ("geom_foot", C.c_int32 * MAXG), ("geom_radius", C.c_float * MAXG),
        ("geom_p0", (C.c_float * 3) * MAXG), ("geom_p1", (C.c_float * 3) * MAXG), ("torso_link", C.c_int32),
        ("foot_link", C.c_int32 * 2), ("num_priority_geoms", C.c_int32), ("num_self_pairs", C.c_int32),
        ("self_pair", C.c_int32 * MAXSP),
    ]


class AsSim(C.Structure):
    _fields_ = [
        ("dt", C.c_float), ("substeps", C.c_int32), ("gravity", C.c_float), ("friction", C.c_float),
        ("margin", C.c_float), ("baumgarte", C.c_float), ("slop", C.c_float), ("max_depen_vel", C.c_float),
        ("pgs_iters", C.c_int32), ("stone_half", C.c_float * 3), ("max_joint_vel", C.c_float),
    ]


class AsTask(C.Structure):
    _fields_ = [
        ("num_steps", C.c_int32), ("step_radius", C.c_float), ("stop_frames", C.c_int32), ("eps", C.c_float),
        ("alive", C.c_float), ("energy", C.c_float), ("action", C.c_float), ("joint_limit", C.c_float),
        ("death", C.c_float), ("dof_vel_scale", C.c_float), ("fall_abs", C.c_float), ("step_dt", C.c_float),
        ("max_episode_length", C.c_int32), ("max_curriculum", C.c_int32), ("curriculum_threshold", C.c_int32),
        ("term_curriculum", C.c_float * 10), ("gain_curriculum", C.c_float * 10), ("init_root", C.c_float * 3),
        ("init_q", C.c_float * 21), ("right_idx", C.c_int32 * 9), ("left_idx", C.c_int32 * 9),
        ("neg_idx", C.c_int32 * 2), ("noise_lo", C.c_float), ("noise_hi", C.c_float), ("clip_lo", C.c_float),
        ("clip_hi", C.c_float), ("regen_footsteps", C.c_int32),
    ]


VP = C.c_void_p


class AsState(C.Structure):
    _fields_ = [(name, VP) for name in (
        "root_pos", "root_quat", "root_lin", "root_ang", "q", "qd", "stones", "pot", "old_pot", "foot_contact",
        "body_pos", "idx", "prev", "next", "count", "swing", "ep_len", "episode", "contact_mask", "curriculum",
        "contact_mask_hind", "feet")]


class AsActuator(C.Structure):
    _fields_ = [("mode", C.c_int32), ("action_scale", C.c_float), ("default_q", C.c_float * 21),
                ("stiffness", C.c_float), ("damping", C.c_float), ("saturation_effort", C.c_float),
                ("effort_limit", C.c_float), ("velocity_limit", C.c_float)]


class AsQuadTask(C.Structure):
    _fields_ = [("stop_frames", C.c_int32), ("alive", C.c_float), ("action_cost", C.c_float), ("death", C.c_float),
                ("min_height", C.c_float), ("up_z_min", C.c_float), ("max_episode_length", C.c_int32),
                ("step_dt", C.c_float), ("stand_height", C.c_float), ("joint_noise", C.c_float),
                ("energy_cost", C.c_float), ("step_radius", C.c_float), ("step_reward", C.c_float),
                ("step_sigma", C.c_float), ("target_bonus", C.c_float), ("bonus_radius", C.c_float),
                ("foot_progress", C.c_float), ("foot_offset_y", C.c_float * 4)]


ACT_TORQUE, ACT_DC_MOTOR = 0, 1
QUAD_OBS_DIM = 64


# (field, rows, dtype) of the SoA state, in as_state_t order
STATE_LAYOUT = [
    ("root_pos", 3, "f"), ("root_quat", 4, "f"), ("root_lin", 3, "f"), ("root_ang", 3, "f"), ("q", 21, "f"),
    ("qd", 21, "f"), ("stones", 60, "f"), ("pot", 1, "f"), ("old_pot", 1, "f"), ("foot_contact", 2, "f"),
    ("body_pos", 9, "f"), ("idx", 1, "i"), ("prev", 1, "i"), ("next", 1, "i"), ("count", 1, "i"),
    ("swing", 1, "i"), ("ep_len", 1, "i"), ("episode", 1, "i"), ("contact_mask", 2, "i"),
]

_LIB = None


def lib_path() -> str:
    return os.environ.get("ALLSTEPS_HIP_LIB", LIB_PATH)


def source_digest() -> str:
    """Provenance digest of the native sources: sha256 over every csrc/*.hip, csrc/*.h and include/*.h
    (name + bytes, sorted by name) and both libraries' compile flags (include path excluded, so the
    digest is the same in any checkout), first 16 hex digits.  build_native() compiles it into
    both libraries (as_build_id / ppo_build_id); load() refuses a library whose id differs."""
    import hashlib

    h = hashlib.sha256()
    files = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".hip", ".h"))]
    files += [os.path.join(INCLUDE, f) for f in os.listdir(INCLUDE) if f.endswith(".h")]
    for path in sorted(files, key=os.path.basename):
        h.update(os.path.basename(path).encode() + b"\0")
        with open(path, "rb") as f:
            h.update(f.read())
        h.update(b"\0")
    for flags in (STEP_FLAGS, PPO_FLAGS):
        h.update(" ".join(x for x in flags if x != INCLUDE).encode() + b"\0")
    return h.hexdigest()[:16]


def check_build_id(lib_id: bytes | str, path: str, env_var: str) -> None:
    """Raise NativeError when the library at `path` was not built from this tree's sources, unless the
    caller chose the library explicitly through `env_var` (A/B variants, diagnostic builds)."""
    if env_var in os.environ:
        return
    got = lib_id.decode(errors="replace") if isinstance(lib_id, bytes) else str(lib_id)
    want = source_digest()
    if got != want:
        raise NativeError(f"{path} was built from other sources (build id {got}, this tree {want}): rebuild it "
                          f"(`python -c 'import __graft_entry__ as g; g.build()'`), or set {env_var} to load a "
                          f"variant on purpose")


def load() -> C.CDLL:
    """Load liballsteps_hip.so (raises NativeError if it is missing: build it with build_native())."""
    global _LIB
    if _LIB is not None:
        return _LIB
    path = lib_path()
    if not os.path.exists(path):
        raise NativeError(f"{path} not found: the HIP extension is not built "
                          f"(run `python -c 'import __graft_entry__ as g; g.build()'`)")
    L = C.CDLL(path)
    V, I32, I64, U64 = C.c_void_p, C.c_int32, C.c_int64, C.c_uint64
    L.as_create.argtypes = [I32, V, V, V, V, U64, I32, I64, C.POINTER(V)]
    L.as_destroy.argtypes = [V]
    L.as_reset_all.argtypes = [V, V, V, V]
    L.as_reset_mask.argtypes = [V, V, V, V, V]
    L.as_step.argtypes = [V, V, V, V, V, V, V, V]
    L.as_physics_step.argtypes = [V, V, V]
    L.as_task_step.argtypes = [V, V, V, V, V, V, V, V]
    L.as_set_seed.argtypes = [V, U64]
    L.as_set_graph_safe.argtypes = [V, I32]
    L.as_profile.argtypes = [V, I32]
    L.as_profile_sampled.argtypes = [V, I32, I32]
    L.as_debug_stamps.argtypes = [V, V]
    L.as_profile_read.argtypes = [V, C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(I32)]
    L.as_generate_stones.argtypes = [V, I32, V, V]
    L.as_step_counters.argtypes = [V, C.POINTER(V)]
    L.as_get_curriculum_host.argtypes = [V, C.POINTER(I32)]
    L.as_step_counters_host.argtypes = [V, C.POINTER(I32), V]
    L.as_hbm_copy.argtypes = [V, V, I64, V]
    L.as_set_actuator.argtypes = [V, V]
    L.as_set_quad_task.argtypes = [V, V]
    L.as_quad_step.argtypes = [V, V, V, V, V, V, V]
    L.as_quad_reset_all.argtypes = [V, V, V]
    L.as_quad_reset_mask.argtypes = [V, V, V, V]
    L.as_body_state.argtypes = [V, V, V, V]
    L.as_sweep_plan.argtypes = [V, C.POINTER(C.c_uint64)]
    L.as_set_contact_report.argtypes = [V, V]
    L.as_contact_forces.argtypes = [V, V, V, V, V]
    L.as_contact_timers.argtypes = [V, V, V, V, C.c_float, I32, V, V, V]
    L.as_ray_cast.argtypes = [V, V, V, V, V, V, V]
    L.as_imu.argtypes = [V, V, C.c_float, I32, V, V, V, V]
    L.as_frame_transformer.argtypes = [V, V, V, V, V]
    L.as_ray_camera.argtypes = [V, V, V, V, V, V, V, V, V]
    L.as_noise_actions.argtypes = [V, V, V, I32, I32, V, V, U64, I64, V]
    L.as_noise_post.argtypes = [V, V, V, I32, I32, V, V, V, V, V, V, U64, I64, V]
    L.as_events_init.argtypes = [V, I32, V, V, I32, V, U64, I64, V]
    L.as_events_interval.argtypes = [V, I32, V, V, V, V, V, I32, C.c_float, V, V, U64, I64, V]
    L.as_commands_step.argtypes = [V, I32, V, V, V, V, V, V, V, V, V, V, V, V, V, I32, C.c_float, V, U64, I64, V]
    L.as_commands_reset.argtypes = [V, I32, V, V, V, V, V, V, V, V, V, I32, V, U64, I64, V]
    L.as_observations_step.argtypes = [V, I32, V, V, I32, I32, I32, V, V, V, V, V, V, I32, V, U64, I64, V]
    L.as_observations_reset.argtypes = [V, I32, V, V, I32, V]
    L.as_rewards_step.argtypes = [V, I32, V, C.c_uint32, V, V, V, V, V, V, V, V, I32, C.c_float, V]
    L.as_rewards_reset.argtypes = [V, I32, V, I32, V, I32, V]
    L.as_terminations_step.argtypes = [V, I32, V, C.c_uint32, V, V, V, V, V, V, V, I32, V]
    L.as_actions_step.argtypes = [V, I32, V, V, V, V, V, V, I32, I32, V]
    L.as_actions_reset.argtypes = [V, I32, V, V, V, V, I32, V, V, I32, V]
    L.as_set_joint_commands.argtypes = [V, V]
    L.as_last_error.restype = C.c_char_p
    L.as_build_id.restype = C.c_char_p
    for name in EXPORTED_SYMBOLS:
        if name not in ("as_last_error", "as_build_id"):
            getattr(L, name).restype = C.c_int
    if L.as_abi_version() != ABI_VERSION:
        raise NativeError(f"ABI version mismatch: library {L.as_abi_version()} != {ABI_VERSION}")
    check_build_id(L.as_build_id(), path, "ALLSTEPS_HIP_LIB")
    _LIB = L
    return L


def check(rc: int, what: str) -> None:
    if rc != 0:
        msg = load().as_last_error().decode(errors="replace")
        raise NativeError(f"{what} failed ({rc}): {msg}")


def hbm_copy_bandwidth(device, nbytes: int = 2 << 30, iters: int = 20) -> float:
    """Achievable HBM bandwidth (GB/s, read + write bytes) of the in-tree STREAM-copy kernel
    (as_hbm_copy) between two `nbytes` device buffers, timed with HIP events on the current stream."""
    import torch

    L = load()
    n16 = nbytes // 16
    src = torch.empty(n16 * 4, dtype=torch.float32, device=device).uniform_()
    dst = torch.empty_like(src)
    stream = torch.cuda.current_stream(device)
    sp = C.c_void_p(stream.cuda_stream)
    for _ in range(3):
        check(L.as_hbm_copy(C.c_void_p(dst.data_ptr()), C.c_void_p(src.data_ptr()), n16, sp), "as_hbm_copy")
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    for _ in range(iters):
        check(L.as_hbm_copy(C.c_void_p(dst.data_ptr()), C.c_void_p(src.data_ptr()), n16, sp), "as_hbm_copy")
    e1.record(stream)
    e1.synchronize()
    ok = bool(torch.equal(src, dst))
    ms = e0.elapsed_time(e1) / iters
    del src, dst
    if not ok:
        raise NativeError("as_hbm_copy: destination differs from source")
    return 2.0 * n16 * 16 / (ms * 1e-3) / 1e9


# the step library's device-code flags (tests/test_kernel_budget.py compiles with exactly these):
# -ffp-contract=off: no implicit FMA contraction -- every FMA of the physics path is an explicit fmaf()
# in the order include/as_detmath.h fixes, so the oracle (built the same way) rounds identically and
# HIP <-> oracle parity is bit-exact.  -fno-slp-vectorize: the SLP pairs of the step kernel's scalar
# code cost more register moves than they save (launch -2 %); the packed math that pays
# (sweep, W rows) is written out as 2-vectors
STEP_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-slp-vectorize", "-I", INCLUDE]
PPO_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fno-slp-vectorize", "-I", INCLUDE]


def build_native(verbose: bool = False) -> str:
    """Compile liballsteps_hip.so and libppo_hip.so for gfx950 in-tree (hipcc)."""
    import subprocess

    srcs = [os.path.join(CSRC, f) for f in ("allsteps_kernels.hip", "allsteps_abi.hip")]
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    digest = source_digest()
    cmd = [hipcc, *STEP_FLAGS, f'-DAS_BUILD_ID="{digest}"', "-fPIC", "-shared", "-Wno-unused-result", "-o",
           LIB_PATH] + srcs
    if verbose:
        print(" ".join(cmd))
    subprocess.run(cmd, check=True)
    # PPO-update kernels (include/ppo.h) -> libppo_hip.so
    cmd = [hipcc, *PPO_FLAGS, f'-DPPO_BUILD_ID="{digest}"', "-fPIC", "-shared", "-Wno-unused-result",
           "-o", PPO_LIB_PATH, os.path.join(CSRC, "ppo_kernels.hip"), os.path.join(CSRC, "ppo_mlp.hip"),
           os.path.join(CSRC, "ppo_wgrad.hip")]
    if verbose:
        print(" ".join(cmd))
    subprocess.run(cmd, check=True)
    return LIB_PATH


# ------------------------------------------------------------------------------------------ structs

def sweep_plan(m: dict) -> tuple[int, int]:
    """as_sweep_plan: (1 if the step kernel's compiled sweep skips hold for model `m`, else 0; the mask of
    column quads that are exactly zero for it).  Host-only (no device)."""
    L = load()
    M = make_model(m)
    mask = C.c_uint64(0)
    rc = L.as_sweep_plan(C.byref(M), C.byref(mask))
    if rc < 0:
        raise NativeError(L.as_last_error().decode())
    return rc, int(mask.value)


def make_model(m: dict) -> AsModel:
    M = AsModel()
    M.num_links = m["num_links"]
    M.num_hinges = m["num_hinges"]
    for name in ("parent", "cfg_dof_link", "geom_link", "geom_type", "geom_foot"):
        getattr(M, name)[:] = [int(x) for x in m[name]]
    for name in ("mass", "armature", "lower", "upper", "gear", "geom_radius"):
        getattr(M, name)[:] = [float(x) for x in m[name]]
    for name in ("offset_pos", "offset_quat", "axis", "anchor", "com", "inertia", "geom_p0", "geom_p1"):
        arr = getattr(M, name)
        for i, row in enumerate(m[name]):
            arr[i][:] = [float(x) for x in row]
    M.num_geoms = m["num_geoms"]
    M.num_priority_geoms = int(m["num_priority_geoms"])
    M.num_self_pairs = int(m["num_self_pairs"])
    M.self_pair[:] = [int(x) for x in m["self_pair"]]
    M.torso_link = int(m["torso_link"])
    M.foot_link[:] = [int(x) for x in m["foot_link"]]
    return M


from .envs.task_table import linspace_f32  # noqa: E402  (re-exported: allsteps_env.py)


def make_task(cfg, dof_names: list) -> AsTask:
    """as_task_t from the cfg (envs/task_table.py: shared with the oracle, dispatched on the cfg type)."""
    from allsteps_isaaclab_amd.envs.task_table import fill, task_fields

    return fill(AsTask(), task_fields(cfg, dof_names))


def make_sim(cfg) -> AsSim:
    S = AsSim()
    s = cfg.sim
    S.dt = s.dt
    S.substeps = cfg.decimation
    S.gravity = s.gravity[2]
    S.friction = s.friction
    S.margin = s.contact_margin
    S.baumgarte = s.baumgarte
    S.slop = s.slop
    S.max_depen_vel = s.max_depenetration_velocity
    S.pgs_iters = s.solver_position_iteration_count
    sz = cfg.step_size
    S.stone_half[:] = [sz[0] / 2, sz[1] / 2, sz[2] / 2]
    S.max_joint_vel = s.max_joint_velocity
    return S


class NativeEnv:
    """Owns an ``as_env_t`` handle over caller-owned (torch) SoA state tensors."""

    def __init__(self, n: int, model: dict, cfg, state: dict, seed: int, device_index: int, env_offset: int = 0):
        self.L = load()
        self.n = n
        self._model = make_model(model)
        self._sim = make_sim(cfg)
        self._task = make_task(cfg, model["dof_names"])
        self._state_tensors = state  # keep alive
        S = AsState()
        for name, _, _ in STATE_LAYOUT:
            setattr(S, name, state[name].data_ptr())
        S.curriculum = state["curriculum"].data_ptr()
        S.contact_mask_hind = _ptr(state.get("contact_mask_hind"))
        S.feet = _ptr(state.get("feet"))
        self._state = S
        h = C.c_void_p()
        check(self.L.as_create(n, C.byref(self._model), C.byref(self._sim), C.byref(self._task), C.byref(S),
                               seed & 0xFFFFFFFFFFFFFFFF, device_index, env_offset, C.byref(h)), "as_create")
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            self.L.as_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def step(self, actions, obs, rew, term, trunc, reset_draws=None, stream=None):
        check(self.L.as_step(self.h, actions.data_ptr(), obs.data_ptr(), rew.data_ptr(), term.data_ptr(),
                             trunc.data_ptr(), _ptr(reset_draws), stream), "as_step")

    def task_step(self, actions, obs, rew, term, trunc, reset_draws=None, stream=None):
        check(self.L.as_task_step(self.h, actions.data_ptr(), obs.data_ptr(), rew.data_ptr(), term.data_ptr(),
                                  trunc.data_ptr(), _ptr(reset_draws), stream), "as_task_step")

    def set_seed(self, seed: int):
        check(self.L.as_set_seed(self.h, seed & 0xFFFFFFFFFFFFFFFF), "as_set_seed")

    def set_graph_safe(self, on: bool):
        check(self.L.as_set_graph_safe(self.h, int(bool(on))), "as_set_graph_safe")

    def reset_all(self, obs, reset_draws=None, stream=None):
        check(self.L.as_reset_all(self.h, obs.data_ptr(), _ptr(reset_draws), stream), "as_reset_all")

    def reset_mask(self, mask, obs, reset_draws=None, stream=None):
        check(self.L.as_reset_mask(self.h, mask.data_ptr(), obs.data_ptr(), _ptr(reset_draws), stream),
              "as_reset_mask")

    def physics_step(self, actions, stream=None):
        check(self.L.as_physics_step(self.h, actions.data_ptr(), stream), "as_physics_step")

    def body_state(self, table: "AsBodyTable", out, stream=None):
        """as_body_state: out [BODY_STATE_ROWS][num_bodies][n] fp32 on the device (ring-2 body views)."""
        check(self.L.as_body_state(self.h, C.byref(table), out.data_ptr(), stream), "as_body_state")

    def set_contact_report(self, depth: int = 0, count=None, records=None, qd_prev=None):
        """as_set_contact_report over caller-owned device tensors: count int32 [depth][n], records int32
        [depth][REPORT_WORDS][MAXC][n], qd_prev fp32 [21][n] (kept alive here); no tensors: report off."""
        if count is None and records is None and qd_prev is None:
            self._report = None
            check(self.L.as_set_contact_report(self.h, None), "as_set_contact_report")
            return
        R = AsContactReport()
        R.depth = int(depth)
        R.count, R.records, R.qd_prev = (_ptr(t) for t in (count, records, qd_prev))
        check(self.L.as_set_contact_report(self.h, C.byref(R)), "as_set_contact_report")
        self._report = (R, count, records, qd_prev)

    def set_joint_commands(self, cmd=None):
        """as_set_joint_commands: every later physics launch reads its joint commands from cmd, float32 (n, joints)
        on the device (kept alive here), in place of the actuator's own formula; None: off."""
        if cmd is not None and (tuple(cmd.shape) != (self.n, int(self._model.num_hinges)) or
                                not cmd.is_contiguous() or str(cmd.dtype) != "torch.float32" or not cmd.is_cuda):
            raise NativeError(f"as_set_joint_commands: cmd must be a contiguous float32 device tensor of shape "
                              f"({self.n}, {int(self._model.num_hinges)})")
        check(self.L.as_set_joint_commands(self.h, _ptr(cmd)), "as_set_joint_commands")
        self._joint_cmd = cmd

    def contact_forces(self, table: "AsBodyTable", force_matrix_out, net_out, stream=None):
        """as_contact_forces: force_matrix_out fp32 [depth][REPORT_FEET][NUM_STONES][3][n], net_out fp32
        [depth][num_bodies][3][n] (impulses, N s) from the report as it stands."""
        check(self.L.as_contact_forces(self.h, C.byref(table) if table is not None else None,
                                       _ptr(force_matrix_out), _ptr(net_out), stream), "as_contact_forces")

    def contact_timers(self, table: "AsBodyTable", timers, timestamp, force_threshold: float, updates: int,
                       reset=None, reset2=None, stream=None):
        """as_contact_timers: `updates` (0 or the report's depth) sensor updates of timers fp32 [TIMER_ROWS]
        [num_bodies][n] and timestamp fp32 [n] from the report as it stands, then the reset of the envs in reset |
        reset2 ([n] uint8 / bool; reset None: all when updates == 0, none otherwise)."""
        check(self.L.as_contact_timers(self.h, C.byref(table) if table is not None else None, _ptr(timers),
                                       _ptr(timestamp), force_threshold, int(updates), _ptr(reset), _ptr(reset2),
                                       stream), "as_contact_timers")

    def ray_cast(self, cfg: "AsRayCaster", rays, hits, surface=None, pose=None, stream=None):
        """as_ray_cast: the rays fp32 [6][num_rays] (device) from every env's root frame against the ground and the
        stones of the state as it stands; hits fp32 [3][num_rays][n], surface int8 [num_rays][n] or None, pose
        fp32 [7][n] or None."""
        check(self.L.as_ray_cast(self.h, C.byref(cfg) if cfg is not None else None, _ptr(rays), _ptr(hits),
                                 _ptr(surface), _ptr(pose), stream), "as_ray_cast")

    def ray_camera(self, cfg: "AsRayCamera", dirs, offset, pose, plane=None, camera=None, normals=None, stream=None):
        """as_ray_camera: the pixels' local directions fp32 [3][R] and the per-env offsets fp32 [7][n] (device) from
        every env's root frame against the ground and the stones; writes pose [7][n] and the images that are not
        None -- plane, camera [n][R], normals [n][R][3], env-major -- one launch on `stream`."""
        check(self.L.as_ray_camera(self.h, C.byref(cfg) if cfg is not None else None, _ptr(dirs), _ptr(offset),
                                   _ptr(pose), _ptr(plane), _ptr(camera), _ptr(normals), stream), "as_ray_camera")

    def imu(self, table: "AsImuTable", dt: float, all_envs: bool, outdated, data, prev, stream=None):
        """as_imu: the IMU update of every sensor of `table` for the envs flagged in outdated uint8 [n] (all_envs:
        every env), flags cleared; data fp32 [IMU_DATA_ROWS][S][n], prev fp32 [IMU_PREV_ROWS][S][n]."""
        check(self.L.as_imu(self.h, C.byref(table) if table is not None else None, dt, int(bool(all_envs)),
                            _ptr(outdated), _ptr(data), _ptr(prev), stream), "as_imu")

    def frame_transformer(self, table: "AsFrameTable", source, target, stream=None):
        """as_frame_transformer: every target frame of every sensor of `table` from the state as it stands; source
        fp32 [FRAME_SOURCE_ROWS][S][n], target fp32 [FRAME_TARGET_ROWS][F][n]."""
        check(self.L.as_frame_transformer(self.h, C.byref(table) if table is not None else None, _ptr(source),
                                          _ptr(target), stream), "as_frame_transformer")

    def set_actuator(self, mode: int, action_scale: float = 0.0, default_q=(), stiffness: float = 0.0,
                     damping: float = 0.0, saturation_effort: float = 0.0, effort_limit: float = 0.0,
                     velocity_limit: float = 0.0):
        A = AsActuator()
        A.mode, A.action_scale = mode, action_scale
        A.default_q[: len(default_q)] = [float(x) for x in default_q]
        A.stiffness, A.damping = stiffness, damping
        A.saturation_effort, A.effort_limit, A.velocity_limit = saturation_effort, effort_limit, velocity_limit
        self._act = A
        check(self.L.as_set_actuator(self.h, C.byref(A)), "as_set_actuator")

    def set_quad_task(self, **kw):
        Q = AsQuadTask()
        for k, v in kw.items():
            if isinstance(v, (list, tuple)):
                getattr(Q, k)[:] = [float(x) for x in v]
            else:
                setattr(Q, k, v)
        self._quad = Q
        check(self.L.as_set_quad_task(self.h, C.byref(Q)), "as_set_quad_task")

    def quad_step(self, actions, obs, rew, term, trunc, stream=None):
        check(self.L.as_quad_step(self.h, actions.data_ptr(), obs.data_ptr(), rew.data_ptr(), term.data_ptr(),
                                  trunc.data_ptr(), stream), "as_quad_step")

    def quad_reset_all(self, obs, stream=None):
        check(self.L.as_quad_reset_all(self.h, obs.data_ptr(), stream), "as_quad_reset_all")

    def quad_reset_mask(self, mask, obs, stream=None):
        """as_quad_reset_mask: mask (n,) uint8 on the device; only the masked envs' rows of obs are written."""
        check(self.L.as_quad_reset_mask(self.h, mask.data_ptr(), obs.data_ptr(), stream), "as_quad_reset_mask")

    def generate_stones(self, level: int, draws=None, stream=None):
        check(self.L.as_generate_stones(self.h, level, _ptr(draws), stream), "as_generate_stones")

    def profile_sampled(self, max_records: int, stride: int):
        check(self.L.as_profile_sampled(self.h, max_records, stride), "as_profile_sampled")

    def profile(self, max_launches: int):
        check(self.L.as_profile(self.h, max_launches), "as_profile")

    def profile_read(self):
        a, b, k = C.c_double(), C.c_double(), C.c_int32()
        check(self.L.as_profile_read(self.h, C.byref(a), C.byref(b), C.byref(k)), "as_profile_read")
        return a.value, b.value, k.value

    def debug_stamps(self, buf):
        check(self.L.as_debug_stamps(self.h, _ptr(buf)), "as_debug_stamps")

    def counters_host(self, stream=None) -> list:
        """The last step's counter words [any reset, target-index sum, regen level, contacts dropped]
        (synchronises `stream`)."""
        out = (C.c_int32 * 4)()
        check(self.L.as_step_counters_host(self.h, out, stream), "as_step_counters_host")
        return list(out)

    def counters_ptr(self) -> int:
        p = C.c_void_p()
        check(self.L.as_step_counters(self.h, C.byref(p)), "as_step_counters")
        return p.value
