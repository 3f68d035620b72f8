/*
 * allsteps.h -- C ABI of the MI355X-native Allsteps-v0 step (liballsteps_hip.so).
 *
 * The reference's hot path is DirectRLEnv.step (isaaclab/envs/direct_rl_env.py:296-383) over the
 * Allsteps task (isaaclab_tasks/direct/allsteps/allsteps_env.py:257-567), whose physics half is
 * the omni.physics.tensors / PhysX operator surface (SURVEY.md §8b "Ring 3"):
 *   set_dof_actuation_forces      (articulation.py:195)          -> as_step (actions in, torque inside)
 *   SimulationContext.step / simulate(dt) x decimation (simulation_context.py:453-478) -> as_step
 *   get_root_transforms / get_root_velocities / get_dof_positions / get_dof_velocities
 *       (articulation_data.py:374-376, 533, 542)                -> state views (as_state_t)
 *   update_articulations_kinematic (articulation_data.py:439)   -> fused FK inside as_step
 *   RigidContactView.get_contact_force_matrix (contact_sensor.py:341) -> contact_mask (as_state_t);
 *       the forces themselves, get_net_contact_forces (contact_sensor.py:329) and joint_acc
 *       (articulation_data.py:547-556) from the opt-in contact report (ABI 6: as_set_contact_report,
 *       as_contact_forces)
 *   set_root_* / set_dof_* on reset (articulation.py:316-341, 400-420, 472-551) -> in-kernel reset
 * and the task code around it (_apply_action, _get_dones, _get_rewards, _reset_idx,
 * _get_observations), fused into two kernels per env step.
 *
 * Conventions: every buffer argument is a DEVICE pointer unless its name ends in _host; the caller
 * owns all buffers (state included, see as_state_t) and keeps them alive for the handle's life;
 * `stream` is a hipStream_t (NULL = default stream).  Calls on one handle are serialised by the
 * caller.  No call synchronises the stream except as_get_curriculum_host.  Every function returns 0
 * on success or a negative AS_ERR_* code; as_last_error() gives a message (thread-local).
 */
#ifndef ALLSTEPS_H
#define ALLSTEPS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AS_ABI_VERSION 6
#define AS_MAX_LINKS 32
#define AS_MAX_GEOMS 32
#define AS_MAX_SELF_PAIRS 256
/* envs per handle: the kernels index the field-major state and the [5][n][20] draw tables with 32-bit
 * offsets (row * n + env, < 2^31); 2^24 envs is ~22 GB of state, far past one GPU's useful launch */
#define AS_MAX_ENVS (1 << 24)
#define AS_NUM_STONES 20
/* Constraint budget per env and substep: every active joint-limit row is kept (a walker has at most
 * 21, one side per hinge); contacts fill the remaining rows three at a time up to AS_MAX_CONTACTS, in
 * priority order: feet on stones, other geoms on stones, robot self-contacts. */
#define AS_MAX_CONTACTS 10
#define AS_MAX_ROWS 30
#define AS_OBS_DIM 59
#define AS_ACT_DIM 21
#define AS_QUAD_OBS_DIM 64

enum {
  AS_OK = 0,
  AS_ERR_INVALID = -1,   /* bad argument (null pointer, size out of range, model too large) */
  AS_ERR_HIP = -2,       /* HIP runtime error (message has the hipError string) */
  AS_ERR_NO_DEVICE = -3, /* no gfx950 device / code object for this device */
};

/* Robot model tables (allsteps_isaaclab_amd/model/walker3d.json; compiled from walker3d.xml). */
typedef struct {
  int32_t num_links;                  /* incl. floating root = link 0; link i >= 1 carries hinge i-1 */
  int32_t num_hinges;                 /* num_links - 1 (== AS_ACT_DIM for the walker) */
  int32_t parent[AS_MAX_LINKS];       /* topological: parent[i] < i */
  float offset_pos[AS_MAX_LINKS][3];
  float offset_quat[AS_MAX_LINKS][4]; /* (w, x, y, z) */
  float axis[AS_MAX_LINKS][3];
  float anchor[AS_MAX_LINKS][3];
  float mass[AS_MAX_LINKS];
  float com[AS_MAX_LINKS][3];
  float inertia[AS_MAX_LINKS][6];     /* about COM, link frame: xx yy zz xy xz yz */
  float armature[AS_MAX_LINKS];
  float lower[AS_MAX_LINKS];
  float upper[AS_MAX_LINKS];
  int32_t cfg_dof_link[AS_MAX_LINKS]; /* PhysX/cfg dof k -> link */
  float gear[AS_MAX_LINKS];           /* cfg order (allsteps_env_cfg.py:133-155) */
  int32_t num_geoms;
  int32_t geom_link[AS_MAX_GEOMS];
  int32_t geom_type[AS_MAX_GEOMS];    /* 0 sphere, 1 capsule */
  int32_t geom_foot[AS_MAX_GEOMS];    /* contact sensor 0..3 or -1 (walker: 0 right, 1 left foot;
                                         quadruped: RF, LF, RH, LH) */
  float geom_radius[AS_MAX_GEOMS];
  float geom_p0[AS_MAX_GEOMS][3];
  float geom_p1[AS_MAX_GEOMS][3];
  int32_t torso_link;
  int32_t foot_link[2];
  int32_t num_priority_geoms;         /* geoms [0, n) (the feet) emit their stone contacts first */
  int32_t num_self_pairs;             /* self-collision geom pairs (walker3d.py:27 enabled_self_collisions) */
  int32_t self_pair[AS_MAX_SELF_PAIRS]; /* g1 | g2 << 8, g1 < g2, ascending (model/__init__.py) */
} as_model_t;

/* Physics constants (simulation_cfg.py; walker3d.py:21-46; allsteps_env_cfg.py:62). */
typedef struct {
  float dt;
  int32_t substeps;
  float gravity;
  float friction;
  float margin;
  float baumgarte;
  float slop;
  float max_depen_vel;
  int32_t pgs_iters;
  float stone_half[3];
  float max_joint_vel;
} as_sim_t;

/* Task constants (allsteps_env.py:29-60; allsteps_env_cfg.py:54-234). */
typedef struct {
  int32_t num_steps;
  float step_radius;
  int32_t stop_frames;
  float eps;
  float alive, energy, action, joint_limit, death, dof_vel_scale, fall_abs;
  float step_dt;
  int32_t max_episode_length;
  int32_t max_curriculum;
  int32_t curriculum_threshold;
  float term_curriculum[10];
  float gain_curriculum[10];
  float init_root[3];
  float init_q[21];
  int32_t right_idx[9], left_idx[9], neg_idx[2];
  float noise_lo, noise_hi, clip_lo, clip_hi;
  /* 0 = reference behaviour (stones never regenerate: _reset_idx resets curr_target_index before its
   * over-half test, allsteps_env.py:492-500); 1 = the intended behaviour: a reset
   * env whose target index was > num_steps / 2 gets new stones at the (post-gate) curriculum level */
  int32_t regen_footsteps;
} as_task_t;

/* Per-env state: structure of arrays, field-major / env-minor ([field][num_envs]), device memory,
 * caller-owned.  These are the ArticulationData views of the reference:
 *   root_pos/root_quat  = root_state_w[:, 0:7]  (root link frame, quat w,x,y,z)
 *   root_lin/root_ang   = root_state_w[:, 7:13] (root link COM velocity, world)
 *   q / qd              = joint_pos / joint_vel (cfg dof order)
 *   body_pos            = body_pos_w[:, {torso, right_foot, left_foot}]
 * and the AllstepsEnv task buffers (allsteps_env.py:66-96). */
typedef struct {
  float* root_pos;      /* [3][n] */
  float* root_quat;     /* [4][n] */
  float* root_lin;      /* [3][n] */
  float* root_ang;      /* [3][n] */
  float* q;             /* [21][n] */
  float* qd;            /* [21][n] */
  float* stones;        /* [20*3][n]  steps_pos, env-local frame (env origin = 0) */
  float* pot;           /* [n] potentials */
  float* old_pot;       /* [n] old_potentials */
  float* foot_contact;  /* [2][n] */
  float* body_pos;      /* [9][n] */
  int32_t* idx;         /* [n] curr_target_index */
  int32_t* prev;        /* [n] */
  int32_t* next;        /* [n] */
  int32_t* count;       /* [n] target_reach_count */
  int32_t* swing;       /* [n] swing_leg */
  int32_t* ep_len;      /* [n] episode_length_buf */
  uint32_t* episode;    /* [n] reset counter: Philox stream of the reset draws */
  uint32_t* contact_mask; /* [2][n] per-foot bitmask of stones with force > eps, last substep */
  int32_t* curriculum;  /* [1] */
  uint32_t* contact_mask_hind; /* [2][n] contact sensors 2 and 3 (a quadruped's hind feet), or NULL */
  int32_t* feet;        /* [8][n] the quadruped task's per-foot target stones (rows 0..3, sensor order)
                           and reach counts (rows 4..7), or NULL (the walker) */
} as_state_t;

/* Actuation of the physics step (as_set_actuator; as_create starts in AS_ACT_TORQUE).
 *   AS_ACT_TORQUE:   tau = gain_curriculum[level] * gear * clip(a, -1, 1)  (the Allsteps walker,
 *                    allsteps_env.py:267-274, an ImplicitActuator with kp = kd = 0);
 *   AS_ACT_DC_MOTOR: joint position targets q* = default_q + action_scale * clip(a, -1, 1)
 *                    (anymal_c_env.py:73-78), tracked by IsaacLab's DCMotor actuator evaluated in
 *                    every physics substep: tau = kp (q* - q) + kd (0 - qd)  (IdealPD,
 *                    actuator_pd.py:184-199), clipped to [tau_min(qd), tau_max(qd)] with
 *                    tau_max = clip(sat (1 - qd / v_max), 0, effort_limit),
 *                    tau_min = clip(sat (-1 - qd / v_max), -effort_limit, 0)  (actuator_pd.py:264-275). */
enum { AS_ACT_TORQUE = 0, AS_ACT_DC_MOTOR = 1 };
typedef struct {
  int32_t mode;
  float action_scale;
  float default_q[AS_ACT_DIM];   /* cfg dof order */
  float stiffness, damping;
  float saturation_effort, effort_limit, velocity_limit;
} as_actuator_t;

/* The BASELINE C5 task: a quadruped crossing the Allsteps stones with the ALLSTEPS reward terms
 * (allsteps_env.py:347-394) and the reference's target machine (:418-457) run per foot (authored here --
 * the reference has no quadruped stepping-stone task; its ANYmal-C task is flat-ground velocity
 * tracking).  Per env step, after the physics substeps:
 *   feet: every sensor foot f (0..3 = RF, LF, RH, LH) has its own target stone t_f (state.feet rows
 *     0..3; 2 for the front feet and 1 for the hind feet after a reset: they stand on stones 1 / 0) and
 *     reach count c_f (rows 4..7); its aim point is stone t_f's centre + (0, foot_offset_y[f]), its
 *     position the tip of its sensor geom (the capsule end p1, FK from q: as_link_point);
 *   target tick per foot (allsteps_env.py:418-440): reached = f pushes on t_f (contact mask bit) and
 *     its xy distance d to the aim point < step_radius; c_f += reached; c_f >= stop_frames: c_f = 0,
 *     t_f += 1 (clamped); the front pair's target idx = min(t_RF, t_LF) (state.idx);
 *   potential (:441-448): pot = -(|stone[idx] - root|_xy + foot_progress sum_f d_f) / step_dt, d_f
 *     the foot's distance to its (updated) aim point;
 *   terminated = body tilted past up_z_min or below the target stone + min_height; truncated at
 *     max_episode_length;
 *   reward (:347-394) = alive + (pot - old_pot) - energy_cost sum|qd a| - action_cost ||a||
 *     + sum_f step_reward exp(-d_f / step_sigma) over the feet with a fresh reach (c_f == 1, t_f <
 *     num_steps - 1) + target_bonus when idx is the last stone and the root is within bonus_radius of
 *     it (xy); death on termination;
 * reset of done envs to the stand pose over stones 0 / 1 (+ U(-1,1) * joint_noise, Philox); observation
 * [64] = root linear / angular velocity (body frame), projected gravity, each foot's aim point and
 * stone idx + 1 relative to the root (body frame), each foot's contact with its target stone [4],
 * q - default_q, qd, the clipped actions. */
typedef struct {
  int32_t stop_frames;
  float alive, action_cost, death;
  float min_height, up_z_min;
  int32_t max_episode_length;
  float step_dt;
  float stand_height;       /* root z above the higher of stones 0 / 1's top face at reset */
  float joint_noise;
  float energy_cost;        /* energy_cost_scale (allsteps_env_cfg.py:222) */
  float step_radius;        /* allsteps_env_cfg.py:97 */
  float step_reward;        /* 50 (allsteps_env.py:380) */
  float step_sigma;         /* 0.25 */
  float target_bonus;       /* 10 (allsteps_env.py:383) */
  float bonus_radius;       /* 0.15 */
  float foot_progress;      /* weight of the feet's distances in the potential */
  float foot_offset_y[4];   /* aim point lateral offset per sensor foot (RF, LF, RH, LH) */
} as_quad_task_t;

typedef struct as_env as_env_t;

/* Create a handle for `num_envs` envs on HIP device `device`.  `env_id_offset` is this shard's
 * first global env id (Philox stream = (seed, env_id_offset + e, episode)), so a sharded run is
 * bit-identical to an unsharded one.  The state pointers are stored, not copied.  The model's
 * 6 + num_hinges must have a compiled step kernel: 27 (the Allsteps walker, as_step / as_task_step /
 * as_physics_step) or 18 (the BASELINE C5 quadruped, as_physics_step); otherwise AS_ERR_INVALID. */
int as_create(int32_t num_envs, const as_model_t* model_host, const as_sim_t* sim_host,
              const as_task_t* task_host, const as_state_t* state, uint64_t seed, int32_t device,
              int64_t env_id_offset, as_env_t** out);
int as_destroy(as_env_t* env);

/* DirectRLEnv.reset (direct_rl_env.py:256-294): _reset_idx(all) -> FK -> observations. */
int as_reset_all(as_env_t* env, float* obs, const float* reset_draws, void* stream);

/* AllstepsEnv._reset_idx(env_ids) (allsteps_env.py:469-567, direct_rl_env.py:563-584) on the envs
 * with mask[e] != 0 (device, [n] uint8), then _get_observations for all envs into obs [n][59].
 * Like the reference's _reset_idx it applies the curriculum gate (mean target index over all envs)
 * and the second foot-state tick to every env; an all-zero mask changes nothing (the reference
 * never calls _reset_idx with no ids).  reset_draws as in as_step. */
int as_reset_mask(as_env_t* env, const uint8_t* mask, float* obs, const float* reset_draws, void* stream);

/* DirectRLEnv.step (direct_rl_env.py:296-383) for all envs: actions [n][21] (any range, clamped
 * to [-1,1] inside) -> obs [n][59], reward [n], terminated [n], truncated [n] (uint8 0/1).
 * reset_draws: NULL (Philox) or [n][22] U[0,1) draws (mirror, 21 joint-noise) for envs that reset
 * this step -- the reference's torch.rand(K) / rand(K,21) (allsteps_env.py:518,542). */
int as_step(as_env_t* env, const float* actions, float* obs, float* reward, uint8_t* terminated,
            uint8_t* truncated, const float* reset_draws, void* stream);

/* Task logic only (the post-physics half of as_step): body_pos / contact_mask are taken from the
 * state as the caller wrote them -- the operator a task-logic golden replay drives. */
int as_task_step(as_env_t* env, const float* actions, float* obs, float* reward, uint8_t* terminated,
                 uint8_t* truncated, const float* reset_draws, void* stream);

/* Re-seed the Philox reset-draw stream (DirectRLEnv.seed / reset(seed=...)). */
int as_set_seed(as_env_t* env, uint64_t seed);

/* Physics only (decimation substeps, no task logic): for known-answer tests and profiling. */
int as_physics_step(as_env_t* env, const float* actions, void* stream);

/* Select the actuation of the physics step (AS_ACT_TORQUE / AS_ACT_DC_MOTOR, see as_actuator_t).
 * as_set_actuator and as_set_quad_task are setup calls: they synchronize the device (every queued
 * launch on every stream finishes first) and then rewrite the handle's constants block.  Not graph-
 * safe: a captured graph keeps reading the block and sees the new values on its next replay. */
int as_set_actuator(as_env_t* env, const as_actuator_t* act_host);
/* BASELINE C5: the quadruped stepping-stone task (as_quad_task_t).  as_quad_step = physics substeps
 * (with the handle's actuator) + the task epilogue of every env, reset of done envs and the
 * observation [n][AS_QUAD_OBS_DIM]; as_quad_reset_all resets every env.  Needs a model whose sensor
 * feet 0..3 are the four feet and state->contact_mask_hind != NULL. */
int as_set_quad_task(as_env_t* env, const as_quad_task_t* task_host);
int as_quad_step(as_env_t* env, const float* actions, float* obs, float* reward, uint8_t* terminated,
                 uint8_t* truncated, void* stream);
int as_quad_reset_all(as_env_t* env, float* obs, void* stream);
/* AnymalCEnv._reset_idx(env_ids): as_quad_reset_all's reset for the envs with mask[e] != 0 (mask: [n] uint8,
 * device) -- stand pose + the env's next Philox joint-noise draw, episode + 1, targets, potentials, ep_len,
 * contact masks and contact-report counts cleared -- in one launch without physics, host synchronisation or
 * atomics; the mask is read on `stream`, so the call can be captured and the mask rewritten between replays.
 * Of obs [n][AS_QUAD_OBS_DIM] only the masked envs' rows are written (action columns zero); an env with
 * mask[e] == 0 keeps its state, masks, report and obs row untouched.  Null arguments, or a call before
 * as_set_quad_task: AS_ERR_INVALID. */
int as_quad_reset_mask(as_env_t* env, const uint8_t* mask, float* obs, void* stream);

/* _generate_foot_steps_allsteps (allsteps_env.py:125-174) on the device at curriculum `level`;
 * draws: [5][n][20] U[0,1) (NULL = Philox stream (seed, env, 0xF007)). Writes state->stones. */
int as_generate_stones(as_env_t* env, int32_t level, const float* draws, void* stream);

/* Ring-2 views, off the hot path (round 6).  The reference's ArticulationData body views
 * (articulation_data.py:430-447 body_state_w -- link-frame pose, COM velocity -- and body_link_state_w --
 * link-frame pose and velocity; body_pos_w = body_state_w[..., :3]) for EVERY body of the model (the
 * walker's 17 MJCF bodies), computed on demand from the SoA state as it stands: root pose / velocity
 * (root_lin is the root COM's velocity, as in the state), q, qd.  FK with the step kernel's own
 * arithmetic, so rows of bodies whose frame is the torso / a foot link equal state->body_pos bit for bit;
 * then per body b, with L = link[b]:
 *   pos  = root_pos + p_L + R_L offset_pos[b]             rot = R_L R(offset_quat[b])  (quat w, x, y, z)
 *   w    = root angular velocity + sum over the hinges j on the path of L of axis_j(world) * qd_j
 *   vfrm = velocity of the body frame's origin             vcom = velocity of the body's own COM (com[b])
 * out: device [AS_BODY_STATE_ROWS][num_bodies][n] fp32 = pos 3 | quat 4 | vfrm 3 | w 3 | vcom 3.
 * as_step never runs it; the caller launches it when a view is read (envs/allsteps_env.py). */
#define AS_MAX_BODIES 32
#define AS_BODY_STATE_ROWS 16
typedef struct {
  int32_t num_bodies;
  int32_t link[AS_MAX_BODIES];          /* the link whose frame carries the body (model body_link) */
  float offset_pos[AS_MAX_BODIES][3];   /* body frame in that link's frame */
  float offset_quat[AS_MAX_BODIES][4];  /* (w, x, y, z) */
  float com[AS_MAX_BODIES][3];          /* the body's own centre of mass, body frame */
} as_body_table_t;
int as_body_state(as_env_t* env, const as_body_table_t* bodies_host, float* out, void* stream);

/* The contact report (ABI 6), off by default: what the reference's ContactSensor reads beyond the flags
 * (contact_sensor.py:329-343 net_forces_w / force_matrix_w, history_length = 4: allsteps_env_cfg.py:119-130)
 * and ArticulationData.joint_acc (articulation_data.py:547-556).  With a report set, every launch with
 * physics (as_step, as_physics_step, as_quad_step) stores for each of its last `depth` substeps the
 * contacts the solver kept -- those the row budget cut are not in it -- in caller-owned device buffers,
 * field-major / env-minor and indexed by env id; substep slot 0 is the launch's last substep:
 *   count   [depth][n]                                     kept contacts
 *   records [depth][AS_REPORT_WORDS][AS_MAX_CONTACTS][n]   per contact slot c < count (zeros past it):
 *             words 0..2  lambda_n * n: the normal impulse (N s, world frame) on the robot link `link`, the
 *                         very floats the contact flags sum; 0 where the normal row was not solved
 *             words 3..5  the contact point, relative to the root link's origin, world axes
 *             word  6     the separation (m, < 0: penetration)
 *             word  7     link | (link2 + 1) << 8 | (stone + 1) << 16 | (foot + 1) << 24, with link2 the
 *                         second robot link of a self-contact, stone the stone of a stone contact and foot
 *                         the geom's contact sensor, each -1 when there is none
 *   qd_prev [AS_ACT_DIM][n]   joint velocities (cfg dof order) at the start of the launch's last substep:
 *                             joint_acc = (qd - qd_prev) / dt
 * Launches without physics (as_reset_*, as_task_step) leave the report as it is, and an env that as_step
 * resets keeps its last substep's records exactly as it keeps its contact_mask; as_quad_step / as_quad_reset_all /
 * as_quad_reset_mask, which clear a reset env's masks, clear its counts.
 * as_set_contact_report is a setup call like as_debug_stamps (not during graph capture): the pointers are
 * stored and every later launch writes through them, a replayed graph included.  1 <= depth <=
 * sim.substeps, else AS_ERR_INVALID; report == NULL switches the report off. */
#define AS_REPORT_WORDS 8
#define AS_REPORT_FEET 4   /* contact sensors 0..3 (as_model_t geom_foot) */
typedef struct {
  int32_t depth;
  int32_t* count;
  uint32_t* records;
  float* qd_prev;
} as_contact_report_t;
int as_set_contact_report(as_env_t* env, const as_contact_report_t* report);
/* Dense, zero-filled sums over the report as it stands (one launch of k_contact_forces on `stream`, never
 * part of as_step; no float atomics: every entry is one thread's sum over the env's records in ascending
 * slot order, from +0 with plain adds -- the contact flags' arithmetic):
 *   force_matrix_out [depth][AS_REPORT_FEET][AS_NUM_STONES][3][n]  impulse of stone s on sensor foot f
 *   net_out          [depth][num_bodies][3][n]  net contact impulse on each body of `bodies_host`: + the
 *                    records whose link is the body's link, - those whose link2 is (a self-contact's second
 *                    body takes the opposite impulse; a stone contact counts for its robot body only)
 * Divide by sim.dt for forces.  AS_ERR_INVALID when no report is set or an argument is NULL. */
int as_contact_forces(as_env_t* env, const as_body_table_t* bodies_host, float* force_matrix_out, float* net_out,
                      void* stream);
/* The air / contact timers of the reference's ContactSensor with track_air_time = True (contact_sensor.py:351-379,
 * 156-161; compute_first_contact / compute_first_air read them), off by default: one launch of k_contact_timers
 * on `stream` over the report as it stands, never part of as_step -- the caller launches it after as_step
 * (envs/direct_rl_env.py), so only steps made that way drive the timers, not bare as_physics_step calls.  One
 * added symbol, no struct change: AS_ABI_VERSION stays 6.
 *   timers    [4][num_bodies][n]  rows current_air, last_air, current_contact, last_contact (s), caller-owned,
 *                                 zeroed at construction and kept with the state
 *   timestamp [n]                 the sensor's float32 time since the env's last reset
 * updates = the report's depth: every env applies `depth` sensor updates, oldest substep (slot depth - 1) first:
 * timestamp += sim.dt; elapsed = the float32 difference of the two timestamps; a body is in contact where the
 * norm of its net impulse (as_contact_forces' net_out: report_body_sum over its link, self-contacts with their
 * sign) / sim.dt exceeds force_threshold; then the reference's four lines in its order
 * (csrc/allsteps_contact_timers.h has the formulas and the float32 rounding order).  updates = 0: no update.
 * Afterwards the envs with reset[e] | reset2[e] != 0 ([n] uint8 each; reset2 may be NULL) get zero timers and a
 * zero timestamp; reset NULL: every env when updates = 0 (reset() and _reset_idx(None)), none otherwise.
 * AS_ERR_INVALID when no report is set, updates is neither 0 nor the report's depth, reset2 comes without reset
 * or timers / timestamp / bodies_host is NULL.  Graph-safe: nothing per call comes from the host but the pointers
 * and the two scalars. */
int as_contact_timers(as_env_t* env, const as_body_table_t* bodies_host, float* timers, float* timestamp,
                      float force_threshold, int32_t updates, const uint8_t* reset, const uint8_t* reset2,
                      void* stream);

/* The reference's RayCaster sensor (ray_caster.py:201-260; a height scanner with a grid pattern) over the ground
 * plane and the env's stones, off by default: one launch of k_ray_cast on `stream` over the state as it stands,
 * never part of as_step.  One added symbol and one added struct: AS_ABI_VERSION stays 6.
 *   rays    [6][num_rays]        device memory: local start xyz | direction xyz of every ray, sensor frame
 *   hits    [3][num_rays][n]     the hit point, env-local frame; (+inf, +inf, +inf) for a miss
 *   surface int8 [num_rays][n]   the stone hit, AS_RAY_HIT_GROUND or AS_RAY_MISS; may be NULL
 *   pose    [7][n]               root_pos | root_quat as the kernel read them; may be NULL
 * The sensor frame is the root link's (root_pos, root_quat).  attach_yaw_only != 0: starts are rotated by the
 * yaw of root_quat only and directions are the local ones; else both are rotated by root_quat.  Directions are
 * not normalised: distances, max_distance included, are in units of |direction|.  surfaces selects the ground
 * plane z = ground_z (hit from above only) and / or the stones, closed boxes stones[3 s .. 3 s + 2] -+
 * sim.stone_half, s < task.num_steps; a ray from inside a box hits its far face.  The nearest hit with t <=
 * max_distance wins; on equal t the ground, then the lowest stone (csrc/allsteps_ray_caster.h has the formulas and
 * the float32 rounding order).  AS_ERR_INVALID, before any device call, for a NULL env / cfg / rays / hits,
 * num_rays outside [1, 1024 = AS_MAX_RAYS], surfaces 0 or with unknown bits, a max_distance that is not finite
 * or <= 0, a ground_z that is not finite.  Graph-safe: the rays are read from device memory at every launch. */
#define AS_RAY_GROUND 1
#define AS_RAY_STONES 2
#define AS_RAY_HIT_GROUND (-1)
#define AS_RAY_MISS (-2)
typedef struct {
  int32_t num_rays;
  int32_t attach_yaw_only;
  int32_t surfaces;     /* AS_RAY_GROUND | AS_RAY_STONES */
  float max_distance;
  float ground_z;
} as_ray_caster_t;
int as_ray_cast(as_env_t* env, const as_ray_caster_t* cfg_host, const float* rays, float* hits, int8_t* surface,
                float* pose, void* stream);

/* The reference's Imu sensor (imu.py:142-203) on any body of the model, off by default: one launch of k_imu on
 * `stream` over the state as it stands, never part of as_step.  One added symbol and one added struct:
 * AS_ABI_VERSION stays 6.  The launch runs as_body_state's FK, forms each sensor's body row (pose, COM velocities)
 * and updates the sensors of every outdated env (csrc/allsteps_imu.h has the formulas and the float32 rounding
 * order); S = num_sensors:
 *   outdated uint8 [n]    != 0: the env is recomputed and its flag cleared; all != 0 treats every env as set
 *   data     [19][S][n]   pos_w 3 | quat_w 4 (w, x, y, z) | lin_vel_b 3 | ang_vel_b 3 | lin_acc_b 3 | ang_acc_b 3
 *   prev     [6][S][n]    the world linear | angular velocity of the env's previous update (zero at first)
 * An env that is not outdated keeps its data and prev rows bit for bit.  Accelerations are (velocity - prev) / dt,
 * the linear one plus gravity_bias.  Per sensor: link / body_offset_* / com are the as_body_table_t row of the body
 * it sits on, offset_pos / offset_rot the sensor frame in that body's frame (offset_rot is used as given).
 * AS_ERR_INVALID, before any device call, for a NULL env / table / outdated / data / prev, num_sensors outside
 * [1, AS_MAX_IMUS], a link outside the model, a dt that is not finite or <= 0.  Graph-safe: dt, the table and `all`
 * are captured by value. */
#define AS_MAX_IMUS 8
typedef struct {
  int32_t num_sensors;
  int32_t link[AS_MAX_IMUS];              /* the link whose frame carries the sensor's body */
  float body_offset_pos[AS_MAX_IMUS][3];  /* the body frame in that link's frame (as_body_table_t.offset_pos) */
  float body_offset_quat[AS_MAX_IMUS][4]; /* (w, x, y, z) */
  float com[AS_MAX_IMUS][3];              /* the body's own centre of mass, body frame */
  float offset_pos[AS_MAX_IMUS][3];       /* the sensor frame in the body frame (ImuCfg.offset.pos) */
  float offset_rot[AS_MAX_IMUS][4];       /* (w, x, y, z), not normalised (ImuCfg.offset.rot) */
  float gravity_bias[AS_MAX_IMUS][3];     /* added to the world linear acceleration (ImuCfg.gravity_bias) */
} as_imu_table_t;
int as_imu(as_env_t* env, const as_imu_table_t* host, float dt, int all, uint8_t* outdated, float* data, float* prev,
           void* stream);

/* The reference's FrameTransformer sensor (frame_transformer.py:322-385) over the model's bodies and the env's
 * stones, off by default: one launch of k_frame_transformer on `stream` over the state as it stands, never part of
 * as_step.  One added symbol and two added structs: AS_ABI_VERSION stays 6.  The launch runs as_body_state's FK and
 * forms, for each of the F = num_frames target frames of the S = num_sensors sensors, the frame's pose in the world
 * and in its sensor's source frame (csrc/allsteps_frame_transformer.h has the formulas and the float32 rounding
 * order):
 *   source [7][S][n]    out: the source frame's pos 3 | quat 4 (w, x, y, z)
 *   target [14][F][n]   out: pos_w 3 | quat_w 4 | pos_source 3 | quat_source 4
 * A frame sits on a robot body (link >= 0: link / body_offset_* are the as_body_table_t row of the body; its link
 * pose is as_body_state rows 0:7) or on a stone (link < 0: position state.stones rows 3 stone .. 3 stone + 2,
 * quaternion (1, 0, 0, 0)), moved by offset_pos / offset_rot (offset_rot is used as given) where the sensor's switch
 * says so: apply_source_offset for the source, apply_target_offset for EVERY target frame of the sensor, identity
 * offsets included (the reference's two switches; a product with the identity quaternion is not a no-op in float32).
 * Frames are grouped by sensor: sensor[] starts at 0, never decreases, steps by at most 1 and ends at S - 1.
 * Positions are env-local.  The sensor keeps no state: the buffers are a function of the state as it stands.
 * AS_ERR_INVALID, before any device call, for a NULL env / table / source / target, num_sensors outside
 * [1, AS_MAX_FRAME_TRANSFORMERS], num_frames outside [1, AS_MAX_FRAMES], a link outside the model, a stone outside
 * [0, task.num_steps), a frame whose sensor is outside [0, S) or out of order.  Graph-safe: the table is captured
 * by value. */
#define AS_MAX_FRAME_TRANSFORMERS 4
#define AS_MAX_FRAMES 32
typedef struct {
  int32_t link;             /* >= 0: the link whose frame carries the body; < 0: the frame sits on a stone */
  int32_t stone;            /* the stone (link < 0) */
  float body_offset_pos[3]; /* the body frame in that link's frame (as_body_table_t.offset_pos) */
  float body_offset_quat[4];/* (w, x, y, z) */
  float offset_pos[3];      /* the frame in the body's (the stone's) frame (OffsetCfg.pos) */
  float offset_rot[4];      /* (w, x, y, z), not normalised (OffsetCfg.rot) */
} as_frame_body_t;
typedef struct {
  int32_t num_sensors;
  int32_t num_frames;
  int32_t apply_source_offset[AS_MAX_FRAME_TRANSFORMERS]; /* != 0: the source offset is applied */
  int32_t apply_target_offset[AS_MAX_FRAME_TRANSFORMERS]; /* != 0: every target offset of the sensor is applied */
  as_frame_body_t source[AS_MAX_FRAME_TRANSFORMERS];      /* per sensor: the source body and the source offset */
  as_frame_body_t target[AS_MAX_FRAMES];                  /* per frame: the target body and the frame's offset */
  int32_t sensor[AS_MAX_FRAMES];                          /* per frame: the sensor it belongs to */
} as_frame_table_t;
int as_frame_transformer(as_env_t* env, const as_frame_table_t* host, float* source, float* target, void* stream);

/* The reference's RayCasterCamera sensor (ray_caster_camera.py:257-318; a depth camera with a pinhole pattern) over
 * the ground plane and the env's stones, off by default: one launch of k_ray_camera on `stream` over the state as it
 * stands, never part of as_step.  One added symbol and one added struct: AS_ABI_VERSION stays 6.  R = width * height:
 *   dirs    [3][R]      device memory: the local direction of every pixel, row-major over the image (pixel (row v,
 *                       column u) is ray v * width + u), camera frame in the "world" convention (x forward, z up)
 *   offset  [7][n]      device memory: the camera frame in the root link's frame, position | quaternion (w, x, y, z)
 *                       in the "world" convention, used as given (not normalised)
 *   pose    [7][n]      out: the camera's pos_w | quat_w_world
 *   plane   [n][R]      out, may be NULL: distance_to_image_plane, the hit's x coordinate in the camera frame
 *   camera  [n][R]      out, may be NULL: distance_to_camera, the distance along the ray in units of |direction|
 *   normals [n][R][3]   out, may be NULL: the outward unit normal of the face hit
 * The images are env-major and contiguous: (n, height, width, 1 | 3).  Every ray starts at the camera's position.
 * surfaces selects what is cast against, as in as_ray_cast, with the same tie rules; the cast's own distance cap is
 * 1e6.  A miss: camera = +inf, plane = NaN (inf times the direction, rotated), normals = +inf.  clipping then maps
 * values above max_distance -- and, in plane, NaN -- to max_distance (AS_CAM_CLIP_MAX) or 0 (AS_CAM_CLIP_ZERO);
 * normals are never clipped (csrc/allsteps_ray_camera.h has the formulas and the float32 rounding order).
 * AS_ERR_INVALID, before any device call, for a NULL env / cfg / dirs / offset / pose, all three images NULL, a
 * non-positive width or height or width * height above AS_MAX_CAMERA_RAYS, surfaces 0 or with unknown bits, an
 * unknown clipping, a max_distance that is not finite or <= 0, a ground_z that is not finite.  Graph-safe: dirs and
 * offset are read from device memory at every launch. */
#define AS_MAX_CAMERA_RAYS 16384 /* 128 x 128 */
#define AS_CAM_CLIP_NONE 0
#define AS_CAM_CLIP_MAX 1
#define AS_CAM_CLIP_ZERO 2
typedef struct {
  int32_t width;
  int32_t height;
  int32_t surfaces;     /* AS_RAY_GROUND | AS_RAY_STONES */
  int32_t clipping;     /* AS_CAM_CLIP_* */
  float max_distance;
  float ground_z;
} as_ray_camera_t;
int as_ray_camera(as_env_t* env, const as_ray_camera_t* cfg_host, const float* dirs, const float* offset,
                  float* pose, float* plane, float* camera, float* normals, void* stream);

/* Noise models, off by default: DirectRLEnv.step's cfg.action_noise_model / cfg.observation_noise_model
 * (direct_rl_env.py:322-323, 379-380, 578-581; isaaclab/utils/noise/noise_model.py).  Stateless entry points
 * over caller-owned device buffers -- no as_env_t: the env step itself is unchanged, the caller launches
 * as_noise_actions before it and as_noise_post after it on the same stream (envs/direct_rl_env.py).  A model
 * is a term (kind, op, two parameter vectors [cols]) and an optional per-env additive bias re-drawn from a
 * second, scalar term for the envs that reset (NoiseModelWithAdditiveBias).  Parameters p0 / p1: the bias
 * / unused (constant), n_min / n_max - n_min (uniform), mean / std (gaussian).  Formulas, Philox stream
 * layout (seed, env_id_offset + e, t[e], column quad, tag) and the float32 rounding order that reproduces
 * torch's bits from the same draws: csrc/allsteps_noise.h.  t [n] is the per-env step counter of the stream,
 * advanced by as_noise_post only; zero it at construction and keep it with the state.  Both calls are
 * graph-safe: nothing per call comes from the host but the pointers. */
enum { AS_NOISE_NONE = 0, AS_NOISE_CONSTANT = 1, AS_NOISE_UNIFORM = 2, AS_NOISE_GAUSSIAN = 3 };
enum { AS_NOISE_ADD = 0, AS_NOISE_SCALE = 1, AS_NOISE_ABS = 2 };
typedef struct {
  int32_t kind, op;           /* the term: AS_NOISE_CONSTANT / UNIFORM / GAUSSIAN, AS_NOISE_ADD / SCALE / ABS */
  const float* p0;            /* [cols] */
  const float* p1;            /* [cols] (not read by the constant term: may be NULL) */
  int32_t bias_kind, bias_op; /* the bias term, AS_NOISE_NONE: a plain NoiseModel without a bias */
  float bias_p0, bias_p1;
  float* bias;                /* [n] the per-env bias (bias_kind != AS_NOISE_NONE) */
} as_noise_model_t;
/* out [n][cols] = model(in [n][cols]), out of place (in is never written; out != in).  draws: NULL (Philox,
 * the action-term stream at t[e]) or [n][cols] injected draws -- uniforms in [0, 1) or unit normals as the
 * kind needs.  1 <= cols <= 256. */
int as_noise_actions(const as_noise_model_t* model, const float* in, float* out, int32_t n, int32_t cols,
                     const uint32_t* t, const float* draws, uint64_t seed, int64_t env_id_offset, void* stream);
/* After the step, in one launch: for the envs with reset[e] | reset2[e] != 0 ([n] uint8 each; reset2 may be
 * NULL; reset NULL: every env) re-draw the bias of action_model and of obs_model (either may be NULL or have
 * no bias); then obs [n][cols] = obs_model(obs) in place with the biases as they now stand; then t[e] += 1.
 * obs NULL (cols ignored) serves reset() and _reset_idx: bias re-draw and counter only.  obs_draws [n][cols],
 * action_bias_draws [n], obs_bias_draws [n]: injected draws or NULL (Philox streams at t[e]). */
int as_noise_post(const as_noise_model_t* action_model, const as_noise_model_t* obs_model, float* obs, int32_t n,
                  int32_t cols, uint32_t* t, const uint8_t* reset, const uint8_t* reset2, const float* obs_draws,
                  const float* action_bias_draws, const float* obs_bias_draws, uint64_t seed,
                  int64_t env_id_offset, void* stream);

/* Interval events, off by default: the "interval" terms of cfg.events that DirectRLEnv.step applies after
 * _reset_idx and before _get_observations (direct_rl_env.py:370-372; EventManager.apply,
 * isaaclab/managers/event_manager.py:200-225).  One term is served: push_by_setting_velocity
 * (isaaclab/envs/mdp/events.py:681-706), which adds a uniform sample to the root velocity.  Stateless entry
 * points over caller-owned device buffers, as the noise models' -- no as_env_t: the caller launches
 * as_events_interval after as_step on the same stream (envs/direct_rl_env.py).  In the reference the push
 * does not reach the observation, reward or dones of the step in which it fires (they are made from values
 * cached before it); the next step's physics sees it first, which is what a launch after as_step gives.
 * Every buffer is field-major / env-minor: root_lin [3][n] and root_ang [3][n] (as_state_t's), time_left
 * [num_terms][n], t [n] (the per-env counter of the event streams), fired [num_terms][n].  Semantics, the
 * float32 rounding order and the Philox stream layout (seed, env_id_offset + e, t[e], term block, tag):
 * csrc/allsteps_events.h.  Both calls are graph-safe: nothing per call comes from the host but the pointers
 * and the fixed dt; the term descriptors are read from device memory at every launch. */
#define AS_MAX_EVENT_TERMS 4
typedef struct {
  float interval_lo, interval_w; /* interval_range_s: lo and float32(double(hi) - double(lo)) */
  float vel_lo[6], vel_w[6];     /* velocity_range x y z roll pitch yaw: float32(lo), float32(hi) - float32(lo) */
} as_event_term_t;
/* The initial timers: time_left[k][e] = u w + lo from the interval stream's draw at counter 0 (or from
 * interval_draws [num_terms][n], NULL: Philox), then t[e] = 1.  terms: num_terms descriptors in device memory. */
int as_events_init(const as_event_term_t* terms, int32_t num_terms, float* time_left, uint32_t* t, int32_t n,
                   const float* interval_draws, uint64_t seed, int64_t env_id_offset, void* stream);
/* One env step of every term in one launch, terms in order: time_left -= dt; where time_left < 1e-6 the term
 * fires: time_left is resampled and the push added to (root_lin, root_ang).  Then t[e] += 1.  fired: NULL or
 * [num_terms][n] uint8, written 0 / 1 for every (term, env).  interval_draws [num_terms][n], push_draws
 * [num_terms][6][n]: injected uniforms in [0, 1), read only where a term fires, or NULL (Philox streams at
 * t[e]).  1 <= num_terms <= AS_MAX_EVENT_TERMS. */
int as_events_interval(const as_event_term_t* terms, int32_t num_terms, float* root_lin, float* root_ang,
                       float* time_left, uint32_t* t, uint8_t* fired, int32_t n, float dt,
                       const float* interval_draws, const float* push_draws, uint64_t seed, int64_t env_id_offset,
                       void* stream);

/* Command manager, off by default: the velocity command terms of cfg.commands (isaaclab/managers/
 * command_manager.py; UniformVelocityCommand / NormalVelocityCommand, isaaclab/envs/mdp/commands/
 * velocity_command.py).  The reference's step resets the envs that are done, then calls
 * command_manager.compute(step_dt), then applies the interval events (manager_based_rl_env.py:220-239): the caller
 * launches as_commands_step after as_step and before as_events_interval on the same stream.  Stateless entry
 * points over caller-owned device buffers, as the events' -- no as_env_t.  Every buffer is field-major /
 * env-minor: root_quat [4][n] (w x y z), root_lin [3][n], root_ang [3][n] (as_state_t's, read only), vel
 * [num_terms][3][n], heading_target [num_terms][n], flags [num_terms][5][n] uint8 (is_heading, is_standing,
 * is_zero_vel_x / y / yaw), time_left [num_terms][n], counter [num_terms][n] int32, metrics and last_metrics
 * [num_terms][2][n] (error_vel_xy, error_vel_yaw), t [n] (the per-env counter of the command streams).
 * Semantics, the float32 rounding order and the Philox stream layout (seed, env_id_offset + e, t[e], term block,
 * phase tag): csrc/allsteps_commands.h.  Both calls are graph-safe: nothing per call comes from the host but the
 * pointers and the fixed dt; the term descriptors are read from device memory at every launch.  The host forms
 * every constant of a descriptor (envs/commands.py). */
#define AS_MAX_COMMAND_TERMS 4
#define AS_COMMAND_DRAWS 11 /* draws a term consumes per resample at most (csrc/allsteps_commands.h) */
enum { AS_COMMAND_UNIFORM = 0, AS_COMMAND_NORMAL = 1 };
typedef struct {
  int32_t kind;             /* AS_COMMAND_UNIFORM / AS_COMMAND_NORMAL */
  int32_t heading;          /* heading_command (uniform term only) */
  float time_lo, time_w;    /* resampling_time_range: float32(lo), float32(hi) - float32(lo) */
  float lo[4], w[4];        /* uniform: lin_vel_x, lin_vel_y, ang_vel_z, heading as float32(lo), float32(hi) -
                               float32(lo); normal: mean_vel in lo[0..2], std_vel in w[0..2] */
  float clip_lo, clip_hi;   /* ang_vel_z as float32: the heading controller's clip */
  float stiffness;          /* heading_control_stiffness */
  float p_heading;          /* rel_heading_envs */
  float p_standing;         /* rel_standing_envs */
  float p_zero[3];          /* zero_prob (normal term) */
  float max_command_step;   /* float32(resampling_time_range[1] / step_dt), the division in double */
} as_command_term_t;
/* One env step of every term in one launch, terms in order.  For an env with reset[e] | reset2[e] != 0 ([n] uint8
 * each, either may be NULL: no env): CommandTerm.reset -- last_metrics = metrics, metrics = 0, counter = 0,
 * resample.  Then for every env CommandTerm.compute(dt): metrics, time_left -= dt, resample where time_left <= 0,
 * the command's update.  Then t[e] += 1.  draws: NULL (Philox) or [2][num_terms][AS_COMMAND_DRAWS][n] injected
 * draws, phase 0 the reset's and phase 1 the compute's, read only where a term resamples -- uniforms in [0, 1),
 * and unit normals in rows 1..3 of a normal term.  last_metrics may be NULL: not written.
 * 1 <= num_terms <= AS_MAX_COMMAND_TERMS. */
int as_commands_step(const as_command_term_t* terms, int32_t num_terms, const float* root_quat,
                     const float* root_lin, const float* root_ang, float* vel, float* heading_target,
                     uint8_t* flags, float* time_left, int32_t* counter, float* metrics, float* last_metrics,
                     uint32_t* t, const uint8_t* reset, const uint8_t* reset2, int32_t n, float dt,
                     const float* draws, uint64_t seed, int64_t env_id_offset, void* stream);
/* CommandTerm.reset alone, no compute (ManagerBasedRLEnv.reset, command_manager.reset(env_ids)): for the envs
 * with mask[e] != 0 ([n] uint8; NULL: every env), then t[e] += 1 for every env.  draws: NULL or
 * [num_terms][AS_COMMAND_DRAWS][n]. */
int as_commands_reset(const as_command_term_t* terms, int32_t num_terms, float* vel, float* heading_target,
                      uint8_t* flags, float* time_left, int32_t* counter, float* metrics, float* last_metrics,
                      uint32_t* t, const uint8_t* mask, int32_t n, const float* draws, uint64_t seed,
                      int64_t env_id_offset, void* stream);

/* Observation manager, off by default: the term groups of cfg.observations (isaaclab/managers/
 * observation_manager.py, the term functions of isaaclab/envs/mdp/observations.py).  One launch assembles one
 * group: per term the value from the env's device state, then noise, clip, scale and the history, written into the
 * row-major out [n][out_cols] -- the terms side by side, each as `history` slots of `width` columns, oldest first.
 * The caller launches it last in a step, after as_step, as_commands_step and as_events_interval, on the same stream
 * (manager_based_rl_env.py step).  Stateless entry points over caller-owned device buffers -- no as_env_t.  The
 * sources are field-major / env-minor ([rows][n]) except the actions ([n][action_cols]).  Formulas, rounding order,
 * history rule and the Philox stream layout: csrc/allsteps_observations.h.  Both calls are graph-safe: the term
 * descriptors, the column table and the output map are read from device memory at every launch. */
#define AS_MAX_OBS_GROUPS 4
#define AS_MAX_OBS_TERMS 16       /* terms of a group */
#define AS_MAX_OBS_COLS 256       /* columns of a group before the history */
#define AS_MAX_OBS_OUT_COLS 1280  /* columns of a group's output, history included */
#define AS_OBS_COL_ROWS 6         /* column table rows: source row (int32) | a | b | noise p0 | noise p1 | scale */
enum {
  AS_OBS_GATHER = 0,         /* src[row] - a                          (a = 0, or the joint default) */
  AS_OBS_LIMIT_NORM = 1,     /* 2 (src[row] - a) / b                  scale_transform: a the centre, b the range */
  AS_OBS_QUAT_UNIQUE = 2,    /* src[row], negated where the quaternion's w < 0 */
  AS_OBS_ROTATE_INVERSE = 3, /* quat_rotate_inverse(root_quat, src rows) -- src AS_OBS_SRC_GRAVITY: (0, 0, -1) */
  AS_OBS_HEIGHT_SCAN = 4,    /* (ray_pose[2] - ray_hits[row]) - a     a the offset */
  AS_OBS_LAST_ACTION = 5     /* actions[e][row], 0 for an env the step reset; flags & 1: clamped to [-1, 1] */
};
enum {
  AS_OBS_SRC_ROOT_POS = 0, AS_OBS_SRC_ROOT_QUAT, AS_OBS_SRC_ROOT_LIN, AS_OBS_SRC_ROOT_ANG, AS_OBS_SRC_Q,
  AS_OBS_SRC_QD, AS_OBS_SRC_COMMANDS, AS_OBS_SRC_IMU, AS_OBS_SRC_RAY_HITS, AS_OBS_SRC_RAY_POSE, AS_OBS_SRC_ACTIONS,
  AS_OBS_SRC_GRAVITY, AS_OBS_NUM_SOURCES
};
typedef struct {
  int32_t kind;               /* AS_OBS_* */
  int32_t source;             /* AS_OBS_SRC_* */
  int32_t width;              /* columns of the term before the history */
  int32_t col;                /* its first column among the group's pre-history columns */
  int32_t out_col;            /* its first column in the output */
  int32_t history;            /* slots, >= 1 (history_length 0 and 1 are both one slot) */
  int32_t noise_kind;         /* AS_NOISE_NONE / CONSTANT / UNIFORM / GAUSSIAN; parameters in the column table */
  int32_t noise_op;           /* AS_NOISE_ADD / SCALE / ABS */
  int32_t clip;               /* != 0: clip to [clip_lo, clip_hi] as torch's clip_ (a NaN stays a NaN) */
  float clip_lo, clip_hi;
  int32_t flags;              /* bit 0: AS_OBS_LAST_ACTION clamps to [-1, 1] (an env whose `actions` clamps) */
} as_observation_term_t;
typedef struct {
  const float* ptr[AS_OBS_NUM_SOURCES]; /* device rows of each source, NULL: not there (reads as 0) */
  int32_t rows[AS_OBS_NUM_SOURCES];     /* rows of each source ([rows][n]; the actions: action columns) */
} as_observation_sources_t;
/* One group, one launch.  terms [num_terms], cols [AS_OBS_COL_ROWS][AS_MAX_OBS_COLS] 32-bit words and omap
 * [out_cols] int32 (pre-history column | last slot << 8 | term width << 9) are device memory.  An env with reset[e]
 * | reset2[e] != 0 ([n] uint8 each, either may be NULL) has its push count set to 0 first and its last action read
 * as 0; an env at push count 0 fills every slot with the new value (CircularBuffer.append).  Then count[e] += 1 and
 * t[e] += 1.  draws: NULL (Philox at (seed, env_id_offset + e, t[e], group * 64 + column / 4, tag)) or [d0][n]
 * injected draws (uniforms in [0, 1) or unit normals as the term's noise takes them). */
int as_observations_step(const as_observation_term_t* terms, int32_t num_terms, const float* cols,
                         const int32_t* omap, int32_t d0, int32_t out_cols, int32_t group,
                         const as_observation_sources_t* sources, float* out, int32_t* count, uint32_t* t,
                         const uint8_t* reset, const uint8_t* reset2, int32_t n, const float* draws, uint64_t seed,
                         int64_t env_id_offset, void* stream);
/* ObservationManager.reset(env_ids) of one group: for the envs with mask[e] != 0 ([n] uint8; NULL: every env) the
 * push count becomes 0 and the output row 0 (CircularBuffer.reset).  Nothing is computed, t is not advanced. */
int as_observations_reset(float* out, int32_t out_cols, int32_t* count, const uint8_t* mask, int32_t n,
                          void* stream);

/* Reward manager, off by default: the weighted term sums of cfg.rewards (isaaclab/managers/reward_manager.py, the
 * term functions of isaaclab/envs/mdp/rewards.py and of the velocity task's mdp/rewards.py).  One launch computes
 * every term of every env: per term in cfg order value = (f weight) dt, reward += value, episode_sums[k] += value,
 * step_reward[k] = value / dt; a term whose weight is exactly 0 is skipped (f is not evaluated, its rows keep their
 * values).  Then, for an env with reset[e] | reset2[e] != 0: last_episode_sums = episode_sums, episode_sums = 0,
 * prev_actions = 0; for every other env prev_actions = actions.  The caller launches it after as_step (and the
 * contact forces, timers and commands its terms read) on the same stream; the state rows of an env the step reset
 * are the post-reset ones.  Stateless entry points over caller-owned device buffers -- no as_env_t.  Every buffer is
 * field-major / env-minor ([rows][n]) except actions and prev_actions ([n][action_cols]).  Formulas and the float32
 * rounding order: csrc/allsteps_rewards.h.  Both calls are graph-safe: the term descriptors and the index table are
 * read from device memory at every launch.  Symbols added only: AS_ABI_VERSION stays 6. */
#define AS_MAX_REW_TERMS 32
#define AS_MAX_REW_IDS 32   /* entries of a term's row of the index table (joints or bodies) */
#define AS_REW_TABLE_ROWS 3 /* table [3][AS_MAX_REW_TERMS][AS_MAX_REW_IDS] words: id (int32) | a | b */
enum {
  AS_REW_IS_ALIVE = 0,          /* 1 - terminated */
  AS_REW_IS_TERMINATED,         /* terminated */
  AS_REW_LIN_VEL_Z_L2,          /* root_lin_vel_b[2]^2 */
  AS_REW_ANG_VEL_XY_L2,         /* root_ang_vel_b[0]^2 + [1]^2 */
  AS_REW_FLAT_ORIENTATION_L2,   /* projected_gravity_b[0]^2 + [1]^2 */
  AS_REW_BASE_HEIGHT_L2,        /* (root_pos[2] - p0)^2                          p0 target_height */
  AS_REW_JOINT_VEL_L1,          /* sum |qd[id]| */
  AS_REW_JOINT_VEL_L2,          /* sum qd[id]^2 */
  AS_REW_JOINT_DEVIATION_L1,    /* sum |q[id] - a|                               a the default pose */
  AS_REW_JOINT_POS_LIMITS,      /* sum -min(q[id] - a, 0) + max(q[id] - b, 0)    a, b the soft limits */
  AS_REW_JOINT_ACC_L2,          /* sum ((qd[id] - qd_prev[id]) / sim_dt)^2 */
  AS_REW_ACTION_L2,             /* sum action^2 */
  AS_REW_ACTION_RATE_L2,        /* sum (action - prev_action)^2 */
  AS_REW_UNDESIRED_CONTACTS,    /* count of bodies whose max-over-slots |net / sim_dt| > p0 */
  AS_REW_CONTACT_FORCES,        /* sum max(that maximum - p0, 0) */
  AS_REW_FEET_AIR_TIME,         /* sum (last_air - p0) first_contact, gated; p1 = float32(step_dt + 1e-8) */
  AS_REW_FEET_AIR_TIME_BIPED,   /* feet_air_time_positive_biped, threshold p0, gated */
  AS_REW_TRACK_LIN_VEL_XY_EXP,  /* exp(-|cmd_xy - root_lin_vel_b_xy|^2 / p0)     p0 = float32(std^2) */
  AS_REW_TRACK_ANG_VEL_Z_EXP,   /* exp(-(cmd_yaw - root_ang_vel_b[2])^2 / p0) */
  AS_REW_TRACK_ANG_VEL_Z_WORLD_EXP, /* exp(-(cmd_yaw - root_ang[2])^2 / p0) */
  AS_REW_TRACK_LIN_VEL_XY_YAW_EXP,  /* exp(-|cmd_xy - quat_rotate_inverse(yaw_quat(root_quat), root_lin)_xy|^2 / p0) */
  AS_REW_NUM_KINDS
};
typedef struct {
  int32_t kind;     /* AS_REW_* */
  float weight;     /* float32(cfg weight); exactly 0: the term is skipped */
  int32_t num_ids;  /* entries of the term's index-table row, <= AS_MAX_REW_IDS */
  int32_t cmd_row;  /* first row of the term's command in `commands` (3 x the command term's index) */
  float p0, p1;     /* the kind's constants, formed by the host as float32 the way torch takes a Python scalar */
  int32_t reserved0, reserved1;
} as_reward_term_t;
typedef struct {
  const float* root_pos;      /* [3][n] */
  const float* root_quat;     /* [4][n] (w x y z) */
  const float* root_lin;      /* [3][n] */
  const float* root_ang;      /* [3][n] */
  const float* q;             /* [joint_rows][n] */
  const float* qd;            /* [joint_rows][n] */
  const float* qd_prev;       /* [qd_prev_rows][n] the contact report's, or NULL */
  const float* commands;      /* [command_rows][n] the command manager's vel rows, or NULL */
  const float* net;           /* [depth][bodies][3][n] as_contact_forces' net impulses, or NULL */
  const float* timers;        /* [4][timer_bodies][n] as_contact_timers' rows, or NULL */
  const float* actions;       /* [n][action_cols], or NULL */
  const uint8_t* terminated;  /* [n] the step's terminated flags, or NULL (reads as 0) */
  int32_t joint_rows, qd_prev_rows, command_rows, depth, bodies, timer_bodies, action_cols;
  int32_t clamp_actions;      /* != 0: an action is read clamped to [-1, 1] (an env whose `actions` clamps) */
  float sim_dt;               /* the physics step: impulses / sim_dt are forces, (qd - qd_prev) / sim_dt joint_acc */
} as_reward_sources_t;
/* terms [num_terms] and table [AS_REW_TABLE_ROWS][AS_MAX_REW_TERMS][AS_MAX_REW_IDS] are device memory.  kinds: bit k
 * set for every AS_REW_* kind a descriptor may hold (the host's knowledge of the device descriptors): a set bit whose
 * source pointer is NULL is AS_ERR_INVALID, as are NULL terms / table / sources / reward / episode_sums /
 * step_reward, num_terms outside [1, AS_MAX_REW_TERMS], a dt that is not finite or <= 0, prev_actions without
 * actions -- all before any device call.  A source that is NULL, or an id outside its rows, reads as 0 on the
 * device.  reward [n], episode_sums, step_reward and last_episode_sums [num_terms][n]; prev_actions
 * [n][action_cols].  last_episode_sums and prev_actions may be NULL (not written) unless an AS_REW_ACTION_RATE_L2
 * term needs the latter. */
int as_rewards_step(const as_reward_term_t* terms, int32_t num_terms, const float* table, uint32_t kinds,
                    const as_reward_sources_t* sources, float* reward, float* episode_sums, float* step_reward,
                    float* last_episode_sums, float* prev_actions, const uint8_t* reset, const uint8_t* reset2,
                    int32_t n, float dt, void* stream);
/* RewardManager.reset(env_ids): for the envs with mask[e] != 0 ([n] uint8; NULL: every env) the episodic sums and
 * prev_actions (may be NULL) become 0; step_reward and the reward are left alone, as in the reference. */
int as_rewards_reset(float* episode_sums, int32_t num_terms, float* prev_actions, int32_t action_cols,
                     const uint8_t* mask, int32_t n, void* stream);

/* Termination manager, off by default: the done terms of cfg.terminations (isaaclab/managers/termination_manager.py,
 * the term functions of isaaclab/envs/mdp/terminations.py).  One launch computes every term of every env: per term in
 * cfg order term_dones[k] = f, and time_outs |= f for a term with time_out != 0, terminated |= f otherwise, both
 * started at 0; dones = time_outs | terminated.  Then, for an env with dones | step_terminated | step_truncated:
 * last_episode_dones[k] = term_dones[k] for every term (what the reference's reset would count, as a captured step
 * serves it); and reset_request = dones & ~(step_terminated | step_truncated): the envs the manager ends and the step
 * did not reset itself.  The caller launches it directly after as_step (and as_contact_forces where a term reads the
 * net forces) on the same stream; the state rows of an env the step reset are the post-reset ones.  A stateless
 * entry point over caller-owned device buffers -- no as_env_t.  Every buffer is field-major / env-minor ([rows][n]).
 * Formulas and the float32 operations: csrc/allsteps_terminations.h.  Graph-safe: the term descriptors and the index
 * table are read from device memory at every launch.  Symbols added only: AS_ABI_VERSION stays 6. */
#define AS_MAX_TERMINATION_TERMS 16
#define AS_MAX_TERMINATION_IDS 32   /* entries of a term's row of the index table (joints or bodies) */
#define AS_TERMINATION_TABLE_ROWS 3 /* table [3][AS_MAX_TERMINATION_TERMS][AS_MAX_TERMINATION_IDS] words: id | a | b */
enum {
  AS_TERMINATION_TIME_OUT = 0,            /* step_truncated | (ep_len >= i0)             i0 max_episode_length */
  AS_TERMINATION_COMMAND_RESAMPLE,        /* (time_left[row] <= p0) & (command_counter[row] == i0)   p0 step_dt */
  AS_TERMINATION_BAD_ORIENTATION,         /* |acos(-projected_gravity_b[2])| > p0        p0 limit_angle */
  AS_TERMINATION_ROOT_HEIGHT_BELOW_MINIMUM, /* root_pos[2] < p0                          p0 minimum_height */
  AS_TERMINATION_JOINT_POS_OUT_OF_LIMIT,  /* any q[id] > b or q[id] < a                  a, b the soft limits */
  AS_TERMINATION_JOINT_POS_OUT_OF_MANUAL_LIMIT, /* any q[id] > p1 or q[id] < p0          p0, p1 the bounds */
  AS_TERMINATION_JOINT_VEL_OUT_OF_MANUAL_LIMIT, /* any |qd[id]| > p0                     p0 max_velocity */
  AS_TERMINATION_ILLEGAL_CONTACT,         /* any body whose max-over-slots |net / sim_dt| > p0   p0 threshold */
  AS_TERMINATION_NUM_KINDS
};
typedef struct {
  int32_t kind;      /* AS_TERMINATION_* */
  int32_t time_out;  /* != 0: the term is a time-out, it enters time_outs; 0: terminated */
  int32_t num_ids;   /* entries of the term's index-table row, <= AS_MAX_TERMINATION_IDS */
  int32_t row;       /* the command term's row of time_left / command_counter */
  float p0, p1;      /* the kind's constants, formed by the host as float32 the way torch takes a Python scalar */
  int32_t i0;        /* max_episode_length / num_resamples */
  int32_t reserved0;
} as_termination_term_t;
typedef struct {
  const float* root_pos;            /* [3][n] */
  const float* root_quat;           /* [4][n] (w x y z) */
  const float* q;                   /* [joint_rows][n] */
  const float* qd;                  /* [joint_rows][n] */
  const float* time_left;           /* [command_terms][n] the command manager's, or NULL */
  const int32_t* command_counter;   /* [command_terms][n] the command manager's, or NULL */
  const float* net;                 /* [depth][bodies][3][n] as_contact_forces' net impulses, or NULL */
  const int32_t* ep_len;            /* [n] the step's episode length counter, or NULL */
  const uint8_t* step_terminated;   /* [n] the step's own flags: the step reset these envs itself; NULL: 0 */
  const uint8_t* step_truncated;    /* [n] or NULL: 0 */
  int32_t joint_rows, command_terms, depth, bodies;
  float sim_dt;                     /* the physics step: impulses / sim_dt are forces */
} as_termination_sources_t;
/* terms [num_terms] and table [AS_TERMINATION_TABLE_ROWS][AS_MAX_TERMINATION_TERMS][AS_MAX_TERMINATION_IDS] are
 * device memory.  kinds: bit k set for every AS_TERMINATION_* kind a descriptor may hold (the host's knowledge of the
 * device descriptors): a set bit whose source pointer is NULL is AS_ERR_INVALID, as are NULL terms / table / sources
 * / term_dones / time_outs / terminated / dones and num_terms outside [1, AS_MAX_TERMINATION_TERMS] -- all before
 * any device call.  A source that is NULL, or an id outside its rows, reads as 0 on the device.  term_dones and
 * last_episode_dones [num_terms][n], time_outs, terminated, dones and reset_request [n], all uint8 0 / 1;
 * last_episode_dones and reset_request may be NULL (not written). */
int as_terminations_step(const as_termination_term_t* terms, int32_t num_terms, const float* table, uint32_t kinds,
                         const as_termination_sources_t* sources, uint8_t* term_dones, uint8_t* time_outs,
                         uint8_t* terminated, uint8_t* dones, uint8_t* last_episode_dones, uint8_t* reset_request,
                         int32_t n, void* stream);

/* Action manager, off by default: the joint action terms of cfg.actions (isaaclab/managers/action_manager.py, the
 * terms of isaaclab/envs/mdp/actions: JointPositionAction, JointEffortAction, JointPositionToLimitsAction,
 * EMAJointPositionToLimitsAction).  A column is one (term, joint) pair in cfg order.  as_actions_step is
 * process_action: per (env, column) prev_action <- action, action <- input, processed <- the term's formula,
 * prev_applied <- processed for an EMA column, cmd[env][joint] <- processed.  as_actions_reset is reset(env_ids) over
 * the envs of mask | mask2 (both NULL: every env): action and prev_action are zeroed, an EMA column's prev_applied
 * becomes q[joint][env].  The caller launches as_actions_step before as_step on the same stream and gives the step
 * the command buffer with as_set_joint_commands.  Stateless entry points over caller-owned device buffers -- no
 * as_env_t.  input, action, prev_action, processed and prev_applied are env-major [n][num_cols]; cmd is
 * [n][cmd_cols] (cfg dof order) and q is field-major [cmd_cols][n].  Formulas and the float32 operations:
 * csrc/allsteps_actions.h.  Graph-safe: the column descriptors are read from device memory at every launch; a
 * column whose joint is outside [0, cmd_cols) stores no command and reads no q.  Symbols added only: AS_ABI_VERSION
 * stays 6. */
enum {
  AS_ACTION_JOINT_POSITION = 0,       /* clamp(raw * scale + offset, clip)            a position target */
  AS_ACTION_JOINT_EFFORT,             /* the same                                     an effort */
  AS_ACTION_POSITION_TO_LIMITS,       /* clamp(raw * scale, clip), rescaled over the soft limits with rescale */
  AS_ACTION_EMA_POSITION_TO_LIMITS,   /* the same, then the moving average over prev_applied, clamped to the limits */
  AS_ACTION_NUM_KINDS
};
typedef struct {
  int32_t joint;     /* the column's joint: its column of cmd and row of q (cfg dof order) */
  int32_t kind;      /* AS_ACTION_* */
  int32_t rescale;   /* != 0: rescale_to_limits */
  int32_t term;      /* the term the column belongs to (informational) */
  float scale, offset;
  float clip_lo, clip_hi;  /* -inf / +inf without a clip */
  float lim_lo, lim_hi;    /* the joint's soft position limits */
  float alpha, one_minus_alpha;  /* both formed by the host as torch forms them */
} as_action_column_t;
/* cols [num_cols] is device memory, 1 <= num_cols <= AS_ACT_DIM, 1 <= cmd_cols <= AS_ACT_DIM.  NULL buffers and
 * counts out of range are AS_ERR_INVALID before any device call. */
int as_actions_step(const as_action_column_t* cols, int32_t num_cols, const float* input, float* action,
                    float* prev_action, float* processed, float* prev_applied, float* cmd, int32_t cmd_cols,
                    int32_t n, void* stream);
int as_actions_reset(const as_action_column_t* cols, int32_t num_cols, float* action, float* prev_action,
                     float* prev_applied, const float* q, int32_t q_rows, const uint8_t* mask, const uint8_t* mask2,
                     int32_t n, void* stream);
/* The seam in the physics step, a setup call like as_set_contact_report: with cmd_dev set, every later as_step,
 * as_physics_step and as_quad_step reads joint j's command of env e at cmd_dev[e * num_hinges + j] (cfg dof order)
 * in place of the actuator's own formula -- in AS_ACT_TORQUE the applied effort is the command itself (no curriculum
 * gain, no gear, no clip), in AS_ACT_DC_MOTOR the position target is the command itself.  The task epilogues keep
 * reading the clamped raw action.  Reset and task-only launches ignore it.  NULL switches it off.  The buffer is
 * caller-owned and must stay alive. */
int as_set_joint_commands(as_env_t* env, const float* cmd_dev);

/* The H^-1 sweep plan for a model (round 6, ABI 5; no device needed). The step kernel sweeps the
 * padded joint-space inertia last block first and, for the trees it is compiled for (the walker, the
 * C5 quadruped), skips the column quads in which the pivot rows are structurally zero -- an exact
 * identity, so results do not depend on it.  Returns 1 when the compiled skips hold for `model` (as_create
 * then launches the skipping kernel), 0 when they do not (the full sweep runs), <0 on an invalid model;
 * *skip_mask (if not NULL) receives the quads that are zero for this model (bit r (NB-1) + q: round r,
 * quad q).  Replaces nothing in the reference: PhysX factors the articulation internally. */
int as_sweep_plan(const as_model_t* model, uint64_t* skip_mask);

/* Per-launch timing: record HIP events around the step kernel (k_step) and the observation
 * kernel (k_obs) of the next `max_launches` calls on their own stream; as_profile_read
 * synchronises on the last event and returns the summed durations (ms) and the launch count. */
int as_profile(as_env_t* env, int32_t max_launches);
/* Sampled form: time every `stride`-th call only (up to `max_records` of them), so the events'
 * launch gaps touch 1 / stride of the calls of a timed loop. */
int as_profile_sampled(as_env_t* env, int32_t max_records, int32_t stride);
int as_profile_read(as_env_t* env, double* step_kernel_ms, double* obs_kernel_ms, int32_t* launches);

/* Diagnostic: when stamps_dev (device, >= 32 uint64) is non-null, every k_step wave adds the
 * s_memtime cycles of each of its 15 phases (load, fk, rnea, H rows, H^-1 sweep, solve, collide,
 * rows, W, pgs, integrate, final fk, task, reset, store) to slots 0..14; slot 15 keeps the largest
 * single-wave total of any launch and slots 16..30 the largest single-wave cycles of each phase
 * (atomicMax).  If slot 31 is non-zero on entry, the buffer must hold 64 + 30 * ceil(num_envs / 2)
 * words and each wave instead stores (no atomics) a 30-word record of its own at 64 + 30 * block,
 * overwritten by every launch (scripts/stamps.py): words 0..25 the phases, total, start / end
 * s_memtime, HW_ID, XCC_ID, rows and contacts per env, start / end s_memrealtime; words 26, 27
 * collide's stone pairs of the wave's first / second env (bits 0-15: summed over the launch's
 * substeps, bits 16-31: the largest single flush); word 28 the wave's stone-pair flushes per lane-group
 * level, 8 bits each (one lane per pair, L = 2, 3, 4); word 29 unused.  A buffer sized for the former
 * 26-word records is too small: the waves write past it.  Pass NULL to switch off. */
int as_debug_stamps(as_env_t* env, uint64_t* stamps_dev);

/* Graph-safe stepping (on != 0): every as_step / as_task_step / as_reset_* uses the SAME counter bank,
 * cleared by a one-block kernel at the start of the call, instead of alternating two banks from host
 * state -- so a call captured once in a HIP graph (hipStreamBeginCapture) can be replayed any number
 * of times.  Off (default): two banks, no memset (lowest eager launch count). */
int as_set_graph_safe(as_env_t* env, int32_t on);

/* Device counters of the last step: [0] = any env reset, [1] = sum of curr_target_index, [3] = contacts
 * the constraint budget cut (found by the narrowphase beyond the AS_MAX_CONTACTS / AS_MAX_ROWS - limit
 * rows cap, summed over the step's envs and substeps; PhysX keeps every contact,
 * simulation_cfg.py:110 gpu_max_rigid_contact_count = 2**23).  Valid until the step after next. */
int as_step_counters(as_env_t* env, const int32_t** counters_dev);
/* The same four words [0..3] copied to the host after `stream` (the stream the step ran on) drains;
 * synchronises the stream -- a diagnostic read (tests, bench), never inside a timed step. */
int as_step_counters_host(as_env_t* env, int32_t* out_host, void* stream);
int as_get_curriculum_host(as_env_t* env, int32_t* level_host); /* synchronises the stream */

/* Diagnostic (SURVEY §8d "confirm with an in-repo STREAM-copy kernel"): dst[i] = src[i] for
 * n16 16-byte elements (both device pointers 16-B aligned, non-overlapping), a grid-stride copy
 * with non-temporal loads/stores sized to fill all 256 CUs.  bench.py times it with HIP events to
 * report the achievable HBM bandwidth beside the 8 TB/s spec peak. */
int as_hbm_copy(void* dst, const void* src, int64_t n16, void* stream);

int as_abi_version(void);
const char* as_last_error(void);
/* Provenance: the source digest the library was compiled from (-DAS_BUILD_ID, computed by
 * allsteps_isaaclab_amd/_native.py::source_digest over csrc/ + include/ + the compile flags).  The
 * Python loader refuses a library whose digest differs from the tree's, so a stale or variant build
 * is never run silently ("unversioned" when built without the define). */
const char* as_build_id(void);

#ifdef __cplusplus
}
#endif
#endif
