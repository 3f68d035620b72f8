// allsteps_kernels.h -- host/device interface of the step kernels (internal to liballsteps_hip.so).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/allsteps.h"
#include "allsteps_consts.h"
#include "allsteps_contact_report.h"
#include "allsteps_lane_table.h"
#include "allsteps_pair_group.h"

namespace as {

// The contact report's buffers (as_contact_report_t) as the kernels read them: a block in device memory that
// as_set_contact_report fills, so that a launch carries one pointer and k_step reads the rest (uniform: scalar
// loads) only where it stores.
struct ReportDesc {
  int32_t* count;
  uint32_t* records;
  float* qd_prev;
  int32_t depth;
};

enum { kModeStep = 0, kModeReset = 1, kModePhysics = 2, kModeTask = 3 };

struct StepArgs {
  const Consts* consts;
  as_state_t st;
  int32_t n;
  int32_t mode;
  const float* actions;
  float* reward;
  float* obs;                  // [n][59] observation rows (speculative second tick, see k_step)
  uint32_t* side;              // [kSideWords][n]: tick-#1 state and observation entries for k_obs
  uint8_t* terminated;
  uint8_t* truncated;
  const float* reset_draws;
  const uint8_t* reset_mask;   // kModeReset: envs to reset (null: all)
  int32_t* counters;  // one bank (kCntBank ints, zero at launch: see k_obs), layout below
  uint64_t seed;
  int64_t env_offset;
  unsigned long long* stamps;  // diagnostic phase timing (s_memtime deltas summed over waves) or null
  const int32_t* wave_map;     // [2 * blocks] env of each workgroup half (see kMapEnvs) or null: xcd_block
  const ReportDesc* rep;       // the opt-in contact report (step_report.h), or null: off
  const float* cmd;            // the opt-in joint commands [n][num_hinges] (as_set_joint_commands) of a physics
                               // launch, or null: the hard-wired action formulas
};

// phase ids of the diagnostic stamps (as_debug_stamps)
enum {
  kStLoad = 0, kStFK, kStLinkQ, kStDyn, kStChol, kStSolve, kStCollide, kStRows, kStWsolve, kStPGS,
  kStIntegrate, kStFKFinal, kStTask, kStReset, kStStore, kNumStamps
};

// Step counters, one bank per launch (two banks alternate; k_obs clears the next one):
//   [0]  any env reset (plain store of 1)
//   [1]  sum of curr_target_index over all envs, published by k_obs from the partial sums
//   [2]  kCntLevel (regen_footsteps)
//   [3]  contacts cut by the row budget in this launch, all envs and substeps (kCntDropped)
//   [kCntStride * (1 + i)], i < kCntSlots: partial sums, one atomic per wave into slot block % kCntSlots
//        (one 64-B line each: 4096 same-address atomics serialise at the memory side)
constexpr int kCntSlots = 16;
constexpr int kCntStride = 16;
constexpr int kCntBank = kCntStride * (1 + kCntSlots);

// side buffer of k_step -> k_obs: idx, prev, next, count, swing, pot, old_pot, foot_contact[2]
// (tick-#1 state) and foot_contact[2], targets[9] (tick-#1 observation entries 48..58)
constexpr int kSideState = 9;
constexpr int kSideObs = 11;
constexpr int kSideRegen = kSideState + kSideObs;  // 1 = reset env due new stones (regen_footsteps)
constexpr int kSideCost = kSideRegen + 1;   // constraint rows of the env over this launch's substeps
constexpr int kSideWords = kSideCost + 1;

// Cost-balanced wave placement (k_obs / k_quad -> the next k_step; placement only, never results).
// k_obs ranks each chunk of kMapEnvs consecutive envs by the constraint rows they had in this launch,
// puts ranks 2p and 2p + 1 in one wave (pair p, 0 = heaviest) and places pair p of chunk w at workgroup
//   resident grid (the whole grid fits the chip, 8 one-wave workgroups per CU):
//     p < 16: p C + w,   p >= 16: n / 4 + (31 - p) C + w        (C = n / 64 chunks)
//   -- workgroups b and b + n / 4 share a SIMD (measured, scripts/simd_mates.py), and a wave's cycles
//   grow with its PARTNER's rows more than with its own, so the heaviest wave gets the lightest partner;
//   streamed grid (more workgroups than slots): p C + w, so the dispatcher starts the heaviest pairs of
//   every chunk first and the lightest last (longest-processing-time-first order).
// Either way workgroup b runs on XCD b % 8 = w % 8 (C is a multiple of 8): a chunk's envs stay in one
// XCD's L2.  wave_map[2 b + h] = the env of workgroup b's half h.
constexpr int kMapEnvs = 64;
__host__ __device__ inline bool wave_map_fits(int n) { return n > 0 && n % (8 * kMapEnvs) == 0; }
__host__ __device__ inline int wave_map_block(int w, int p, int n, bool streamed) {
  const int C = n / kMapEnvs;
  if (streamed || p < kMapEnvs / 4) return p * C + w;
  return (n >> 2) + (kMapEnvs / 2 - 1 - p) * C + w;
}
constexpr int kCntLevel = 2;  // counter-bank word: the curriculum level k_step saw (k_obs regen level)
constexpr int kCntDropped = 3;  // counter-bank word: contacts found past the row budget (as_step_counters [3])

// k_quad (BASELINE C5 task epilogue, one env per lane)
struct QuadArgs {
  const Consts* consts;
  as_state_t st;
  int32_t n;
  int32_t reset_all;           // 1: reset every env (as_quad_reset_all), no task step
  const float* actions;        // [n][nh]
  float* obs;                  // [n][AS_QUAD_OBS_DIM]
  float* reward;
  uint8_t* terminated;
  uint8_t* truncated;
  uint64_t seed;
  int64_t env_offset;
  const uint32_t* side;        // k_step's side buffer (the row counts of the placement)
  int32_t* wave_map;           // null, or rebuilt here for the next k_step (kMapEnvs)
  int32_t map_streamed;        // wave_map_block
  const ReportDesc* rep;       // the contact report, whose counts are cleared for the envs reset here, or null
};

struct ObsArgs {
  const Consts* consts;
  as_state_t st;
  int32_t n;
  int32_t* counters;       // this launch's bank (k_obs publishes the sum into [1])
  int32_t* next_counters;  // the other bank, cleared here for the next launch
  float* obs;
  const uint32_t* side;
  uint64_t seed;
  int64_t env_offset;
  int32_t* wave_map;       // null, or rebuilt here for the next k_step from the side buffer's row counts
  int32_t map_streamed;    // wave_map_block: the grid streams through the chip (LPT order)
};

struct StonesArgs {
  const Consts* consts;
  float* stones;
  int32_t n;
  int32_t level;
  const float* draws;
  uint64_t seed;
  int64_t env_offset;
};

// k_body_state (ring-2 views, as_body_state): the step kernel's FK of the current state, then every
// body's pose and velocities
struct BodyArgs {
  const Consts* consts;
  as_state_t st;
  int32_t n;
  float* out;                  // [AS_BODY_STATE_ROWS][nb][n]
  as_body_table_t bodies;
};

// k_imu (as_imu, imu_kernels.h): k_body_state's FK, then the IMU update of every sensor of every outdated env;
// buffers field-major / env-minor (allsteps_imu.h)
struct ImuArgs {
  const Consts* consts;
  as_state_t st;
  int32_t n;
  int32_t all;                 // != 0: treat every env as outdated
  float dt;
  uint8_t* outdated;           // [n]
  float* data;                 // [19][S][n]
  float* prev;                 // [6][S][n]
  as_imu_table_t imus;
};

// k_frame_transformer (as_frame_transformer, frame_transformer_kernels.h): k_body_state's FK, then every target
// frame of every sensor in the world and in its source frame; buffers field-major / env-minor
// (allsteps_frame_transformer.h)
struct FrameTransformerArgs {
  const Consts* consts;
  as_state_t st;
  int32_t n;
  float* source;               // [7][S][n]
  float* target;               // [14][F][n]
  as_frame_table_t frames;
};

// k_contact_forces (as_contact_forces): dense sums over the contact report
struct ForcesArgs {
  int32_t n;
  int32_t depth;
  const int32_t* count;
  const uint32_t* records;
  float* matrix;               // [depth][AS_REPORT_FEET][AS_NUM_STONES][3][n]
  float* net;                  // [depth][nb][3][n]
  int32_t num_bodies;
  int32_t link[AS_MAX_BODIES];
};

// k_noise_actions / k_noise_post (as_noise_actions / as_noise_post, noise_kernels.h).  A model travels by
// value; kind AS_NOISE_NONE: no model.  gshift = log2(noise_group(cols)): lanes per env
struct NoiseActArgs {
  as_noise_model_t m;
  const float* in;             // [n][cols]
  float* out;                  // [n][cols]
  int32_t n, cols, gshift;
  const uint32_t* t;           // [n] per-env step counter of the noise stream
  const float* draws;          // [n][cols] injected draws or null: Philox
  uint64_t seed;
  int64_t env_offset;
};

struct NoisePostArgs {
  as_noise_model_t act, obs;
  float* data;                 // [n][cols] observations, noised in place, or null: biases and counter only
  int32_t n, cols, gshift;
  uint32_t* t;
  const uint8_t* reset;        // [n] envs whose biases are re-drawn (null: all)
  const uint8_t* reset2;       // [n] a second mask, ORed with the first, or null
  const float* obs_draws;      // [n][cols] or null
  const float* act_bias_draws; // [n] or null
  const float* obs_bias_draws; // [n] or null
  uint64_t seed;
  int64_t env_offset;
};

// k_events_interval / k_events_init (as_events_interval / as_events_init, event_kernels.h): every buffer
// field-major / env-minor.  k_events_init reads terms, num_terms, n, time_left, t, interval_draws, seed,
// env_offset only
struct EventsArgs {
  const as_event_term_t* terms;  // [num_terms] device memory
  int32_t num_terms, n;
  float* root_lin;               // [3][n]
  float* root_ang;               // [3][n]
  float* time_left;              // [num_terms][n]
  uint32_t* t;                   // [n] per-env counter of the event streams
  uint8_t* fired;                // [num_terms][n] or null: not written
  const float* interval_draws;   // [num_terms][n] injected draws or null: Philox
  const float* push_draws;       // [num_terms][6][n] injected draws or null: Philox
  float dt;
  uint64_t seed;
  int64_t env_offset;
};

// k_observations / k_observations_reset (as_observations_step / as_observations_reset, observation_kernels.h): one
// group of cfg.observations.  k_observations_reset reads out, out_cols, count, n and `reset` as its mask (null: every
// env) only
struct ObservationsArgs {
  const as_observation_term_t* terms;  // [num_terms] device memory
  const float* cols;                   // [AS_OBS_COL_ROWS][AS_MAX_OBS_COLS] 32-bit words, device memory
  const int32_t* omap;                 // [out_cols] device memory
  int32_t num_terms, d0, out_cols, group, n;
  as_observation_sources_t src;
  float* out;                          // [n][out_cols]
  int32_t* count;                      // [n] pushes since the env's reset
  uint32_t* t;                         // [n] per-env counter of the group's stream
  const uint8_t* reset;                // [n] or null
  const uint8_t* reset2;               // [n] a second mask, ORed with the first, or null
  const float* draws;                  // [d0][n] injected draws or null: Philox
  uint64_t seed;
  int64_t env_offset;
};

// k_rewards_step / k_rewards_reset (as_rewards_step / as_rewards_reset, reward_kernels.h): the terms of cfg.rewards.
// k_rewards_reset reads episode_sums, num_terms, prev_actions, src.action_cols, n and `reset` as its mask (null:
// every env) only
struct RewardsArgs {
  const as_reward_term_t* terms;  // [num_terms] device memory
  const float* table;             // [AS_REW_TABLE_ROWS][AS_MAX_REW_TERMS][AS_MAX_REW_IDS] 32-bit words, device memory
  int32_t num_terms, n;
  as_reward_sources_t src;
  float* reward;                  // [n]
  float* episode_sums;            // [num_terms][n]
  float* step_reward;             // [num_terms][n]
  float* last_episode_sums;       // [num_terms][n] or null: not written
  float* prev_actions;            // [n][action_cols] or null: not written, reads as 0
  const uint8_t* reset;           // [n] or null
  const uint8_t* reset2;          // [n] a second mask, ORed with the first, or null
  float dt;
};

// k_terminations_step (as_terminations_step, termination_kernels.h): the terms of cfg.terminations
struct TerminationsArgs {
  const as_termination_term_t* terms;  // [num_terms] device memory
  const float* table;  // [AS_TERMINATION_TABLE_ROWS][AS_MAX_TERMINATION_TERMS][AS_MAX_TERMINATION_IDS] words, device
  int32_t num_terms, n;
  as_termination_sources_t src;
  uint8_t* term_dones;          // [num_terms][n]
  uint8_t* time_outs;           // [n]
  uint8_t* terminated;          // [n]
  uint8_t* dones;               // [n]
  uint8_t* last_episode_dones;  // [num_terms][n] or null: not written
  uint8_t* reset_request;       // [n] or null: not written
};

// k_actions_process / k_actions_reset (as_actions_step / as_actions_reset, action_kernels.h): the joint terms of
// cfg.actions.  The per-column buffers are env-major [n][num_cols]
struct ActionsArgs {
  const as_action_column_t* cols;  // [num_cols] device memory
  int32_t num_cols, cmd_cols, n;   // cmd_cols: the robot's hinges, the rows of q and the columns of cmd
  const float* input;              // [n][num_cols] the policy's action (process only)
  float* action;                   // [n][num_cols]
  float* prev_action;              // [n][num_cols]
  float* processed;                // [n][num_cols] (process only)
  float* prev_applied;             // [n][num_cols] the EMA columns' state
  float* cmd;                      // [n][cmd_cols] the joint commands, cfg dof order (process only)
  const float* q;                  // [cmd_cols][n] joint positions (reset only)
  const uint8_t* mask;             // [n] reset: the envs to reset, with mask2; both null: every env
  const uint8_t* mask2;
};

// k_commands_step / k_commands_reset (as_commands_step / as_commands_reset, command_kernels.h): every buffer
// field-major / env-minor.  k_commands_reset reads no root state, no dt and `reset` as its mask (null: every env)
struct CommandsArgs {
  const as_command_term_t* terms;  // [num_terms] device memory
  int32_t num_terms, n;
  const float* root_quat;          // [4][n]
  const float* root_lin;           // [3][n]
  const float* root_ang;           // [3][n]
  float* vel;                      // [num_terms][3][n]
  float* heading_target;           // [num_terms][n]
  uint8_t* flags;                  // [num_terms][kCommandFlagRows][n]
  float* time_left;                // [num_terms][n]
  int32_t* counter;                // [num_terms][n]
  float* metrics;                  // [num_terms][kCommandMetricRows][n]
  float* last_metrics;             // [num_terms][kCommandMetricRows][n] or null: not written
  uint32_t* t;                     // [n] per-env counter of the command streams
  const uint8_t* reset;            // [n] or null
  const uint8_t* reset2;           // [n] a second mask, ORed with the first, or null
  const float* draws;              // [phases][num_terms][kCommandDraws][n] injected draws or null: Philox
  float dt;
  uint64_t seed;
  int64_t env_offset;
};

// k_contact_timers (as_contact_timers, contact_timer_kernels.h): the air / contact timers over the contact
// report; every buffer field-major / env-minor
struct TimersArgs {
  int32_t n;
  int32_t updates;             // sensor updates to apply: 0 (reset only) or the report's depth
  const int32_t* count;
  const uint32_t* records;
  float* timers;               // [kTimerRows][nb][n]
  float* timestamp;            // [n]
  const uint8_t* reset;        // [n] envs reset after the updates, or null: all when updates == 0, else none
  const uint8_t* reset2;       // [n] a second mask, ORed with the first, or null
  float dt;                    // sim.dt
  float force_threshold;
  int32_t num_bodies;
  int32_t link[AS_MAX_BODIES];
};

// k_ray_cast (as_ray_cast, ray_caster_kernels.h): the height scanner's rays against the ground and the stones;
// every buffer field-major / env-minor (allsteps_ray_caster.h)
struct RayArgs {
  int32_t n;
  int32_t num_rays;
  int32_t chunk;               // rays per slice (launch_ray_cast sizes it)
  int32_t attach_yaw_only;
  int32_t surfaces;            // AS_RAY_GROUND | AS_RAY_STONES
  int32_t num_steps;           // stones per env
  float max_distance, ground_z;
  float half[3];               // sim.stone_half
  const float* root_pos;       // [3][n]
  const float* root_quat;      // [4][n]
  const float* stones;         // [3 * AS_NUM_STONES][n]
  const float* rays;           // [6][num_rays] device memory
  float* hits;                 // [3][num_rays][n]
  int8_t* surface;             // [num_rays][n] or null
  float* pose;                 // [7][n] or null
};

// k_ray_camera (as_ray_camera, ray_camera_kernels.h): the depth camera's pixels against the ground and the stones;
// inputs env-minor, images env-major (allsteps_ray_camera.h)
struct CamArgs {
  int32_t n;
  int32_t num_rays;            // width * height
  int32_t surfaces;            // AS_RAY_GROUND | AS_RAY_STONES
  int32_t clipping;            // AS_CAM_CLIP_*
  int32_t num_steps;           // stones per env
  float max_distance, ground_z;
  float half[3];               // sim.stone_half
  const float* root_pos;       // [3][n]
  const float* root_quat;      // [4][n]
  const float* stones;         // [3 * AS_NUM_STONES][n]
  const float* dirs;           // [3][num_rays] device memory
  const float* offset;         // [7][n] device memory
  float* pose;                 // [7][n]
  float* plane;                // [n][num_rays] or null
  float* camera;               // [n][num_rays] or null
  float* normals;              // [n][num_rays][3] or null
};

bool step_supported_nv(int nv);
hipError_t launch_ray_cast(RayArgs a, hipStream_t stream);
hipError_t launch_ray_camera(const CamArgs& a, hipStream_t stream);
hipError_t launch_imu(const ImuArgs& a, hipStream_t stream);
hipError_t launch_frame_transformer(const FrameTransformerArgs& a, hipStream_t stream);
hipError_t launch_contact_timers(const TimersArgs& a, hipStream_t stream);
hipError_t launch_commands_step(const CommandsArgs& a, hipStream_t stream);
hipError_t launch_commands_reset(const CommandsArgs& a, hipStream_t stream);
hipError_t launch_observations(const ObservationsArgs& a, hipStream_t stream);
hipError_t launch_observations_reset(const ObservationsArgs& a, hipStream_t stream);
hipError_t launch_rewards_step(const RewardsArgs& a, hipStream_t stream);
hipError_t launch_rewards_reset(const RewardsArgs& a, hipStream_t stream);
hipError_t launch_terminations_step(const TerminationsArgs& a, hipStream_t stream);
hipError_t launch_actions_process(const ActionsArgs& a, hipStream_t stream);
hipError_t launch_actions_reset(const ActionsArgs& a, hipStream_t stream);
hipError_t launch_events_interval(const EventsArgs& a, hipStream_t stream);
hipError_t launch_events_init(const EventsArgs& a, hipStream_t stream);
hipError_t launch_noise_actions(const NoiseActArgs& a, hipStream_t stream);
hipError_t launch_noise_post(const NoisePostArgs& a, hipStream_t stream);
hipError_t launch_contact_forces(const ForcesArgs& a, hipStream_t stream);
hipError_t launch_body_state(const BodyArgs& a, hipStream_t stream);
hipError_t launch_step(const StepArgs& a, int nv, bool sweep_skip, hipStream_t stream);
hipError_t launch_obs(const ObsArgs& a, hipStream_t stream);
hipError_t launch_stones(const StonesArgs& a, hipStream_t stream);
hipError_t launch_quad(const QuadArgs& a, hipStream_t stream);
// k_quad's reset path for the envs of a device mask [n] (uint8), nothing for the others; a.reset_all, a.actions,
// a.reward, a.terminated, a.truncated, a.side, a.wave_map are not read
hipError_t launch_quad_reset_mask(const QuadArgs& a, const uint8_t* mask, hipStream_t stream);
// zero n int32 words with a kernel (graph-safe stepping: a kernel node instead of a memset node)
hipError_t launch_zero(int32_t* p, int n, hipStream_t stream);
size_t step_lds_bytes();

}  // namespace as
