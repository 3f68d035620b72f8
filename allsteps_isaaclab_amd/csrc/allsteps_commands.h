// allsteps_commands.h -- the command manager's velocity commands (cfg.commands): the term step, the draw layout
// and the Philox stream.
//
// The reference's ManagerBasedRLEnv.step resets the envs that are done, then calls command_manager.compute(dt),
// then applies the interval events (manager_based_rl_env.py:220-239, 347-380).  Its velocity terms are
// UniformVelocityCommand and NormalVelocityCommand (envs/mdp/commands/velocity_command.py) on the base class
// CommandTerm (managers/command_manager.py).  Per term and per env, in float32, every operation rounded on its own
// (the library is built with -ffp-contract=off), so the same draws give torch's bits.  The one fused operation is
// the sample s(d, w, lo) = fmaf(d, w, lo): torch's uniform_ and normal_ fills are compiled with their multiply-add
// contracted, on the CPU's vector loops as by nvcc's default, which tests/golden/gen_commands.py establishes
// against real torch; fmaf is correctly rounded on the host and on the device alike.  Two more of torch's kernels
// are compiled that way and restated with fmaf: a cross product's a1 b2 - a2 b1 = fmaf(a1, b2, -(a2 b1)), and
// torch.norm's sum of squares, fmaf(y, y, x x).
//
//   reset (CommandTerm.reset, an env the step reset):
//     last_metrics = metrics;  metrics = 0;  command_counter = 0;  resample
//   compute (CommandTerm.compute(dt), every env):
//     lin_b = quat_rotate_inverse(q, root_lin);  ang_b = quat_rotate_inverse(q, root_ang)       math.py:606-625
//     error_vel_xy  += sqrtf(fmaf(dy, dy, dx dx)) / max_command_step  dx = vel[0] - lin_b[0], dy = vel[1] - lin_b[1]
//     error_vel_yaw += fabsf(vel[2] - ang_b[2]) / max_command_step    an IEEE division each
//     time_left -= dt;  resample where time_left <= 0;  update
//   resample (CommandTerm._resample):
//     time_left = s(d0, time_w, time_lo);  command_counter += 1
//     uniform term: vel[c] = s(d(1 + c), w[c], lo[c])  (c = x y yaw);  with heading_command: heading_target =
//                   s(d4, w[3], lo[3]), is_heading = d5 <= p_heading;  is_standing = d6 <= p_standing
//     normal term:  vel[c] = s(d(1 + c), std[c], mean[c]) (d(4 + c) <= 0.5 ? 1 : -1);  is_zero[c] = d(7 + c) <=
//                   p_zero[c];  is_standing = d10 <= p_standing        d1..d3 unit normals, the rest uniforms
//   update (_update_command):
//     uniform term with heading_command, a heading env:
//       fwd = quat_apply(q, (1, 0, 0))  (math.py:546-564: t = (xyz x v) 2;  (v + w t) + xyz x t)
//       heading_w = as_atan2f(fwd.y, fwd.x)                             include/as_detmath.h, <= 2.5 ulp: the one
//       a = heading_target - heading_w                                  operation that is not torch's bit for bit
//       m = fmodf(a + pi, 2 pi), + 2 pi where m < 0 (torch's %);  e = (m == 0 and a > 0) ? pi : m - pi   wrap_to_pi
//       vel[2] = min(max(stiffness e, clip_lo), clip_hi)
//     then a standing env has vel = 0; the normal term then zeroes vel[c] where is_zero[c].
// The host forms every constant of as_command_term_t (envs/commands.py); nothing here forms one.
//
// An env the step reset resamples in its reset and may resample again in the same step's compute (its new
// time_left - dt <= 0), so the two phases draw from separate sets.
//
// Draws: Philox4x32-10 keyed by the env's seed, counter (env_id_offset + e, t[e], block, tag) -- the layout of the
// reset, noise and event streams with a per-env command counter t[e] of its own, advanced once per launch of
// k_commands_step or k_commands_reset (command_kernels.h).  The tag is the phase: "CmRs" the reset's resample,
// "CmCp" the compute's.  Term k owns blocks 3k .. 3k + 2, twelve uniforms u0 .. u11, and consumes kCommandDraws =
// 11 draws d0 .. d10 of them:
//     uniform term   d0 .. d6 = u0 .. u6       time | x y yaw | heading | is_heading | is_standing
//     normal term    d0 = u0                   time
//                    (d1, d2) = noise_box_muller(u1, u2);  d3 = the first of noise_box_muller(u3, u4)
//                    d4 .. d10 = u5 .. u11     three signs | three zero tests | is_standing
// A term draws what the reference draws, in its order; a draw the term's cfg does not use is not consumed.  The
// global env id is in the counter, so shards equal the unsharded run.
//
// Plain C++ with no HIP dependency: tests/commands_check.cpp runs all of it on the host.
#pragma once

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/allsteps.h"
#include "../../include/as_detmath.h"
#include "allsteps_base_frame.h"
#include "allsteps_noise.h"

// the short loops over components are unrolled on the device, so that the draws and the state stay in registers
#if defined(__HIPCC__) || defined(__CUDACC__)
#define AS_CMD_UNROLL _Pragma("unroll")
#else
#define AS_CMD_UNROLL
#endif

namespace as {

constexpr uint32_t kCommandResetTag = 0x436d5273u;    // "CmRs": the resample of an env's reset
constexpr uint32_t kCommandComputeTag = 0x436d4370u;  // "CmCp": the resample of compute's time-out
constexpr int kCommandDraws = 11;                     // draws a term consumes per resample, at most
constexpr int kCommandBlocks = 3;                     // Philox blocks a term owns per phase
constexpr float kCommandPi = 3.14159274101257324219f;     // float32(torch.pi)
constexpr float kCommandTwoPi = 6.28318548202514648438f;  // float32(2 torch.pi)

// the flag rows of a term: flags [terms][kCommandFlagRows][n] uint8
enum { kCmdHeading = 0, kCmdStanding = 1, kCmdZeroX = 2, kCmdZeroY = 3, kCmdZeroYaw = 4, kCommandFlagRows = 5 };
// the metric rows of a term: metrics / last_metrics [terms][kCommandMetricRows][n]
enum { kCmdErrXY = 0, kCmdErrYaw = 1, kCommandMetricRows = 2 };

// One env's state of one term, held by the caller
struct CommandState {
  float vel[3];          // vel_command_b
  float heading_target;
  bool flag[kCommandFlagRows];
  float time_left;
  int32_t counter;       // command_counter
  float metrics[kCommandMetricRows];
};

// the kCommandDraws draws of term k in the phase `tag`
AS_NZ_FN void command_draws(const as_command_term_t& c, uint64_t seed, uint32_t env, uint32_t t, int term,
                            uint32_t tag, float (&d)[kCommandDraws]) {
  // every element is assigned once, by value: a store under the kind's branch would make the index dynamic on the
  // device and put the draws into scratch memory
  const bool normal = c.kind == AS_COMMAND_NORMAL;
  float a[4], b[4], g[4] = {0.f, 0.f, 0.f, 0.f}, z0 = 0.f, z1 = 0.f, z2 = 0.f;
  noise_philox_block(seed, env, t, (uint32_t)(kCommandBlocks * term), tag, a);
  noise_philox_block(seed, env, t, (uint32_t)(kCommandBlocks * term + 1), tag, b);
  if (normal) {
    float unused;
    noise_philox_block(seed, env, t, (uint32_t)(kCommandBlocks * term + 2), tag, g);
    noise_box_muller(a[1], a[2], &z0, &z1);
    noise_box_muller(a[3], b[0], &z2, &unused);
  }
  d[0] = a[0];
  d[1] = normal ? z0 : a[1];
  d[2] = normal ? z1 : a[2];
  d[3] = normal ? z2 : a[3];
  d[4] = normal ? b[1] : b[0];
  d[5] = normal ? b[2] : b[1];
  d[6] = normal ? b[3] : b[2];
  d[7] = g[0]; d[8] = g[1]; d[9] = g[2]; d[10] = g[3];
}

// tensor.uniform_(lo, hi) and normal_(mean, std) from a unit draw: one fused multiply-add, as torch's fills
AS_NZ_FN float command_sample(float d, float w, float lo) { return fmaf(d, w, lo); }

// CommandTerm._resample and the term's _resample_command
AS_NZ_FN void command_resample(const as_command_term_t& c, CommandState& s, const float (&d)[kCommandDraws]) {
  s.time_left = command_sample(d[0], c.time_w, c.time_lo);
  s.counter += 1;
  if (c.kind == AS_COMMAND_NORMAL) {
    AS_CMD_UNROLL
    for (int k = 0; k < 3; ++k) {
      const float v = command_sample(d[1 + k], c.w[k], c.lo[k]);
      s.vel[k] = v * (d[4 + k] <= 0.5f ? 1.0f : -1.0f);
      s.flag[kCmdZeroX + k] = d[7 + k] <= c.p_zero[k];
    }
    s.flag[kCmdStanding] = d[10] <= c.p_standing;
  } else {
    AS_CMD_UNROLL
    for (int k = 0; k < 3; ++k) s.vel[k] = command_sample(d[1 + k], c.w[k], c.lo[k]);
    if (c.heading) {
      s.heading_target = command_sample(d[4], c.w[3], c.lo[3]);
      s.flag[kCmdHeading] = d[5] <= c.p_heading;
    }
    s.flag[kCmdStanding] = d[6] <= c.p_standing;
  }
}

// CommandTerm.reset up to its resample: the metrics' snapshot and the counter
AS_NZ_FN void command_reset_head(CommandState& s, float (&last_metrics)[kCommandMetricRows]) {
  AS_CMD_UNROLL
  for (int k = 0; k < kCommandMetricRows; ++k) {
    last_metrics[k] = s.metrics[k];
    s.metrics[k] = 0.0f;
  }
  s.counter = 0;
}

// the base-frame expressions (cross, quat_rotate_inverse, the heading's forward vector): allsteps_base_frame.h,
// shared with the observation terms
AS_NZ_FN float command_heading_w(const float (&q)[4]) {
  float fwd[3];
  base_forward(q, fwd);
  return as_atan2f(fwd[1], fwd[0]);
}

// math.py:96-117 wrap_to_pi; torch's % is fmodf and a shift into the divisor's sign
AS_NZ_FN float command_wrap_to_pi(float a) {
  float m = fmodf(a + kCommandPi, kCommandTwoPi);
  if (m != 0.0f && m < 0.0f) m = m + kCommandTwoPi;
  return (m == 0.0f && a > 0.0f) ? kCommandPi : m - kCommandPi;
}

// _update_metrics
AS_NZ_FN void command_update_metrics(const as_command_term_t& c, CommandState& s, const float (&q)[4],
                                     const float (&lin)[3], const float (&ang)[3]) {
  float lin_b[3], ang_b[3];
  base_rotate_inverse(q, lin, lin_b);
  base_rotate_inverse(q, ang, ang_b);
  const float dx = s.vel[0] - lin_b[0], dy = s.vel[1] - lin_b[1];
  // torch.norm over the two components accumulates acc = fma(x, x, acc) from 0: dx dx rounded, then one fused step
  s.metrics[kCmdErrXY] = s.metrics[kCmdErrXY] + sqrtf(fmaf(dy, dy, dx * dx)) / c.max_command_step;
  s.metrics[kCmdErrYaw] = s.metrics[kCmdErrYaw] + fabsf(s.vel[2] - ang_b[2]) / c.max_command_step;
}

// _update_command of both terms
AS_NZ_FN void command_update(const as_command_term_t& c, CommandState& s, const float (&q)[4]) {
  if (c.kind == AS_COMMAND_UNIFORM && c.heading && s.flag[kCmdHeading]) {
    const float e = command_wrap_to_pi(s.heading_target - command_heading_w(q));
    const float v = c.stiffness * e;
    s.vel[2] = fminf(fmaxf(v, c.clip_lo), c.clip_hi);
  }
  if (s.flag[kCmdStanding]) s.vel[0] = s.vel[1] = s.vel[2] = 0.0f;
  if (c.kind == AS_COMMAND_NORMAL)
    AS_CMD_UNROLL
    for (int k = 0; k < 3; ++k)
      if (s.flag[kCmdZeroX + k]) s.vel[k] = 0.0f;
}

// One env's step of one term on values held by the caller.  reset: the step reset this env; compute: run
// CommandTerm.compute (false: the reset-only entry).  draws(tag, d) fills the kCommandDraws draws of a phase and
// is called only for a phase that resamples.  Returns a bit per resample: 1 the reset's, 2 the compute's.
template <typename Draws>
AS_NZ_FN int command_term_step(const as_command_term_t& c, CommandState& s, float (&last_metrics)[kCommandMetricRows],
                               bool reset, bool compute, float dt, const float (&q)[4], const float (&lin)[3],
                               const float (&ang)[3], Draws&& draws) {
  int resampled = 0;
  float d[kCommandDraws];
  if (reset) {
    command_reset_head(s, last_metrics);
    draws(kCommandResetTag, d);
    command_resample(c, s, d);
    resampled |= 1;
  }
  if (compute) {
    command_update_metrics(c, s, q, lin, ang);
    s.time_left = s.time_left - dt;
    if (s.time_left <= 0.0f) {
      draws(kCommandComputeTag, d);
      command_resample(c, s, d);
      resampled |= 2;
    }
    command_update(c, s, q);
  }
  return resampled;
}

}  // namespace as
