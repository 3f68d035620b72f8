// allsteps_events.h -- interval events (cfg.events): timers, fire test, resample, push and stream layout.
//
// The reference's DirectRLEnv.step applies the "interval" terms of cfg.events after _reset_idx and before
// _get_observations (direct_rl_env.py:370-372): EventManager.apply(mode="interval", dt=step_dt)
// (event_manager.py:200-225).  Per env, per term, per env step:
//     time_left -= dt                         dt = step_dt rounded to float32
//     fires where time_left < 1e-6            compared in float32
//     on firing: time_left = u w + lo         w = float32(double(hi) - double(lo)): two Python floats
//                term(env)                    in cfg order: term k reads the velocity term k - 1 left
// The one term served is push_by_setting_velocity (isaaclab/envs/mdp/events.py:681-706):
//     root_vel[c] += u_c w_c + lo_c           c = x y z roll pitch yaw; w_c = float32(hi_c) - float32(lo_c),
//                                             a float32 subtraction: the ranges pass through a tensor
// Every multiply and add is rounded on its own (the library is built with -ffp-contract=off), so the same
// draws give torch's bits.  The host forms lo / w / lo_c / w_c (envs/events.py); the kernels only read them.
//
// Draws: Philox4x32-10 keyed by the env's seed, counter (env_id_offset + e, t[e], block, tag) -- the reset
// and noise streams' layout with a per-env event counter t[e] of its own, advanced once per launch of
// k_events_interval (event_kernels.h).  The block carries the term:
//     interval resample of term k    tag "EvIv", block k, word 0
//     push of term k                 tag "EvPu", blocks 2k and 2k + 1, words x y z roll | pitch yaw
// The initial timers (event_manager.py:383-385) are the interval draw at t = 0; as_events_init then sets
// t = 1.  The global env id is in the counter, so shards equal the unsharded run.
//
// Plain C++ with no HIP dependency: tests/events_check.cpp runs all of it on the host.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "../../include/allsteps.h"
#include "allsteps_noise.h"

namespace as {

constexpr uint32_t kEventIntervalTag = 0x45764976u;  // "EvIv": interval resamples and the initial timers
constexpr uint32_t kEventPushTag = 0x45765075u;      // "EvPu": the six velocity draws of a push
constexpr float kEventFireEps = 1e-6f;               // event_manager.py:218, as float32

// time_left -= dt; the term fires where the new value is below 1e-6
AS_NZ_FN bool event_tick(float* time_left, float dt) {
  *time_left = *time_left - dt;
  return *time_left < kEventFireEps;
}

// rand * (hi - lo) + lo: the resampled interval, and one component of the velocity sample
AS_NZ_FN float event_sample(float u, float w, float lo) { return u * w + lo; }

// vel += sample
AS_NZ_FN float event_push(float v, float u, float w, float lo) { return v + event_sample(u, w, lo); }

// the interval stream's draw of term k: block k, word 0
AS_NZ_FN float event_interval_draw(uint64_t seed, uint32_t env, uint32_t t, int term) {
  float u4[4];
  noise_philox_block(seed, env, t, (uint32_t)term, kEventIntervalTag, u4);
  return u4[0];
}

// the push stream's six draws of term k: blocks 2k (x y z roll) and 2k + 1 (pitch yaw)
AS_NZ_FN void event_push_draws(uint64_t seed, uint32_t env, uint32_t t, int term, float* u6) {
  float a[4], b[4];
  noise_philox_block(seed, env, t, (uint32_t)(2 * term), kEventPushTag, a);
  noise_philox_block(seed, env, t, (uint32_t)(2 * term + 1), kEventPushTag, b);
  u6[0] = a[0]; u6[1] = a[1]; u6[2] = a[2]; u6[3] = a[3];
  u6[4] = b[0]; u6[5] = b[1];
}

// One env's step of one term on values held by the caller: returns whether it fired.  iv_u / push_u are read
// only when it does.
AS_NZ_FN bool event_term_step(const as_event_term_t& c, float dt, float* time_left, float* vel6, float iv_u,
                              const float* push_u6) {
  if (!event_tick(time_left, dt)) return false;
  *time_left = event_sample(iv_u, c.interval_w, c.interval_lo);
  for (int k = 0; k < 6; ++k) vel6[k] = event_push(vel6[k], push_u6[k], c.vel_w[k], c.vel_lo[k]);
  return true;
}

}  // namespace as
