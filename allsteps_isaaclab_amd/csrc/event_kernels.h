// event_kernels.h -- k_events_interval / k_events_init, the opt-in interval events of cfg.events
// (as_events_interval / as_events_init).  Semantics, formulas and stream layout: allsteps_events.h.  Neither
// kernel is part of as_step: the env launches k_events_interval after it when its cfg names events, so the
// default step keeps its launches.  No host sync, no atomics, no LDS.
#pragma once

#include <hip/hip_runtime.h>

#include "allsteps_events.h"
#include "allsteps_kernels.h"

namespace as {

// One thread per env, envs along the lanes: every buffer is field-major / env-minor (root_lin [3][n],
// root_ang [3][n], time_left [terms][n], fired [terms][n], t [n], injected draws [terms][n] and
// [terms][6][n]), so a wave's access to a row is one contiguous run.  The terms are looped in the thread in cfg
// order on the velocity held in registers -- term k reads what term k - 1 left -- and an env's timers, counter
// and velocity are read and written by its own thread only: no hazard between threads, no second launch.  The
// term descriptors are read from device memory (the same address in every lane), so a descriptor rewritten by
// set_term_cfg takes effect in a graph that is already captured.
constexpr int kEventThreads = 256;

__global__ __launch_bounds__(kEventThreads) void k_events_interval(EventsArgs P) {
  const int64_t e = (int64_t)blockIdx.x * kEventThreads + threadIdx.x;
  if (e >= P.n) return;
  const size_t n = (size_t)P.n, i = (size_t)e;
  const uint32_t t = P.t[i];
  const uint32_t env = (uint32_t)(P.env_offset + e);
  float v[6];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    v[k] = P.root_lin[(size_t)k * n + i];
    v[3 + k] = P.root_ang[(size_t)k * n + i];
  }
  bool pushed = false;
  for (int k = 0; k < P.num_terms; ++k) {
    const as_event_term_t c = P.terms[k];
    const size_t ki = (size_t)k * n + i;
    float tl = P.time_left[ki];
    bool fire = event_tick(&tl, P.dt);
    if (fire) {
      float u6[6];
      const float iu = P.interval_draws ? P.interval_draws[ki] : event_interval_draw(P.seed, env, t, k);
      if (P.push_draws) {
#pragma unroll
        for (int a = 0; a < 6; ++a) u6[a] = P.push_draws[((size_t)k * 6 + (size_t)a) * n + i];
      } else {
        event_push_draws(P.seed, env, t, k, u6);
      }
      tl = event_sample(iu, c.interval_w, c.interval_lo);
#pragma unroll
      for (int a = 0; a < 6; ++a) v[a] = event_push(v[a], u6[a], c.vel_w[a], c.vel_lo[a]);
      pushed = true;
    }
    P.time_left[ki] = tl;
    if (P.fired) P.fired[ki] = fire ? (uint8_t)1 : (uint8_t)0;
  }
  if (pushed) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      P.root_lin[(size_t)k * n + i] = v[k];
      P.root_ang[(size_t)k * n + i] = v[3 + k];
    }
  }
  P.t[i] = t + 1u;
}

// The initial timers (event_manager.py:383-385): one interval draw per (term, env) at t = 0, then t = 1
__global__ __launch_bounds__(kEventThreads) void k_events_init(EventsArgs P) {
  const int64_t e = (int64_t)blockIdx.x * kEventThreads + threadIdx.x;
  if (e >= P.n) return;
  const size_t n = (size_t)P.n, i = (size_t)e;
  const uint32_t env = (uint32_t)(P.env_offset + e);
  for (int k = 0; k < P.num_terms; ++k) {
    const as_event_term_t c = P.terms[k];
    const size_t ki = (size_t)k * n + i;
    const float iu = P.interval_draws ? P.interval_draws[ki] : event_interval_draw(P.seed, env, 0u, k);
    P.time_left[ki] = event_sample(iu, c.interval_w, c.interval_lo);
  }
  P.t[i] = 1u;
}

}  // namespace as
