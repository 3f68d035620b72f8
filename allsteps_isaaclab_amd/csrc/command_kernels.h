// command_kernels.h -- k_commands_step / k_commands_reset, the opt-in command manager of cfg.commands
// (as_commands_step / as_commands_reset).  Semantics, formulas, draw layout and stream: allsteps_commands.h.
// Neither kernel is part of as_step: the env launches k_commands_step after it (and before k_events_interval,
// the reference's order) when its cfg names commands, so the default step keeps its launches.  No host sync, no
// atomics, no LDS, no scratch.
#pragma once

#include <hip/hip_runtime.h>

#include "allsteps_commands.h"
#include "allsteps_kernels.h"

namespace as {

// One thread per env, envs along the lanes: every buffer is field-major / env-minor, so a wave's access to a row
// is one contiguous run.  The terms are looped in the thread in cfg order; an env's rows are read and written by
// its own thread only: no hazard between threads, no second launch.  The term descriptors are read from device
// memory (the same address in every lane), so a descriptor rewritten by set_term_cfg or a range edit takes effect
// in a graph that is already captured.  The root pose and velocities are read once and serve every term.
constexpr int kCommandThreads = 256;

struct CommandRows {
  size_t vel, heading, flags, time_left, counter, metrics;
};

__device__ __forceinline__ CommandRows command_rows(int k, size_t n, size_t i) {
  const size_t K = (size_t)k;
  return {K * 3 * n + i, K * n + i, K * kCommandFlagRows * n + i, K * n + i, K * n + i,
          K * kCommandMetricRows * n + i};
}

__device__ __forceinline__ void command_load(const CommandsArgs& P, const CommandRows& r, size_t n, CommandState& s) {
#pragma unroll
  for (int a = 0; a < 3; ++a) s.vel[a] = P.vel[r.vel + (size_t)a * n];
  s.heading_target = P.heading_target[r.heading];
#pragma unroll
  for (int a = 0; a < kCommandFlagRows; ++a) s.flag[a] = P.flags[r.flags + (size_t)a * n] != 0;
  s.time_left = P.time_left[r.time_left];
  s.counter = P.counter[r.counter];
#pragma unroll
  for (int a = 0; a < kCommandMetricRows; ++a) s.metrics[a] = P.metrics[r.metrics + (size_t)a * n];
}

// what a resample changes is stored only when one happened; last_metrics only for an env that was reset
__device__ __forceinline__ void command_store(const CommandsArgs& P, const CommandRows& r, size_t n,
                                              const CommandState& s, const float (&last)[kCommandMetricRows],
                                              int resampled) {
#pragma unroll
  for (int a = 0; a < 3; ++a) P.vel[r.vel + (size_t)a * n] = s.vel[a];
#pragma unroll
  for (int a = 0; a < kCommandMetricRows; ++a) P.metrics[r.metrics + (size_t)a * n] = s.metrics[a];
  P.time_left[r.time_left] = s.time_left;
  if (resampled) {
    P.heading_target[r.heading] = s.heading_target;
#pragma unroll
    for (int a = 0; a < kCommandFlagRows; ++a) P.flags[r.flags + (size_t)a * n] = s.flag[a] ? (uint8_t)1 : (uint8_t)0;
    P.counter[r.counter] = s.counter;
  }
  if ((resampled & 1) && P.last_metrics) {
#pragma unroll
    for (int a = 0; a < kCommandMetricRows; ++a) P.last_metrics[r.metrics + (size_t)a * n] = last[a];
  }
}

// kStep: the reset phase for the envs of reset | reset2, then compute for every env.  !kStep: the reset phase
// alone for the envs of `reset` (null: every env).
template <bool kStep>
__device__ __forceinline__ void commands_env(const CommandsArgs& P) {
  const int64_t e = (int64_t)blockIdx.x * kCommandThreads + threadIdx.x;
  if (e >= P.n) return;
  const size_t n = (size_t)P.n, i = (size_t)e;
  const uint32_t t = P.t[i];
  const uint32_t env = (uint32_t)(P.env_offset + e);
  bool reset;
  if (kStep)
    reset = (P.reset && P.reset[i]) || (P.reset2 && P.reset2[i]);
  else
    reset = !P.reset || P.reset[i];
  float q[4] = {1.f, 0.f, 0.f, 0.f}, lin[3] = {0.f, 0.f, 0.f}, ang[3] = {0.f, 0.f, 0.f};
  if (kStep) {
#pragma unroll
    for (int a = 0; a < 4; ++a) q[a] = P.root_quat[(size_t)a * n + i];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      lin[a] = P.root_lin[(size_t)a * n + i];
      ang[a] = P.root_ang[(size_t)a * n + i];
    }
  }
  if (kStep || reset) {
    for (int k = 0; k < P.num_terms; ++k) {
      const as_command_term_t c = P.terms[k];
      const CommandRows r = command_rows(k, n, i);
      CommandState s;
      command_load(P, r, n, s);
      float last[kCommandMetricRows] = {0.f, 0.f};
      // (inlined at both of its call sites: otherwise the draws would be handed over through scratch memory)
      auto draws = [&](uint32_t tag, float (&d)[kCommandDraws]) __attribute__((always_inline)) {
        if (P.draws) {
          const size_t phase = kStep && tag == kCommandComputeTag ? 1 : 0;
          const size_t base = ((phase * (size_t)P.num_terms + (size_t)k) * kCommandDraws) * n + i;
#pragma unroll
          for (int a = 0; a < kCommandDraws; ++a) d[a] = P.draws[base + (size_t)a * n];
        } else {
          command_draws(c, P.seed, env, t, k, tag, d);
        }
      };
      const int resampled = command_term_step(c, s, last, reset, kStep, P.dt, q, lin, ang, draws);
      command_store(P, r, n, s, last, resampled);
    }
  }
  P.t[i] = t + 1u;
}

__global__ __launch_bounds__(kCommandThreads) void k_commands_step(CommandsArgs P) { commands_env<true>(P); }

__global__ __launch_bounds__(kCommandThreads) void k_commands_reset(CommandsArgs P) { commands_env<false>(P); }

}  // namespace as
