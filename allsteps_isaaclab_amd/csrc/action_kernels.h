// action_kernels.h -- k_actions_process and k_actions_reset, the opt-in action manager of cfg.actions
// (as_actions_step / as_actions_reset).  Semantics and the float32 operations: allsteps_actions.h.  The kernels are
// not part of as_step: the env launches k_actions_process before the step (after the action noise model) when its cfg
// names actions, and k_actions_reset directly after it on the step's own flags; the step reads the command buffer
// through StepArgs::cmd (as_set_joint_commands).  No host sync, no atomics, no LDS, no scratch.
#pragma once

#include <hip/hip_runtime.h>

#include "allsteps_actions.h"
#include "allsteps_kernels.h"

namespace as {

// One thread per (env, column), t = env * num_cols + column: input, action, prev_action, processed and prev_applied
// are env-major [n][num_cols] as the reference's tensors are, so every load and store of a wave is one contiguous
// run of 64 words; the command store scatters inside the env's own row of cmd (at most num_hinges words).  The
// column descriptors are read from device memory, so a descriptor the host rewrites takes effect in a graph that is
// already captured; the table is at most AS_ACT_DIM rows of 48 bytes and stays in cache.
// (AS_ACTION_WAVES: the waves per block of a variant build, for measurements; DESIGN.md §3 "Action manager")
#ifndef AS_ACTION_WAVES
#define AS_ACTION_WAVES 4
#endif
constexpr int kActionWaves = AS_ACTION_WAVES;
constexpr int kActionThreads = 64 * kActionWaves;

__global__ __launch_bounds__(kActionThreads) void k_actions_process(ActionsArgs P) {
  const int64_t t = (int64_t)blockIdx.x * kActionThreads + threadIdx.x;
  const int64_t total = (int64_t)P.n * P.num_cols;
  if (t >= total) return;
  const size_t e = (size_t)(t / P.num_cols);
  const int c = (int)(t - (int64_t)e * P.num_cols);
  const as_action_column_t C = P.cols[c];
  actions_process_one(C, (size_t)t, e, P.cmd_cols, P.input, P.action, P.prev_action, P.processed, P.prev_applied,
                      P.cmd);
}

__global__ __launch_bounds__(kActionThreads) void k_actions_reset(ActionsArgs P) {
  const int64_t t = (int64_t)blockIdx.x * kActionThreads + threadIdx.x;
  const int64_t total = (int64_t)P.n * P.num_cols;
  if (t >= total) return;
  const size_t e = (size_t)(t / P.num_cols);
  // the envs of mask | mask2 (the step's terminated and truncated flags); neither: every env
  if ((P.mask || P.mask2) && !((P.mask && P.mask[e] != 0) || (P.mask2 && P.mask2[e] != 0))) return;
  const int c = (int)(t - (int64_t)e * P.num_cols);
  const as_action_column_t C = P.cols[c];
  actions_reset_one(C, (size_t)t, e, (size_t)P.n, P.cmd_cols, P.q, P.action, P.prev_action, P.prev_applied);
}

}  // namespace as
