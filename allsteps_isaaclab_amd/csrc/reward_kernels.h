// reward_kernels.h -- k_rewards_step / k_rewards_reset, the opt-in reward manager of cfg.rewards (as_rewards_step /
// as_rewards_reset).  Semantics, formulas and rounding order: allsteps_rewards.h.  Neither kernel is part of
// as_step: the env launches k_rewards_step after it, the sensors, the commands and the events when its cfg names
// rewards, so the default step keeps its launches.  No host sync, no atomics, no scratch.
#pragma once

#include <hip/hip_runtime.h>

#include "allsteps_kernels.h"
#include "allsteps_rewards.h"

namespace as {

// Every source is field-major ([rows][n], envs contiguous), so lanes run along the envs and every load is one
// contiguous run of 64 envs.  A block takes kRewEnvs = 64 consecutive envs with kRewWaves = 8 waves (measured against
// 1, 2, 4 and 16: DESIGN.md §3 "Reward manager"); wave w takes the terms w, w + kRewWaves, ... one at a time, so the
// descriptor, the kind switch and the term's row of the index table are the same in every lane of a wave (the wave
// index goes through readfirstlane, which lets the compiler keep them in scalar registers and load them with scalar
// loads): no divergence across kinds.  The lane that made a term's value updates that term's episodic-sum and
// step-reward rows (and, for an env that is done, moves the sum to last_episode_sums) and leaves the value in LDS
// [term][env]; after a barrier wave 0's lane of each env adds the values in cfg order and stores the reward, and the
// block copies its contiguous run of the row-major actions into prev_actions (zero for an env that is done).  The
// action terms read prev_actions before the barrier, the copy writes it after.  The term descriptors and the index
// table are read from device memory, so a descriptor rewritten by set_term_cfg takes effect in a graph that is
// already captured.
// (AS_REW_WAVES: the waves per block of a variant build, for measurements; DESIGN.md §3 "Reward manager")
#ifndef AS_REW_WAVES
#define AS_REW_WAVES 8
#endif
constexpr int kRewEnvs = 64;
constexpr int kRewWaves = AS_REW_WAVES;
constexpr int kRewThreads = 64 * kRewWaves;

__global__ __launch_bounds__(kRewThreads) void k_rewards_step(RewardsArgs P) {
  __shared__ float s_val[AS_MAX_REW_TERMS * kRewEnvs];
  __shared__ uint8_t s_done[kRewEnvs];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int64_t e0 = (int64_t)blockIdx.x * kRewEnvs;
  const int64_t e = e0 + lane;
  const bool valid = e < P.n;
  const size_t n = (size_t)P.n, i = (size_t)(valid ? e : 0);
  const int T = P.num_terms < AS_MAX_REW_TERMS ? P.num_terms : AS_MAX_REW_TERMS;
  const bool done = valid && ((P.reset && P.reset[i]) || (P.reset2 && P.reset2[i]));
  if (wave == 0) s_done[lane] = done ? 1 : 0;
  const RewardEnv E{&P.src, n, i};
  const float* prev = P.prev_actions ? P.prev_actions + i * (size_t)P.src.action_cols : nullptr;
  const uint32_t* tab = reinterpret_cast<const uint32_t*>(P.table);
  for (int k = wave; k < T; k += kRewWaves) {
    const as_reward_term_t term = P.terms[k];
    float value = 0.0f;
    if (valid) {
      const size_t at = (size_t)k * n + i;
      float sum = P.episode_sums[at], step = 0.0f;
      const bool live = term.weight != 0.0f;
      value = reward_term_step(term, reinterpret_cast<const int32_t*>(tab + rew_table_at(kRewTabId, k, 0)),
                               P.table + rew_table_at(kRewTabA, k, 0), P.table + rew_table_at(kRewTabB, k, 0), E,
                               prev, P.dt, &sum, &step);
      if (live) P.step_reward[at] = step;
      if (done) {
        if (P.last_episode_sums) P.last_episode_sums[at] = sum;
        sum = 0.0f;
      }
      if (live || done) P.episode_sums[at] = sum;
    }
    s_val[k * kRewEnvs + lane] = value;
  }
  __syncthreads();
  if (wave == 0 && valid) {
    float total = 0.0f;
    for (int k = 0; k < T; ++k) total = total + s_val[k * kRewEnvs + lane];
    P.reward[i] = total;
  }
  if (P.prev_actions && P.src.actions) {
    const int A = P.src.action_cols;
    const int64_t left = (int64_t)P.n - e0;
    const int items = (int)(left < kRewEnvs ? left : kRewEnvs) * A;
    const size_t base = (size_t)e0 * (size_t)A;
    for (int it = threadIdx.x; it < items; it += kRewThreads)
      P.prev_actions[base + it] =
          s_done[it / A] ? 0.0f : rew_action_value(P.src.actions[base + it], P.src.clamp_actions);
  }
}

// RewardManager.reset(env_ids): the episodic sums and prev_actions of the masked envs (null: every env)
__global__ __launch_bounds__(kRewThreads) void k_rewards_reset(RewardsArgs P) {
  const int64_t e = (int64_t)blockIdx.x * kRewThreads + threadIdx.x;
  if (e >= P.n || (P.reset && !P.reset[e])) return;
  const size_t n = (size_t)P.n, i = (size_t)e;
  for (int k = 0; k < P.num_terms; ++k) P.episode_sums[(size_t)k * n + i] = 0.0f;
  if (P.prev_actions)
    for (int j = 0; j < P.src.action_cols; ++j) P.prev_actions[i * (size_t)P.src.action_cols + (size_t)j] = 0.0f;
}

}  // namespace as
