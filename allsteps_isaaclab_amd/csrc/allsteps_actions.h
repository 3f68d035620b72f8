// allsteps_actions.h -- the action manager's joint terms (cfg.actions): one column of one env from the policy's
// action to the joint command, and what a reset leaves behind.
//
// The reference's ActionManager.process_action() (managers/action_manager.py) keeps prev_action <- action,
// action <- input, and hands each term its columns; a term keeps raw_actions <- its columns and forms
// processed_actions, which apply_action() passes to the asset as the joint target of every physics substep.  Here a
// column is one (term, joint) pair in cfg order; `joint` is its column of the command buffer (cfg dof order).
//
// The terms (envs/mdp/actions), by as_action_column_t.kind.  Every float32 operation is rounded on its own (the
// library is built without contraction) and runs in the reference's order; every constant is formed by the host
// (envs/actions.py) as torch forms it, a Python float against a float32 tensor being rounded to float32 first:
//   JOINT_POSITION / JOINT_EFFORT   p = clamp(raw * scale + offset, clip_lo, clip_hi)      (joint_actions.py:130-139)
//   POSITION_TO_LIMITS              p = clamp(raw * scale, clip_lo, clip_hi); with rescale
//                                   p = ((clamp(p, -1, 1) * (hi - lo)) * 0.5) + ((lo + hi) * 0.5), lo / hi the soft
//                                   joint position limits            (joint_actions_to_limits.py:112-132, math.py
//                                   unscale_transform)
//   EMA_POSITION_TO_LIMITS          the same p, then e = alpha * p; e += one_minus_alpha * prev_applied;
//                                   p = clamp(e, lo, hi); prev_applied = p               (:208-221)
// clip_lo / clip_hi are -inf / +inf for a column without a clip, and the clamp is then the identity.  clamp is
// torch.clamp: a NaN passes, otherwise min(max(x, lo), hi) with std::max / std::min's comparisons, which keep the
// sign of a zero that compares equal to a bound.
//
// reset (ActionManager.reset(env_ids), :reset of the terms): action, prev_action and raw_actions (the columns of
// action) are zeroed; an EMA column's prev_applied becomes the env's current joint position.  processed_actions and
// the command stay as they are, as in the reference.
//
// Plain C++ with no HIP dependency: tests/actions_check.cpp runs all of it on the host.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "../../include/allsteps.h"
#include "allsteps_noise.h"

namespace as {

// torch.clamp(x, lo, hi) for one float32
AS_NZ_FN float action_clamp(float x, float lo, float hi) {
  if (x != x) return x;
  const float m = x < lo ? lo : x;
  return hi < m ? hi : m;
}

// processed_actions of one column from its raw action; prev: the column's prev_applied (EMA only)
AS_NZ_FN float action_process(const as_action_column_t& C, float raw, float prev) {
  float p = raw * C.scale;
  if (C.kind == AS_ACTION_JOINT_POSITION || C.kind == AS_ACTION_JOINT_EFFORT) p = p + C.offset;
  p = action_clamp(p, C.clip_lo, C.clip_hi);
  if (C.kind == AS_ACTION_JOINT_POSITION || C.kind == AS_ACTION_JOINT_EFFORT) return p;
  if (C.rescale != 0) {
    const float x = action_clamp(p, -1.0f, 1.0f);
    const float off = (C.lim_lo + C.lim_hi) * 0.5f;
    p = ((x * (C.lim_hi - C.lim_lo)) * 0.5f) + off;
  }
  if (C.kind == AS_ACTION_EMA_POSITION_TO_LIMITS) {
    float e = C.alpha * p;
    e = e + C.one_minus_alpha * prev;
    p = action_clamp(e, C.lim_lo, C.lim_hi);
  }
  return p;
}

// One (env, column) of process_action on host arrays -- what k_actions_process does per thread.  input, action,
// prev_action, processed and prev_applied are [n][num_cols], cmd is [n][cmd_cols]; a column whose joint is outside
// the command buffer stores no command.
AS_NZ_FN void actions_process_one(const as_action_column_t& C, size_t at, size_t e, int32_t cmd_cols,
                                  const float* input, float* action, float* prev_action, float* processed,
                                  float* prev_applied, float* cmd) {
  const float raw = input[at];
  prev_action[at] = action[at];
  action[at] = raw;
  const float p = action_process(C, raw, prev_applied[at]);
  processed[at] = p;
  if (C.kind == AS_ACTION_EMA_POSITION_TO_LIMITS) prev_applied[at] = p;
  if (C.joint >= 0 && C.joint < cmd_cols) cmd[e * (size_t)cmd_cols + (size_t)C.joint] = p;
}

// One (env, column) of reset; q [q_rows][n] the joint positions, cfg dof order.
AS_NZ_FN void actions_reset_one(const as_action_column_t& C, size_t at, size_t e, size_t n, int32_t q_rows,
                                const float* q, float* action, float* prev_action, float* prev_applied) {
  action[at] = 0.0f;
  prev_action[at] = 0.0f;
  if (C.kind == AS_ACTION_EMA_POSITION_TO_LIMITS && C.joint >= 0 && C.joint < q_rows)
    prev_applied[at] = q[(size_t)C.joint * n + e];
}

}  // namespace as
