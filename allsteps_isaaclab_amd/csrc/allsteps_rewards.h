// allsteps_rewards.h -- the reward manager's terms (cfg.rewards): the term values, the weighted sum, the episodic
// sums and the reset rule.
//
// The reference's RewardManager.compute(dt) (managers/reward_manager.py:128-157) evaluates the terms in cfg order;
// per term, skipped when its weight is exactly 0:
//     value = (f weight) dt;   reward += value;   episode_sums[k] += value;   step_reward[k] = value / dt
// with weight and dt as float32 (torch takes a Python scalar at the tensor's type), every operation rounded on its
// own (the library is built with -ffp-contract=off).  reward starts at +0; a skipped term adds +0, which changes no
// bit of a sum that started at +0.  RewardManager.reset(env_ids) (:100-126) zeroes the episodic sums of the envs
// that are done; here the sums are first copied to last_episode_sums, the form a captured step serves.
//
// The term functions f (envs/mdp/rewards.py and the velocity task's mdp/rewards.py), by as_reward_term_t.kind; ids /
// a / b are the term's row of the index table, p0 / p1 its constants, all formed by the host (envs/rewards.py):
//   IS_ALIVE / IS_TERMINATED    1 - terminated / terminated
//   LIN_VEL_Z_L2                v[2] v[2],            v = quat_rotate_inverse(root_quat, root_lin)
//   ANG_VEL_XY_L2               w[0] w[0] + w[1] w[1], w = quat_rotate_inverse(root_quat, root_ang)
//   FLAT_ORIENTATION_L2         g[0] g[0] + g[1] g[1], g = quat_rotate_inverse(root_quat, (0, 0, -1))
//   BASE_HEIGHT_L2              d d,                  d = root_pos[2] - p0
//   JOINT_VEL_L1 / _L2          sum |qd[id]| / sum qd[id]^2
//   JOINT_DEVIATION_L1          sum |q[id] - a|
//   JOINT_POS_LIMITS            sum (-min(q[id] - a, 0) + max(q[id] - b, 0))    torch's clip: a NaN passes
//   JOINT_ACC_L2                sum x x,              x = (qd[id] - qd_prev[id]) / sim_dt
//   ACTION_L2 / ACTION_RATE_L2  sum u u / sum (u - prev) (u - prev), u the action, clamped where the env clamps
//   UNDESIRED_CONTACTS          the number of bodies with m > p0, as a float; m = the maximum over the history slots
//                               of |F|, F = net / sim_dt per component, |F| = sqrtf(fmaf(z, z, fmaf(y, y, x x)))
//                               (torch.norm accumulates with a fused multiply-add, as allsteps_commands.h found); the
//                               maximum passes a NaN on, as torch.max does
//   CONTACT_FORCES              sum max(m - p0, 0)                              a NaN passes
//   FEET_AIR_TIME               (sum (last_air - p0) first) gate;  first = (current_contact > 0) (current_contact <
//                               p1) as 0 / 1, p1 = float32(step_dt + 1e-8);  gate = |cmd_xy| > 0.1f as 0 / 1,
//                               |cmd_xy| = sqrtf(fmaf(y, y, x x)); the products are float products (inf 0 = NaN)
//   FEET_AIR_TIME_BIPED         min over the ids of (single ? (contact > 0 ? contact : air) : 0), single: exactly one
//                               id has contact > 0; then min(., p0), then the gate; minimum and clamp pass a NaN on
//   TRACK_LIN_VEL_XY_EXP        as_expf(-(dx dx + dy dy) / p0), d = cmd_xy - v_xy, p0 = float32(std^2)
//   TRACK_ANG_VEL_Z_EXP         as_expf(-(d d) / p0), d = cmd_yaw - w[2]
//   TRACK_ANG_VEL_Z_WORLD_EXP   the same on root_ang[2]
//   TRACK_LIN_VEL_XY_YAW_EXP    TRACK_LIN_VEL_XY_EXP with v = quat_rotate_inverse(yaw_quat(root_quat), root_lin);
//                               yaw_quat (math.py:522-542): yaw = as_atan2f(2 (w z + x y), 1 - 2 (y y + z z)),
//                               (c, 0, 0, s) = as_sincosf(yaw / 2), divided by max(sqrtf(fmaf(s, s, c c)), 1e-9):
//                               atan2, sin and cos are the library's (include/as_detmath.h), not torch's bit for bit
// Reductions over the ids run in ascending table order from +0, each operation rounded on its own: a decision of
// this project (torch's CPU sum has an ISA-dependent association that cannot be restated).  The sum carries a
// compensation term (Kahan: y = v - c; t = acc + y; c = (t - acc) - y, c = 0 once t is not finite, so inf and NaN
// behave as in the plain sum): where every partial sum is exact it is the plain sum bit for bit, and elsewhere its
// error stays near one ulp however many addends there are -- the plain sequential sum of 21 squares was measured at 3
// times the error of torch's tree-shaped device sum.  exp is as_expf
// (include/as_detmath.h, <= 2 ulp): the one operation that is not torch's bit for bit.
//
// Plain C++ with no HIP dependency: tests/rewards_check.cpp runs all of it on the host.
#pragma once

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/allsteps.h"
#include "../../include/as_detmath.h"
#include "allsteps_base_frame.h"
#include "allsteps_noise.h"

namespace as {

// rows of the index table: table [AS_REW_TABLE_ROWS][AS_MAX_REW_TERMS][AS_MAX_REW_IDS] 32-bit words
enum { kRewTabId = 0, kRewTabA = 1, kRewTabB = 2 };
// the timer rows of as_contact_timers
enum { kRewTimerCurAir = 0, kRewTimerLastAir = 1, kRewTimerCurContact = 2 };

AS_NZ_FN size_t rew_table_at(int row, int term, int i) {
  return ((size_t)row * AS_MAX_REW_TERMS + (size_t)term) * AS_MAX_REW_IDS + (size_t)i;
}

// One env's window onto the sources.  A source that is not there, or a row outside it, reads as 0.
struct RewardEnv {
  const as_reward_sources_t* s;
  size_t n, e;

  AS_NZ_FN float row(const float* p, int rows, int r) const {
    return (p && r >= 0 && r < rows) ? p[(size_t)r * n + e] : 0.0f;
  }
  AS_NZ_FN float root_pos(int r) const { return row(s->root_pos, 3, r); }
  AS_NZ_FN float root_lin(int r) const { return row(s->root_lin, 3, r); }
  AS_NZ_FN float root_ang(int r) const { return row(s->root_ang, 3, r); }
  AS_NZ_FN void quat(float (&q)[4]) const {
    AS_BF_UNROLL
    for (int k = 0; k < 4; ++k) q[k] = row(s->root_quat, 4, k);
  }
  AS_NZ_FN float q(int r) const { return row(s->q, s->joint_rows, r); }
  AS_NZ_FN float qd(int r) const { return row(s->qd, s->joint_rows, r); }
  AS_NZ_FN float qd_prev(int r) const { return row(s->qd_prev, s->qd_prev_rows, r); }
  AS_NZ_FN float cmd(int r) const { return row(s->commands, s->command_rows, r); }
  AS_NZ_FN float net(int slot, int body, int c) const {
    if (body < 0 || body >= s->bodies) return 0.0f;
    return row(s->net, s->depth * s->bodies * 3, (slot * s->bodies + body) * 3 + c);
  }
  AS_NZ_FN float timer(int t, int body) const {
    if (body < 0 || body >= s->timer_bodies) return 0.0f;
    return row(s->timers, 4 * s->timer_bodies, t * s->timer_bodies + body);
  }
  AS_NZ_FN bool terminated() const { return s->terminated && s->terminated[e] != 0; }
};

// the env's action column j as the terms read it
AS_NZ_FN float rew_action_value(float x, int clamp) {
  if (!clamp) return x;
  const float y = x < -1.0f ? -1.0f : x;
  return y > 1.0f ? 1.0f : y;
}
AS_NZ_FN float rew_action(const RewardEnv& E, int j) {
  const as_reward_sources_t& s = *E.s;
  if (!s.actions || j < 0 || j >= s.action_cols) return 0.0f;
  return rew_action_value(s.actions[E.e * (size_t)s.action_cols + (size_t)j], s.clamp_actions);
}

// acc += v with the compensation c (see above)
AS_NZ_FN void rew_add(float& acc, float& c, float v) {
  const float y = v - c;
  const float t = acc + y;
  c = (t - acc) - y;
  if (!(fabsf(t) <= 3.402823466e+38f)) c = 0.0f;
  acc = t;
}

// max(|F|) over the history slots of one body; torch.max passes a NaN on
AS_NZ_FN float rew_contact_max(const RewardEnv& E, int body) {
  const float dt = E.s->sim_dt;
  float m = 0.0f;
  for (int d = 0; d < E.s->depth; ++d) {
    const float x = E.net(d, body, 0) / dt, y = E.net(d, body, 1) / dt, z = E.net(d, body, 2) / dt;
    const float v = sqrtf(fmaf(z, z, fmaf(y, y, x * x)));
    if (d == 0 || (m == m && (v > m || v != v))) m = v;
  }
  return m;
}

// math.py:522-542 yaw_quat, normalize included
AS_NZ_FN void rew_yaw_quat(const float (&q)[4], float (&o)[4]) {
  const float qw = q[0], qx = q[1], qy = q[2], qz = q[3];
  const float yaw = as_atan2f(2.0f * (qw * qz + qx * qy), 1.0f - 2.0f * (qy * qy + qz * qz));
  float s, c;
  as_sincosf(yaw / 2.0f, &s, &c);
  const float nrm = fmaxf(sqrtf(fmaf(s, s, c * c)), 1e-9f);
  o[0] = c / nrm;
  o[1] = 0.0f / nrm;
  o[2] = 0.0f / nrm;
  o[3] = s / nrm;
}

// the command gate of the air-time terms: |cmd_xy| > 0.1 as 1 / 0
AS_NZ_FN float rew_command_gate(const RewardEnv& E, int cmd_row) {
  const float x = E.cmd(cmd_row), y = E.cmd(cmd_row + 1);
  return sqrtf(fmaf(y, y, x * x)) > 0.1f ? 1.0f : 0.0f;
}

// f of one term for one env.  ids / ca / cb: the term's rows of the index table.  prev: the env's prev_actions row
// (null reads as 0).
AS_NZ_FN float reward_term_value(const as_reward_term_t& T, const int32_t* ids, const float* ca, const float* cb,
                                 const RewardEnv& E, const float* prev) {
  const int K = T.num_ids < AS_MAX_REW_IDS ? T.num_ids : AS_MAX_REW_IDS;
  switch (T.kind) {
    case AS_REW_IS_ALIVE:
      return E.terminated() ? 0.0f : 1.0f;
    case AS_REW_IS_TERMINATED:
      return E.terminated() ? 1.0f : 0.0f;
    case AS_REW_LIN_VEL_Z_L2:
    case AS_REW_ANG_VEL_XY_L2:
    case AS_REW_FLAT_ORIENTATION_L2:
    case AS_REW_TRACK_LIN_VEL_XY_EXP:
    case AS_REW_TRACK_LIN_VEL_XY_YAW_EXP:
    case AS_REW_TRACK_ANG_VEL_Z_EXP: {
      float q[4], u[3] = {0.0f, 0.0f, -1.0f}, o[3];
      E.quat(q);
      if (T.kind == AS_REW_TRACK_LIN_VEL_XY_YAW_EXP) {
        float qy[4];
        rew_yaw_quat(q, qy);
        AS_BF_UNROLL
        for (int k = 0; k < 4; ++k) q[k] = qy[k];
      }
      const bool lin = T.kind == AS_REW_LIN_VEL_Z_L2 || T.kind == AS_REW_TRACK_LIN_VEL_XY_EXP ||
                       T.kind == AS_REW_TRACK_LIN_VEL_XY_YAW_EXP;
      if (T.kind != AS_REW_FLAT_ORIENTATION_L2) {
        AS_BF_UNROLL
        for (int k = 0; k < 3; ++k) u[k] = lin ? E.root_lin(k) : E.root_ang(k);
      }
      base_rotate_inverse(q, u, o);
      if (T.kind == AS_REW_LIN_VEL_Z_L2) return o[2] * o[2];
      if (T.kind == AS_REW_TRACK_LIN_VEL_XY_EXP || T.kind == AS_REW_TRACK_LIN_VEL_XY_YAW_EXP) {
        const float dx = E.cmd(T.cmd_row) - o[0], dy = E.cmd(T.cmd_row + 1) - o[1];
        return as_expf(-(dx * dx + dy * dy) / T.p0);
      }
      if (T.kind == AS_REW_TRACK_ANG_VEL_Z_EXP) {
        const float d = E.cmd(T.cmd_row + 2) - o[2];
        return as_expf(-(d * d) / T.p0);
      }
      return o[0] * o[0] + o[1] * o[1];
    }
    case AS_REW_TRACK_ANG_VEL_Z_WORLD_EXP: {
      const float d = E.cmd(T.cmd_row + 2) - E.root_ang(2);
      return as_expf(-(d * d) / T.p0);
    }
    case AS_REW_BASE_HEIGHT_L2: {
      const float d = E.root_pos(2) - T.p0;
      return d * d;
    }
    case AS_REW_JOINT_VEL_L1:
    case AS_REW_JOINT_VEL_L2:
    case AS_REW_JOINT_DEVIATION_L1:
    case AS_REW_JOINT_POS_LIMITS:
    case AS_REW_JOINT_ACC_L2: {
      float acc = 0.0f, comp = 0.0f;
      for (int i = 0; i < K; ++i) {
        const int id = ids[i];
        float v;
        if (T.kind == AS_REW_JOINT_VEL_L1) {
          v = fabsf(E.qd(id));
        } else if (T.kind == AS_REW_JOINT_VEL_L2) {
          const float x = E.qd(id);
          v = x * x;
        } else if (T.kind == AS_REW_JOINT_DEVIATION_L1) {
          v = fabsf(E.q(id) - ca[i]);
        } else if (T.kind == AS_REW_JOINT_POS_LIMITS) {
          const float x = E.q(id);
          const float lo = x - ca[i], hi = x - cb[i];
          const float below = lo != lo ? lo : (lo > 0.0f ? 0.0f : lo);
          const float above = hi != hi ? hi : (hi < 0.0f ? 0.0f : hi);
          v = -below + above;
        } else {
          const float x = (E.qd(id) - E.qd_prev(id)) / E.s->sim_dt;
          v = x * x;
        }
        rew_add(acc, comp, v);
      }
      return acc;
    }
    case AS_REW_ACTION_L2:
    case AS_REW_ACTION_RATE_L2: {
      float acc = 0.0f, comp = 0.0f;
      const int A = E.s->action_cols;
      for (int j = 0; j < A; ++j) {
        float u = rew_action(E, j);
        if (T.kind == AS_REW_ACTION_RATE_L2) u = u - (prev ? prev[j] : 0.0f);
        rew_add(acc, comp, u * u);
      }
      return acc;
    }
    case AS_REW_UNDESIRED_CONTACTS:
    case AS_REW_CONTACT_FORCES: {
      float acc = 0.0f, comp = 0.0f;
      int count = 0;
      for (int i = 0; i < K; ++i) {
        const float m = rew_contact_max(E, ids[i]);
        if (T.kind == AS_REW_UNDESIRED_CONTACTS) {
          count += m > T.p0 ? 1 : 0;
        } else {
          const float d = m - T.p0;
          rew_add(acc, comp, d != d ? d : (d < 0.0f ? 0.0f : d));
        }
      }
      return T.kind == AS_REW_UNDESIRED_CONTACTS ? (float)count : acc;
    }
    case AS_REW_FEET_AIR_TIME: {
      float acc = 0.0f, comp = 0.0f;
      for (int i = 0; i < K; ++i) {
        const float cc = E.timer(kRewTimerCurContact, ids[i]);
        const float first = (cc > 0.0f && cc < T.p1) ? 1.0f : 0.0f;
        rew_add(acc, comp, (E.timer(kRewTimerLastAir, ids[i]) - T.p0) * first);
      }
      return acc * rew_command_gate(E, T.cmd_row);
    }
    case AS_REW_FEET_AIR_TIME_BIPED: {
      int in_contact = 0;
      for (int i = 0; i < K; ++i) in_contact += E.timer(kRewTimerCurContact, ids[i]) > 0.0f ? 1 : 0;
      const bool single = in_contact == 1;
      float m = 0.0f;
      for (int i = 0; i < K; ++i) {
        const float cc = E.timer(kRewTimerCurContact, ids[i]);
        const float mode = cc > 0.0f ? cc : E.timer(kRewTimerCurAir, ids[i]);
        const float v = single ? mode : 0.0f;
        if (i == 0 || (m == m && (v < m || v != v))) m = v;
      }
      m = m > T.p0 ? T.p0 : m;
      return m * rew_command_gate(E, T.cmd_row);
    }
    default:
      return 0.0f;
  }
}

// One (term, env) item of a launch: the value, the episodic sum and the step reward.  A term of weight 0 is skipped:
// its rows keep their values and it adds +0 to the total.  Returns what the total adds.
AS_NZ_FN float reward_term_step(const as_reward_term_t& T, const int32_t* ids, const float* ca, const float* cb,
                                const RewardEnv& E, const float* prev, float dt, float* episode_sum,
                                float* step_reward) {
  if (T.weight == 0.0f) return 0.0f;
  const float value = (reward_term_value(T, ids, ca, cb, E, prev) * T.weight) * dt;
  *episode_sum = *episode_sum + value;
  *step_reward = value / dt;
  return value;
}

// One env's launch on host arrays -- what k_rewards_step does per env, in the same pieces.  table: the index table;
// reward [n], episode_sums / step_reward / last_episode_sums [num_terms][n], prev_actions [n][action_cols] (the last
// two may be null).
inline void rewards_env_step(const as_reward_term_t* terms, int num_terms, const uint32_t* table,
                             const as_reward_sources_t& S, size_t n, size_t e, bool done, float dt, float* reward,
                             float* episode_sums, float* step_reward, float* last_episode_sums,
                             float* prev_actions) {
  const RewardEnv E{&S, n, e};
  const float* prev = prev_actions ? prev_actions + e * (size_t)S.action_cols : nullptr;
  float total = 0.0f;
  for (int k = 0; k < num_terms; ++k) {
    const int32_t* ids = reinterpret_cast<const int32_t*>(table + rew_table_at(kRewTabId, k, 0));
    const float* ca = reinterpret_cast<const float*>(table + rew_table_at(kRewTabA, k, 0));
    const float* cb = reinterpret_cast<const float*>(table + rew_table_at(kRewTabB, k, 0));
    total = total + reward_term_step(terms[k], ids, ca, cb, E, prev, dt, &episode_sums[(size_t)k * n + e],
                                     &step_reward[(size_t)k * n + e]);
  }
  reward[e] = total;
  for (int k = 0; k < num_terms && done; ++k) {
    if (last_episode_sums) last_episode_sums[(size_t)k * n + e] = episode_sums[(size_t)k * n + e];
    episode_sums[(size_t)k * n + e] = 0.0f;
  }
  if (prev_actions && S.actions)
    for (int j = 0; j < S.action_cols; ++j)
      prev_actions[e * (size_t)S.action_cols + (size_t)j] = done ? 0.0f : rew_action(E, j);
}

}  // namespace as
