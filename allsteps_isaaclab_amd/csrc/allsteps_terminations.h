// allsteps_terminations.h -- the termination manager's terms (cfg.terminations): one term's flag for one env, the
// union into time_outs / terminated / dones, and what a done env leaves behind.
//
// The reference's TerminationManager.compute() (managers/termination_manager.py:151-174) clears both buffers and
// evaluates the terms in cfg order; per term
//     value = f(env);   (time_out ? truncated : terminated) |= value;   term_dones[k] = value
// and returns truncated | terminated.  The flags are booleans, so the order of the ORs changes nothing; it is kept
// anyway.  reset(env_ids) (:127-149) counts term_dones over env_ids; here the term flags of an env that is done (by
// the manager or by the step's own flags) are copied to last_episode_dones, the form a captured step serves.
//
// The term functions f (envs/mdp/terminations.py), by as_termination_term_t.kind; ids / a / b are the term's row of
// the index table, p0 / p1 / i0 its constants, all formed by the host (envs/terminations.py).  Every comparison is
// float32 against a float32 constant (torch takes a Python scalar at the tensor's type) and strict where the
// reference's is; a comparison with a NaN is false, as in torch:
//   TIME_OUT                     step_truncated | (ep_len >= i0), i0 = max_episode_length.  For an env the step
//                                reset in-kernel ep_len is already 0 and step_truncated carries what the reference
//                                computed before its reset
//   COMMAND_RESAMPLE             (time_left[row] <= p0) & (command_counter[row] == i0), p0 = float32(step_dt)
//   BAD_ORIENTATION              fabsf(term_acosf(-g[2])) > p0, g = quat_rotate_inverse(root_quat, (0, 0, -1))
//                                (allsteps_base_frame.h).  term_acosf(x) = as_atan2f(sqrtf((1 - x) (1 + x)), x): the
//                                library's atan2 (include/as_detmath.h), not torch's acos bit for bit; NaN for |x| > 1
//                                and for a NaN, as torch.acos -- -g[2] can round to just above 1, and the flag is then
//                                false, as in the reference
//   ROOT_HEIGHT_BELOW_MINIMUM    root_pos[2] < p0
//   JOINT_POS_OUT_OF_LIMIT       any q[id] > b[i]  or  any q[id] < a[i], a / b the soft limits of the selected joints
//                                (the reference's function indexes a 1-D tensor with [:, joint_ids] and cannot run;
//                                this is its documented meaning)
//   JOINT_POS_OUT_OF_MANUAL_LIMIT  any q[id] > p1  or  any q[id] < p0
//   JOINT_VEL_OUT_OF_MANUAL_LIMIT  any fabsf(qd[id]) > p0
//   ILLEGAL_CONTACT              any body id with m > p0; m = the maximum over the history slots of |F|, F = net /
//                                sim_dt per component, |F| = sqrtf(fmaf(z, z, fmaf(y, y, x x))) (torch.norm accumulates
//                                with a fused multiply-add: allsteps_rewards.h's contact terms); the maximum passes a
//                                NaN on, as torch.max does, and the comparison is then false
//
// Plain C++ with no HIP dependency: tests/terminations_check.cpp runs all of it on the host.
#pragma once

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/allsteps.h"
#include "../../include/as_detmath.h"
#include "allsteps_base_frame.h"
#include "allsteps_noise.h"

namespace as {

// rows of the index table: table [AS_TERMINATION_TABLE_ROWS][AS_MAX_TERMINATION_TERMS][AS_MAX_TERMINATION_IDS] words
enum { kTermTabId = 0, kTermTabA = 1, kTermTabB = 2 };

AS_NZ_FN size_t term_table_at(int row, int term, int i) {
  return ((size_t)row * AS_MAX_TERMINATION_TERMS + (size_t)term) * AS_MAX_TERMINATION_IDS + (size_t)i;
}

// acos on the library's atan2: NaN outside [-1, 1] and for a NaN
AS_NZ_FN float term_acosf(float x) {
  if (!(fabsf(x) <= 1.0f)) return __builtin_nanf("");
  return as_atan2f(sqrtf((1.0f - x) * (1.0f + x)), x);
}

// One env's window onto the sources.  A source that is not there, or a row outside it, reads as 0.
struct TerminationEnv {
  const as_termination_sources_t* s;
  size_t n, e;

  AS_NZ_FN float row(const float* p, int rows, int r) const {
    return (p && r >= 0 && r < rows) ? p[(size_t)r * n + e] : 0.0f;
  }
  AS_NZ_FN float root_pos(int r) const { return row(s->root_pos, 3, r); }
  AS_NZ_FN void quat(float (&q)[4]) const {
    AS_BF_UNROLL
    for (int k = 0; k < 4; ++k) q[k] = row(s->root_quat, 4, k);
  }
  AS_NZ_FN float q(int r) const { return row(s->q, s->joint_rows, r); }
  AS_NZ_FN float qd(int r) const { return row(s->qd, s->joint_rows, r); }
  AS_NZ_FN float time_left(int r) const { return row(s->time_left, s->command_terms, r); }
  AS_NZ_FN int32_t command_counter(int r) const {
    return (s->command_counter && r >= 0 && r < s->command_terms) ? s->command_counter[(size_t)r * n + e] : 0;
  }
  AS_NZ_FN float net(int slot, int body, int c) const {
    if (body < 0 || body >= s->bodies) return 0.0f;
    return row(s->net, s->depth * s->bodies * 3, (slot * s->bodies + body) * 3 + c);
  }
  AS_NZ_FN int32_t ep_len() const { return s->ep_len ? s->ep_len[e] : 0; }
  AS_NZ_FN bool step_terminated() const { return s->step_terminated && s->step_terminated[e] != 0; }
  AS_NZ_FN bool step_truncated() const { return s->step_truncated && s->step_truncated[e] != 0; }
};

// max(|F|) over the history slots of one body; torch.max passes a NaN on
AS_NZ_FN float term_contact_max(const TerminationEnv& E, int body) {
  const float dt = E.s->sim_dt;
  float m = 0.0f;
  for (int d = 0; d < E.s->depth; ++d) {
    const float x = E.net(d, body, 0) / dt, y = E.net(d, body, 1) / dt, z = E.net(d, body, 2) / dt;
    const float v = sqrtf(fmaf(z, z, fmaf(y, y, x * x)));
    if (d == 0 || (m == m && (v > m || v != v))) m = v;
  }
  return m;
}

// the angle BAD_ORIENTATION compares: |acos(-projected_gravity_b[2])|
AS_NZ_FN float term_orientation_angle(const TerminationEnv& E) {
  float q[4], o[3];
  const float u[3] = {0.0f, 0.0f, -1.0f};
  E.quat(q);
  base_rotate_inverse(q, u, o);
  return fabsf(term_acosf(-o[2]));
}

// f of one term for one env.  ids / ca / cb: the term's rows of the index table.
AS_NZ_FN bool termination_term_flag(const as_termination_term_t& T, const int32_t* ids, const float* ca,
                                    const float* cb, const TerminationEnv& E) {
  const int K = T.num_ids < AS_MAX_TERMINATION_IDS ? T.num_ids : AS_MAX_TERMINATION_IDS;
  switch (T.kind) {
    case AS_TERMINATION_TIME_OUT:
      return E.step_truncated() || E.ep_len() >= T.i0;
    case AS_TERMINATION_COMMAND_RESAMPLE:
      return E.time_left(T.row) <= T.p0 && E.command_counter(T.row) == T.i0;
    case AS_TERMINATION_BAD_ORIENTATION:
      return term_orientation_angle(E) > T.p0;
    case AS_TERMINATION_ROOT_HEIGHT_BELOW_MINIMUM:
      return E.root_pos(2) < T.p0;
    case AS_TERMINATION_JOINT_POS_OUT_OF_LIMIT:
    case AS_TERMINATION_JOINT_POS_OUT_OF_MANUAL_LIMIT:
    case AS_TERMINATION_JOINT_VEL_OUT_OF_MANUAL_LIMIT: {
      bool any = false;
      for (int i = 0; i < K; ++i) {
        if (T.kind == AS_TERMINATION_JOINT_POS_OUT_OF_LIMIT) {
          const float x = E.q(ids[i]);
          any = any || x > cb[i] || x < ca[i];
        } else if (T.kind == AS_TERMINATION_JOINT_POS_OUT_OF_MANUAL_LIMIT) {
          const float x = E.q(ids[i]);
          any = any || x > T.p1 || x < T.p0;
        } else {
          any = any || fabsf(E.qd(ids[i])) > T.p0;
        }
      }
      return any;
    }
    case AS_TERMINATION_ILLEGAL_CONTACT: {
      bool any = false;
      for (int i = 0; i < K; ++i) any = any || term_contact_max(E, ids[i]) > T.p0;
      return any;
    }
    default:
      return false;
  }
}

// The union of one env's term flags in cfg order; flags[k * stride] is term k's.
AS_NZ_FN void terminations_union(const as_termination_term_t* terms, int num_terms, const uint8_t* flags,
                                 size_t stride, bool* time_out, bool* terminated) {
  bool to = false, te = false;
  for (int k = 0; k < num_terms; ++k) {
    const bool f = flags[(size_t)k * stride] != 0;
    if (terms[k].time_out != 0) {
      to = to || f;
    } else {
      te = te || f;
    }
  }
  *time_out = to;
  *terminated = te;
}

// One env's launch on host arrays -- what k_terminations_step does per env, in the same pieces.  table: the index
// table; term_dones / last_episode_dones [num_terms][n], time_outs / terminated / dones / reset_request [n] (the
// last and last_episode_dones may be null).
inline void terminations_env_step(const as_termination_term_t* terms, int num_terms, const uint32_t* table,
                                  const as_termination_sources_t& S, size_t n, size_t e, uint8_t* term_dones,
                                  uint8_t* time_outs, uint8_t* terminated, uint8_t* dones,
                                  uint8_t* last_episode_dones, uint8_t* reset_request) {
  const TerminationEnv E{&S, n, e};
  for (int k = 0; k < num_terms; ++k) {
    const int32_t* ids = reinterpret_cast<const int32_t*>(table + term_table_at(kTermTabId, k, 0));
    const float* ca = reinterpret_cast<const float*>(table + term_table_at(kTermTabA, k, 0));
    const float* cb = reinterpret_cast<const float*>(table + term_table_at(kTermTabB, k, 0));
    term_dones[(size_t)k * n + e] = termination_term_flag(terms[k], ids, ca, cb, E) ? 1 : 0;
  }
  bool to, te;
  terminations_union(terms, num_terms, term_dones + e, n, &to, &te);
  time_outs[e] = to ? 1 : 0;
  terminated[e] = te ? 1 : 0;
  dones[e] = (to || te) ? 1 : 0;
  const bool stepped = E.step_terminated() || E.step_truncated();
  if (last_episode_dones && (to || te || stepped))
    for (int k = 0; k < num_terms; ++k) last_episode_dones[(size_t)k * n + e] = term_dones[(size_t)k * n + e];
  if (reset_request) reset_request[e] = ((to || te) && !stepped) ? 1 : 0;
}

}  // namespace as
