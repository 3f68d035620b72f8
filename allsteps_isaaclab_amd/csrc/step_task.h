// step_task.h -- what k_step's task epilogue shares with k_obs: the foot-state tick, targets and potentials of
// one env (compute_useful), the XCD-aware env placement, and the one-wave workgroup size.
// Touches no EnvS field: callers pass the state words in and out by reference.
#pragma once

#include <hip/hip_runtime.h>

#include "allsteps_device.h"
#include "allsteps_kernels.h"

namespace as {

// ------------------------------------------------------------------------------------------------
// task logic helpers (allsteps_env.py)

struct Useful {
  float h, roll, pitch, body_dist, dist_s;  // dist_s: swing-foot xy distance to the target
  int reached;
};

// allsteps_env.py:418-457 foot-state tick + 459-467 targets + 407-416 potentials (one env, serial).
// dist_s is the swing foot's distance with the swing leg AFTER the tick (allsteps_env.py:371).
// TaskT: as_task_t in the generic or the constant address space (k_step: uniform scalar loads)
// pose: u.h, u.roll and u.pitch are formed here; false (wave-uniform) when u already holds them for this
// root_quat and bp (k_step's second tick in a wave where no env reset).
template <class TaskT>
__device__ void compute_useful(TaskT& T, const float* root_pos, const float* root_quat, const float* bp,
                               const float* stones_env, int stride, uint32_t mask_r, uint32_t mask_l, int& idx,
                               int& prev, int& next, int& count, int& swing, float& pot, float& old_pot,
                               float* foot_contact, bool tick, Useful& u, bool pose = true) {
  const int N = T.num_steps;
  if (pose) {
    float lower = fminf(bp[8], bp[5]);   // minimum(left_z, right_z)
    u.h = bp[2] - lower;
    euler_rp_from_quat(root_quat, &u.roll, &u.pitch);
  }
  u.reached = 0;
  u.dist_s = 0.f;
  if (tick) {
    float cf0 = ((mask_r >> idx) & 1u) ? 1.f : 0.f;
    float cf1 = ((mask_l >> idx) & 1u) ? 1.f : 0.f;
    foot_contact[0] = cf0;
    foot_contact[1] = cf1;
    float tx = stones_env[(idx * 3 + 0) * stride], ty = stones_env[(idx * 3 + 1) * stride];
    float dx0 = bp[3] - tx, dy0 = bp[4] - ty, dx1 = bp[6] - tx, dy1 = bp[7] - ty;
    float d0 = sqrtf(dx0 * dx0 + dy0 * dy0), d1 = sqrtf(dx1 * dx1 + dy1 * dy1);
    float cfs = swing == 0 ? cf0 : cf1;
    float ds = swing == 0 ? d0 : d1;
    u.reached = (cfs > 0.f) && (ds < T.step_radius);
    if (u.reached) count += 1;
    if (count >= T.stop_frames) {
      swing ^= 1;
      int ni = min(max(idx + 1, 0), N - 1);
      idx = ni;
      prev = min(max(ni - 1, 0), N - 1);
      next = min(max(ni + 1, 0), N - 1);
      count = 0;
    }
    u.dist_s = swing == 0 ? d0 : d1;
  }
  float dx = stones_env[(next * 3 + 0) * stride] - root_pos[0];
  float dy = stones_env[(next * 3 + 1) * stride] - root_pos[1];
  u.body_dist = sqrtf(dx * dx + dy * dy);
  old_pot = pot;
  pot = -(u.body_dist) / T.step_dt;
}

// ------------------------------------------------------------------------------------------------
// XCD-aware env mapping.  Workgroup b is dispatched to XCD b % 8; a 128-B line of an SoA field
// holds 32 consecutive envs = 16 workgroups, which with the identity mapping would be split over all
// eight per-XCD L2s (each fetching and writing back the whole line for 16 useful bytes).  Give XCD x
// a contiguous range of env pairs instead (a bijection for any grid size; placement only affects
// speed, never results).
__device__ __forceinline__ int xcd_block(int b, int nb) {
  const int q = nb >> 3, r = nb & 7, x = b & 7, slot = b >> 3;
  return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + slot;
}

// k_step's workgroup is exactly ONE wave: its __syncthreads are LDS fences only, and the FK pointer
// jumping relies on a single wave's LDS operations completing in issue order (no barrier between
// rounds).  Launch and launch bound both use this constant; widening it must add those barriers.
constexpr int kStepThreads = 64;
static_assert(kStepThreads == 64, "k_step assumes a one-wave (wave64) workgroup: see the FK rounds");

}  // namespace as
