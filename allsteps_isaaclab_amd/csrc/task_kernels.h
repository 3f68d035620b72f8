// task_kernels.h -- the one-env-per-lane task kernels around k_step: k_obs (K2), k_stones and k_quad.
// They read and write the SoA state and k_step's side buffer directly; none of them uses EnvS.
#pragma once

#include <hip/hip_runtime.h>

#include "allsteps_device.h"
#include "allsteps_kernels.h"
#include "step_scratch.h"
#include "step_task.h"

namespace as {

// ------------------------------------------------------------------------------------------------
// K2: the launch-wide part of the observation step.  If any env reset this step (device counter
// written by k_step): the curriculum gate (allsteps_env.py:471-479, evaluated on the tick-#1 target
// indices) -- k_step has already applied the second tick.  If none did: restore the tick-#1 state
// and observation entries k_step saved in the side buffer.
__device__ void gen_stones(const as_task_t& T, int level, uint64_t seed, uint32_t env, uint32_t episode,
                           const float* draws, float* stones, int n, int e);

// The next k_step's placement (kMapEnvs), by one wave (t = lane): env chunk w's 64 envs ranked by their
// constraint rows in this launch (a bitonic sort of (rows, lane) keys across the wave, unique keys:
// deterministic), rank q -> pair q / 2, half q % 2 (rows is at most substeps x 30: 16 bits hold it).
__device__ __forceinline__ void build_wave_map(const uint32_t* side, int32_t* wave_map, int n, bool streamed, int w,
                                               int t) {
  static_assert(kMapEnvs == 64, "one wave per env chunk");
  const uint32_t rows = min(side[kSideCost * n + w * kMapEnvs + t], 0xFFFFu);
  uint32_t key = rows << 6 | (uint32_t)(63 - t);  // descending rows, ascending env on ties
#pragma unroll
  for (int k = 2; k <= 64; k <<= 1)
#pragma unroll
    for (int j = k >> 1; j > 0; j >>= 1) {
      const uint32_t o = (uint32_t)__shfl_xor((int)key, j);
      const bool desc = (t & k) == 0, first = (t & j) == 0;  // descending overall
      key = first == desc ? max(key, o) : min(key, o);
    }
  wave_map[EPB * wave_map_block(w, t >> 1, n, streamed) + (t & 1)] = w * kMapEnvs + 63 - (int)(key & 63u);
}

__global__ __launch_bounds__(64) void k_obs(ObsArgs P) {
  const Consts& K = *(const Consts*)(CK*)P.consts;
  const as_task_t& T = K.task;
  const int n = P.n;
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  const int any_reset = P.counters[0];
  if (P.wave_map) build_wave_map(P.side, P.wave_map, n, P.map_streamed != 0, blockIdx.x, threadIdx.x);
  if (blockIdx.x == 0) {
    // the gate's inputs in one memory round trip: lane i < kCntSlots reads partial sum i, lane
    // kCntSlots the curriculum level (all issued before any store: the stores below may alias them)
    const int t = threadIdx.x;
    int v = 0;
    if (t < kCntSlots) v = P.counters[kCntStride * (1 + t)];
    else if (t == kCntSlots) v = P.st.curriculum[0];
    const int c = __shfl(v, kCntSlots);
    int part = t < kCntSlots ? v : 0;
#pragma unroll
    for (int off = kCntSlots / 2; off > 0; off >>= 1) part += __shfl_xor(part, off);
    const int sum = __builtin_amdgcn_readfirstlane(part);  // lanes 0..15 hold the total (exact integers)
    if (t == 0) {
      P.counters[1] = sum;
      // (regen below recomputes this gate per thread from the bank, race-free)
      if (any_reset && (float)sum / (float)n > (float)T.curriculum_threshold)
        P.st.curriculum[0] = min(c + 1, T.max_curriculum);
    }
  }
  // the next launch's bank (this launch reads the other one)
  for (int k = e; k < kCntBank; k += gridDim.x * blockDim.x) P.next_counters[k] = 0;
  if (any_reset && T.regen_footsteps && e < n && P.side[kSideRegen * n + e]) {
    int sum = 0;
    for (int i = 0; i < kCntSlots; ++i) sum += P.counters[kCntStride * (1 + i)];
    const int c0 = P.counters[kCntLevel];
    const int level = (float)sum / (float)n > (float)T.curriculum_threshold ? min(c0 + 1, T.max_curriculum) : c0;
    gen_stones(T, level, P.seed, (uint32_t)(P.env_offset + e), P.st.episode[e], nullptr, P.st.stones, n, e);
  }
  if (any_reset) return;
  if (e >= n) return;
  const as_state_t& st = P.st;
  const uint32_t* sd = P.side;
  st.idx[e] = (int)sd[e];
  st.prev[e] = (int)sd[n + e];
  st.next[e] = (int)sd[2 * n + e];
  st.count[e] = (int)sd[3 * n + e];
  st.swing[e] = (int)sd[4 * n + e];
  st.pot[e] = __uint_as_float(sd[5 * n + e]);
  st.old_pot[e] = __uint_as_float(sd[6 * n + e]);
  st.foot_contact[e] = __uint_as_float(sd[7 * n + e]);
  st.foot_contact[n + e] = __uint_as_float(sd[8 * n + e]);
  float* o = P.obs + (size_t)e * AS_OBS_DIM;
  for (int k = 0; k < kSideObs; ++k) o[48 + k] = __uint_as_float(sd[(kSideState + k) * n + e]);
}

// ------------------------------------------------------------------------------------------------
// allsteps_env.py:125-174 _generate_foot_steps_allsteps (+ env origin = 0)
__device__ float lerp_t(float a, float b, float w) {  // torch.lerp (ATen Lerp.h)
  return fabsf(w) < 0.5f ? a + w * (b - a) : b - (b - a) * (1.0f - w);
}

// one env's course at `level`: draws[3][n][N] if given, else Philox (seed, env, episode, k, "Ston")
__device__ void gen_stones(const as_task_t& T, int level, uint64_t seed, uint32_t env, uint32_t episode,
                           const float* draws, float* stones, int n, int e) {
  const int N = T.num_steps, maxc = T.max_curriculum;
  const int c = min(level, maxc);
  const float ratio = (float)c / (float)maxc;
  const float step = (0.9f - 0.75f) / (float)maxc;  // torch.linspace(0.75, 0.9, 10)[c]
  const float dist_hi = c < (maxc + 1) / 2 ? 0.75f + step * (float)c : 0.9f - step * (float)(maxc - c);
  const float d2r = 0.01745329251994329577f;
  const float yaw_lo = (-20.0f * ratio) * d2r, yaw_hi = (20.0f * ratio) * d2r;
  const float p_lo = (-30.0f * ratio) * d2r + 1.57079632679489661923f;
  const float p_hi = (30.0f * ratio) * d2r + 1.57079632679489661923f;
  float x = 0.f, y = 0.f, z = 0.f, phi = 0.f;
  for (int k = 0; k < N; ++k) {
    float w[3];
    if (draws) {
      for (int j = 0; j < 3; ++j) w[j] = draws[((size_t)j * n + e) * N + k];
    } else {
      float blk[4];
      philox_block(seed, env, episode, (uint32_t)k, kStonesTag, blk);
      w[0] = blk[0]; w[1] = blk[1]; w[2] = blk[2];
    }
    float dr = lerp_t(0.75f, dist_hi, w[0]);
    float dph = lerp_t(yaw_lo, yaw_hi, w[1]);
    float dth = lerp_t(p_lo, p_hi, w[2]);
    if (k == 0) { dr = 0.f; dph = 0.f; dth = 1.57079632679489661923f; }
    if (k == 1 || k == 2) { dr = 0.75f; dph = 0.f; dth = 1.57079632679489661923f; }
    phi += dph;
    float st_, ct_, sp, cp;
    as_sincosf(dth, &st_, &ct_);
    as_sincosf(phi, &sp, &cp);
    x += dr * st_ * cp;
    y += dr * st_ * sp;
    z += dr * ct_;
    stones[(k * 3 + 0) * n + e] = x;
    stones[(k * 3 + 1) * n + e] = y;
    stones[(k * 3 + 2) * n + e] = z;
  }
}

__global__ __launch_bounds__(256) void k_stones(StonesArgs P) {
  const as_task_t& T = ((const Consts*)(CK*)P.consts)->task;
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= P.n) return;
  gen_stones(T, P.level, P.seed, (uint32_t)(P.env_offset + e), 0u, P.draws, P.stones, P.n, e);
}

// ------------------------------------------------------------------------------------------------
// k_quad: the BASELINE C5 task epilogue (include/allsteps.h as_quad_task_t), one env per lane, after
// the physics substeps of k_step<18> (AS_ACT_DC_MOTOR); oracle/quad.c or_quad_post_physics is its
// serial restatement.  Coalesced SoA loads / stores (64-thread workgroups, like k_obs).
constexpr uint32_t kQuadTag = 0x51756164u;  // "Quad": reset-draw stream of the quadruped task

// k_quad: 64 envs per 256-thread workgroup.  The four feet's tips (FK of a 3-link chain each) run one
// thread per (env, foot) -- as one thread per env they were 11 % of the C5 step, a quarter of the
// SIMDs busy -- with the model tables they walk staged in LDS; the task logic then runs one thread
// per env.  Phases: (1) tips of the stepped state; (2) target ticks, rewards, dones, the reset of done
// envs (its joint angles also to LDS); (3) tips of the reset pose for the reset envs; (4) their
// potential, the state and the observation.  Per element the operations are as_link_point's
// (include/as_detmath.h, shared with oracle/quad.c) in the same order.
constexpr int kQuadEnvs = 64;
struct QuadSmem {
  int32_t parent[AS_MAX_LINKS], link_dof[AS_MAX_LINKS];
  float off_pos[AS_MAX_LINKS][3], off_quat[AS_MAX_LINKS][4], axis[AS_MAX_LINKS][3], anchor[AS_MAX_LINKS][3];
  int32_t foot_link[4];
  float foot_p1[4][3];
  float tip[kQuadEnvs][4][3];
  float root[kQuadEnvs][7];   // reset envs: the stand pose (position, quaternion)
  float qres[kQuadEnvs][AS_ACT_DIM];
  int32_t reset[kQuadEnvs];
  float obs[kQuadEnvs][AS_QUAD_OBS_DIM + 1];  // observation rows, written out coalesced (+1: banks)
};

// The mode is a compile-time parameter.  k_quad<false> is the step (or, with P.reset_all, the reset of every
// env) and never reads `mask`; its instruction stream is that of the kernel without the parameter.
// k_quad<true> is the masked reset (as_quad_reset_mask): the reset_all path for the envs whose mask byte
// ([n] uint8) is set and nothing at all for the others -- an unmasked env is not live (no load, no store;
// tail lanes do not read the mask), phase 3 skips it and the write-out copies only the reset envs' rows.
// It leaves the wave map alone: only k_step writes the cost rows the map is ranked by, so a rebuild here
// would reproduce the map that stands.
template <bool kMasked>
__global__ __launch_bounds__(4 * kQuadEnvs) void k_quad(QuadArgs P, const uint8_t* mask) {
  const Consts& K = *(const Consts*)(CK*)P.consts;
  const as_model_t& m = K.model;
  const as_quad_task_t& Q = K.quad;
  __shared__ QuadSmem qs;
  const int tid = threadIdx.x;
  const int n = P.n, nh = m.num_hinges, N = K.task.num_steps;
  const as_state_t& st = P.st;
  static_assert(kQuadEnvs == kMapEnvs, "a workgroup's envs are one placement chunk");
  if (!kMasked && P.wave_map && tid < kMapEnvs)
    build_wave_map(P.side, P.wave_map, n, P.map_streamed != 0, blockIdx.x, tid);  // (wave 0)
  // ---- the model tables of the feet's chains, once per workgroup
  if (tid == 0) as_link_dof_map(m.cfg_dof_link, nh, AS_MAX_LINKS, qs.link_dof);
  if (tid < AS_MAX_LINKS) {
    const int i = tid;
    qs.parent[i] = m.parent[i];
    for (int k = 0; k < 3; ++k) {
      qs.off_pos[i][k] = m.offset_pos[i][k];
      qs.axis[i][k] = m.axis[i][k];
      qs.anchor[i][k] = m.anchor[i][k];
    }
    for (int k = 0; k < 4; ++k) qs.off_quat[i][k] = m.offset_quat[i][k];
  }
  if (tid < 4) {  // sensor foot f's geom: its link and capsule end p1
    int g = 0;
    for (int j = 0; j < m.num_geoms; ++j)
      if (m.geom_foot[j] == tid) { g = j; break; }
    qs.foot_link[tid] = m.geom_link[g];
    for (int k = 0; k < 3; ++k) qs.foot_p1[tid][k] = m.geom_p1[g][k];
  }
  __syncthreads();
  // foot f's tip from the joint-angle column q_col[k * stride] and the root pose
  auto tip_of = [&](int f, const float* q_col, int stride, const float* rp, const float* rq, float* tip) {
    as_link_point(qs.parent, qs.link_dof, &qs.off_pos[0][0], &qs.off_quat[0][0], &qs.axis[0][0],
                  &qs.anchor[0][0], q_col, stride, qs.foot_link[f], rp, rq, qs.foot_p1[f], tip);
  };
  // ---- (1) tips of the stepped state, thread = (env, foot)
  {
    const int le = tid >> 2, f = tid & 3, e = blockIdx.x * kQuadEnvs + le;
    if (!(kMasked || P.reset_all) && e < n) {
      float rp[3], rq[4];
      for (int k = 0; k < 3; ++k) rp[k] = st.root_pos[k * n + e];
      for (int k = 0; k < 4; ++k) rq[k] = st.root_quat[k * n + e];
      tip_of(f, st.q + e, n, rp, rq, qs.tip[le][f]);
    }
  }
  __syncthreads();
  // ---- (2) task logic, thread = env
  const int le = tid, e = blockIdx.x * kQuadEnvs + le;
  bool live = tid < kQuadEnvs && e < n;
  if (kMasked) live = live && mask[e] != 0;
  auto stone = [&](int k, int c) { return st.stones[(3 * k + c) * n + e]; };
  // xy distance of foot f's tip to the aim point on stone k
  auto aim_dist = [&](int f, int k, const float* tip) {
    const float fx = tip[0] - stone(k, 0), fy = tip[1] - (stone(k, 1) + Q.foot_offset_y[f]);
    return sqrtf(fx * fx + fy * fy);
  };
  float rp[3], rq[4], lin[3], ang[3], a[AS_ACT_DIM], q[AS_ACT_DIM], qd[AS_ACT_DIM];
  int idx = 0, ep_len = 0, t[4], c[4];
  uint32_t episode = 0u, mk[4];
  float pot = 0.f, old_pot = 0.f;
  bool was_reset = false;
  if (live) {
    for (int k = 0; k < 3; ++k) {
      rp[k] = st.root_pos[k * n + e];
      lin[k] = st.root_lin[k * n + e];
      ang[k] = st.root_ang[k * n + e];
    }
    for (int k = 0; k < 4; ++k) rq[k] = st.root_quat[k * n + e];
    for (int k = 0; k < nh; ++k) {
      const float x = (kMasked || P.reset_all) ? 0.f : P.actions[(size_t)e * nh + k];
      a[k] = fminf(fmaxf(x, -1.f), 1.f);
    }
    idx = st.idx[e];
    ep_len = st.ep_len[e];
    for (int f = 0; f < 4; ++f) {
      t[f] = st.feet[f * n + e];
      c[f] = st.feet[(4 + f) * n + e];
    }
    episode = st.episode[e];
    mk[0] = st.contact_mask[e];
    mk[1] = st.contact_mask[n + e];
    mk[2] = st.contact_mask_hind[e];
    mk[3] = st.contact_mask_hind[n + e];
    pot = st.pot[e];
    old_pot = st.old_pot[e];
    bool term = false, trunc = false;
    if (!(kMasked || P.reset_all)) {
      ep_len += 1;
      // target tick per foot (allsteps_env.py:418-440) and the step reward of a fresh reach (:377-380)
      float step_hit = 0.f, fsum = 0.f;
      for (int f = 0; f < 4; ++f) {
        const float* tip = qs.tip[le][f];
        const float d = aim_dist(f, t[f], tip);
        const bool reached = ((mk[f] >> t[f]) & 1u) && d < Q.step_radius;
        if (reached) c[f] += 1;
        if (c[f] >= Q.stop_frames) {
          c[f] = 0;
          t[f] = min(t[f] + 1, N - 1);
        }
        if (reached && c[f] == 1 && t[f] < N - 1) step_hit += Q.step_reward * as_expf(-d / Q.step_sigma);
        fsum += aim_dist(f, t[f], tip);  // to the (updated) target: the potential
      }
      idx = min(t[0], t[1]);
      old_pot = pot;
      const float dx = stone(idx, 0) - rp[0], dy = stone(idx, 1) - rp[1];
      const float bd = sqrtf(dx * dx + dy * dy);
      pot = -(bd + Q.foot_progress * fsum) / Q.step_dt;
      const float down[3] = {0.f, 0.f, -1.f};
      float gb[3];
      quat_rotate_inverse(rq, down, gb);
      term = gb[2] > -Q.up_z_min || rp[2] < stone(idx, 2) + Q.min_height;
      trunc = ep_len >= Q.max_episode_length;
      float a2 = 0.f, en = 0.f;
      for (int k = 0; k < nh; ++k) {
        a2 += a[k] * a[k];
        en += fabsf(st.qd[k * n + e] * a[k]);
      }
      const float bonus = idx == N - 1 && bd < Q.bonus_radius ? Q.target_bonus : 0.f;
      const float progress = pot - old_pot;
      P.reward[e] = term ? Q.death
                         : (((Q.alive + progress) - Q.energy_cost * en) - Q.action_cost * sqrtf(a2)) + step_hit + bonus;
      P.terminated[e] = term;
      P.truncated[e] = trunc;
    }
    for (int k = 0; k < nh; ++k) {
      q[k] = st.q[k * n + e];
      qd[k] = st.qd[k * n + e];
    }
    was_reset = kMasked || P.reset_all || term || trunc;
    if (was_reset) {
      // the stand pose over stones 0 (hind feet) and 1 (front feet), joints + U(-1, 1) * noise
      float blk[4];
      for (int k = 0; k < nh; ++k) {
        if ((k & 3) == 0) philox_block(P.seed, (uint32_t)(P.env_offset + e), episode, (uint32_t)(k >> 2), kQuadTag, blk);
        q[k] = K.act.default_q[k] + Q.joint_noise * (2.f * blk[k & 3] - 1.f);
        qd[k] = 0.f;
        st.q[k * n + e] = q[k];
        st.qd[k * n + e] = 0.f;
        qs.qres[le][k] = q[k];
      }
      episode += 1u;
      rp[0] = 0.5f * (stone(0, 0) + stone(1, 0));
      rp[1] = 0.5f * (stone(0, 1) + stone(1, 1));
      rp[2] = fmaxf(stone(0, 2), stone(1, 2)) + K.sim.stone_half[2] + Q.stand_height;
      rq[0] = 1.f; rq[1] = rq[2] = rq[3] = 0.f;
      for (int k = 0; k < 3; ++k) {
        lin[k] = ang[k] = 0.f;
        st.root_pos[k * n + e] = rp[k];
        st.root_lin[k * n + e] = 0.f;
        st.root_ang[k * n + e] = 0.f;
        qs.root[le][k] = rp[k];
      }
      for (int k = 0; k < 4; ++k) {
        st.root_quat[k * n + e] = rq[k];
        qs.root[le][3 + k] = rq[k];
      }
    }
  }
  if (tid < kQuadEnvs) qs.reset[tid] = was_reset;
  __syncthreads();
  // ---- (3) tips of the reset pose (joint angles from LDS), thread = (env, foot)
  {
    const int le3 = tid >> 2, f = tid & 3;
    if (qs.reset[le3]) tip_of(f, qs.qres[le3], 1, &qs.root[le3][0], &qs.root[le3][3], qs.tip[le3][f]);
  }
  __syncthreads();
  // ---- (4) the reset envs' targets and potential; the state and the observation, thread = env
  if (live) {
    if (was_reset) {
      ep_len = 0;
      float fsum = 0.f;
      for (int f = 0; f < 4; ++f) {
        t[f] = min(f < 2 ? 2 : 1, N - 1);
        c[f] = 0;
        fsum += aim_dist(f, t[f], qs.tip[le][f]);
      }
      idx = min(t[0], t[1]);
      const float dx = stone(idx, 0) - rp[0], dy = stone(idx, 1) - rp[1];
      pot = -(sqrtf(dx * dx + dy * dy) + Q.foot_progress * fsum) / Q.step_dt;
      old_pot = pot;
      for (int k = 0; k < 4; ++k) mk[k] = 0u;
      st.contact_mask[e] = 0u;
      st.contact_mask[n + e] = 0u;
      st.contact_mask_hind[e] = 0u;
      st.contact_mask_hind[n + e] = 0u;
      // the contact report follows the masks: no contacts in any stored substep of a reset env
      if (P.rep)
        for (int k = 0; k < P.rep->depth; ++k) P.rep->count[report_count_index(k, e, n)] = 0;
    }
    st.idx[e] = idx;
    for (int f = 0; f < 4; ++f) {
      st.feet[f * n + e] = t[f];
      st.feet[(4 + f) * n + e] = c[f];
    }
    st.ep_len[e] = ep_len;
    st.episode[e] = episode;
    st.pot[e] = pot;
    st.old_pot[e] = old_pot;
    // observation [64]: lin / ang velocity (body), projected gravity, each foot's aim point and stone
    // idx + 1 relative to the root (body), each foot on its target stone, q - default, qd, actions --
    // staged in LDS, then the block's rows (contiguous in memory) written by all 256 threads
    float* o = qs.obs[le];
    float v[3];
    quat_rotate_inverse(rq, lin, v);
    o[0] = v[0]; o[1] = v[1]; o[2] = v[2];
    quat_rotate_inverse(rq, ang, v);
    o[3] = v[0]; o[4] = v[1]; o[5] = v[2];
    const float down[3] = {0.f, 0.f, -1.f};
    quat_rotate_inverse(rq, down, v);
    o[6] = v[0]; o[7] = v[1]; o[8] = v[2];
    for (int f = 0; f < 5; ++f) {
      const int k = f < 4 ? t[f] : min(idx + 1, N - 1);
      const float oy = f < 4 ? Q.foot_offset_y[f] : 0.f;
      const float d[3] = {stone(k, 0) - rp[0], (stone(k, 1) + oy) - rp[1], stone(k, 2) - rp[2]};
      quat_rotate_inverse(rq, d, v);
      o[9 + 3 * f] = v[0]; o[10 + 3 * f] = v[1]; o[11 + 3 * f] = v[2];
    }
    for (int f = 0; f < 4; ++f) o[24 + f] = (mk[f] >> t[f]) & 1u ? 1.f : 0.f;
    for (int k = 0; k < nh; ++k) {
      o[28 + k] = q[k] - K.act.default_q[k];
      o[28 + nh + k] = qd[k];
      o[28 + 2 * nh + k] = was_reset ? 0.f : a[k];  // _reset_idx zeroes _actions (anymal_c_env.py:171-172)
    }
  }
  __syncthreads();
  const int e0 = blockIdx.x * kQuadEnvs, rows = min(kQuadEnvs, n - e0);
  float* ob = P.obs + (size_t)e0 * AS_QUAD_OBS_DIM;
  for (int x = tid; x < rows * AS_QUAD_OBS_DIM; x += 4 * kQuadEnvs)
    if (!kMasked || qs.reset[x / AS_QUAD_OBS_DIM]) ob[x] = qs.obs[x / AS_QUAD_OBS_DIM][x % AS_QUAD_OBS_DIM];
}

}  // namespace as
