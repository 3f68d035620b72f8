// allsteps_kernels.hip -- MI355X (gfx950) step kernels for Allsteps-v0.
//
// k_step (K1): one env per 32-lane group (two envs per 64-lane wave, one wave per workgroup).
//   For each env: load the SoA state once, run `decimation` physics substeps, then the task
//   epilogue of DirectRLEnv.step (direct_rl_env.py:349-364): episode counter, foot-state tick #1,
//   targets, potentials, dones, rewards and -- for envs that are done -- the in-kernel reset
//   (allsteps_env.py:469-565) with Philox draws and an FK of the new pose.  The state is read and
//   written exactly once per env step.
//   One substep (oracle/physics.c is its serial restatement):
//     FK (level-synchronous, lanes = links) -> link inertias / motion subspaces -> RNEA bias and
//     composite inertias (lanes = links) -> joint-space inertia rows H_j (lane = dof j, from the
//     ancestor bitmasks) -> H^-1 by in-register Gauss-Jordan (one row per lane, pivot row broadcast
//     through LDS) -> u* = u + dt H^-1 (tau - C) -> stone contacts + joint-limit rows ->
//     W = H^-1 J^T (lane = dof, J and W columns in VGPRs) -> projected Gauss-Seidel on the impulses
//     with DPP cross-lane reductions -> semi-implicit integration.
// k_obs (K2): one env per lane.  If any env reset this step (device counter written by K1), the
//   second _compute_useful_values over ALL envs (allsteps_env.py:567: foot-state tick #2 with the
//   stale last-substep contacts, targets, potentials) and the curriculum gate
//   (allsteps_env.py:471-479); then the observation (allsteps_env.py:326-345).
// k_stones: _generate_foot_steps_allsteps (allsteps_env.py:125-174), one env per lane.
//
// This file is the one translation unit: k_step and the launchers.  Everything k_step calls is in the phase
// headers below, included in definition order (the order also fixes the order of the compiled listing):
//   step_scratch.h  LDS layout -> step_lanes.h  cross-lane primitives -> step_dynamics.h  FK, dynamics,
//   H^-1 sweep -> step_collide.h  contacts -> step_solve.h  rows, PGS, substep -> step_report.h  the opt-in
//   contact report's stores -> step_task.h  task helpers;
// after k_step: task_kernels.h (k_obs, k_stones, k_quad), body_state_kernel.h (k_body_state) and
// contact_forces_kernel.h (k_contact_forces), noise_kernels.h, event_kernels.h, contact_timer_kernels.h
// (k_contact_timers), ray_caster_kernels.h (k_ray_cast), imu_kernels.h (k_imu), ray_camera_kernels.h
// (k_ray_camera), frame_transformer_kernels.h (k_frame_transformer), command_kernels.h (k_commands_step,
// k_commands_reset), observation_kernels.h (k_observations, k_observations_reset), reward_kernels.h
// (k_rewards_step, k_rewards_reset), termination_kernels.h (k_terminations_step) and action_kernels.h
// (k_actions_process, k_actions_reset).
#include <hip/hip_runtime.h>

#include "../../include/allsteps.h"
#include "allsteps_device.h"
#include "allsteps_kernels.h"

#include "step_scratch.h"
#include "step_lanes.h"
#include "step_dynamics.h"
#include "step_collide.h"
#include "step_solve.h"
#include "step_report.h"
#include "step_task.h"

namespace as {

typedef const __attribute__((address_space(4))) StepArgs KArgs;  // the launch arguments in the kernarg segment

// The workgroup's LDS: the stamps' accumulators exist in the diagnostic twin alone.
template <bool kDiag>
struct StepLds {
  Smem sm;
};
template <>
struct StepLds<true> {
  Smem sm;
  unsigned long long stamp_acc[kNumStamps];
};

// The body of k_step (kDiag = false) and of its diagnostic twin k_step_diag (kDiag = true): the same code, with
// Stamp<kDiag> for the phase stamps.  kargs: where the calling kernel's StepArgs parameter lies in its kernarg
// segment (step_kargs below), handed in by the kernel, which alone knows its parameter list.
template <int NV, uint64_t SKIP, bool kDiag>
__device__ __forceinline__ void step_body(const StepArgs& P, KArgs* kargs) {
  __shared__ StepLds<kDiag> lds;
  Smem& sm = lds.sm;
  // model / plan constants stay in global memory (5.7 KB, L1/K$-resident): LDS is the occupancy
  // budget, see EnvS
  // The launch arguments that live across the substep loop (the constants pointer, n, the report pointer below)
  // are read through an opaque copy of the pointer to the arguments in the kernarg segment, a scalar load and
  // a register of its own each.  As parts of the wide scalar loads that fetch
  // the other arguments, a spill across the loop saved and restored the whole 4- or 16-register load for the
  // one pointer, inside the loop.
  KArgs* ka = kargs;
  asm volatile("" : "+s"(ka));
  CK* Kc = (CK*)ka->consts;
  const Consts& K = *(const Consts*)Kc;
  const int el = threadIdx.x >> 5, lane = threadIdx.x & 31;
  const int n = ka->n;
  EnvS& s = sm.env[el];
  const as_state_t& st = P.st;
  Stamp<kDiag> ts;
  if constexpr (kDiag) {
    ts.p = P.stamps;
    ts.acc = lds.stamp_acc;
    ts.t = 0ull;
  }
  ts.start();
  // ---- load, batch 1: everything whose address is known at launch start, issued together -- the env
  //      of this half, this lane's table row (allsteps_lane_table.h), the curriculum level and both
  //      curriculum tables (lane c < 10 reads entry c; the level then picks a lane, not an address)
  int e_raw = xcd_block(blockIdx.x, gridDim.x) * EPB + el;
  if (P.wave_map) e_raw = P.wave_map[EPB * blockIdx.x + el];
  const ConstV4* rowp = (const ConstV4*)&Kc->lane[lane];
  u32x4 rc[kLaneChunks];
#pragma unroll
  for (int k = 0; k < kLaneChunks; ++k) rc[k] = rowp[k];
  const int cur = *(const __attribute__((address_space(4))) int32_t*)st.curriculum;
  const float cur_gain = Kc->task.gain_curriculum[lane < 10 ? lane : 0];
  const float cur_term = Kc->task.term_curriculum[lane < 10 ? lane : 0];
  const bool valid = e_raw < n;
  const int e = valid ? e_raw : n - 1;
  // Under the wave map the second half of the grid holds the predicted-light waves, each the SIMD
  // partner of a heavy one.  The light wave starts with issue priority, until the first substep's row
  // count sets the rule below: with the heavy wave ahead from the first instruction the light partner
  // finished last (a wave's cycles grow more with its partner's rows than with its own, r06j), and
  // light-first for the opening phases only (not every substep's, nor the first two) measured best (r06k).
  if (P.wave_map && blockIdx.x >= (gridDim.x >> 1)) __builtin_amdgcn_s_setprio(1);
  const __attribute__((address_space(4))) as_model_t& m = Kc->model;
  const int nh = m.num_hinges;
  const __attribute__((address_space(4))) as_task_t& T = Kc->task;
  // ---- load, batch 2: every per-env word of the launch, the task epilogue's included, behind one
  //      wait.  The loads are unconditional at clamped rows (a lane past a field re-reads a row of the
  //      same field) so that no branch, with a wait of its own, separates them; lane t < kPkWords
  //      fetches epilogue word t.
  const int l3 = lane < 3 ? lane : 0, l4 = lane < 4 ? lane : 0, lh = lane < nh ? lane : 0;
  const int ns3 = 3 * T.num_steps;
  const int k0 = lane < ns3 ? lane : 0, k1 = lane + G < ns3 ? lane + G : 0;
  const float v_rp = st.root_pos[l3 * n + e], v_rl = st.root_lin[l3 * n + e], v_ra = st.root_ang[l3 * n + e];
  const float v_rq = st.root_quat[l4 * n + e];
  const float v_q = st.q[lh * n + e], v_qd = st.qd[lh * n + e];
  // (a reset launch has no actions: it reads q at the same offset, in bounds, and drops the value)
  const float* actp = P.mode != kModeReset ? P.actions : st.q;
  float v_a = actp[(size_t)e * nh + lh];
  if (P.mode == kModeReset) v_a = 0.f;
  // the opt-in joint commands (as_set_joint_commands; the host passes them to physics launches only): lane lh's
  // command, loaded unconditionally in this batch at a pointer that falls back to the actions', so no branch and
  // no wait of its own is added
  const float* cmdp = P.cmd ? P.cmd : actp;
  const float v_c = cmdp[(size_t)e * nh + lh];
  const float v_s0 = st.stones[k0 * n + e], v_s1 = st.stones[k1 * n + e];
  uint32_t mask[4] = {st.contact_mask[e], st.contact_mask[n + e], 0u, 0u};
  uint32_t v_pk;
  {
    const void* const fp[kPkBody] = {st.idx, st.prev, st.next, st.count, st.swing, st.ep_len,
                                     st.pot, st.old_pot, st.foot_contact, st.foot_contact, st.episode};
    const void* pp = fp[0];
#pragma unroll
    for (int k = 1; k < kPkBody; ++k) pp = lane == k ? fp[k] : pp;
    const bool body = lane >= kPkBody && lane < kPkWords;
    pp = body ? st.body_pos : pp;
    v_pk = ((StateWord*)pp)[lane == kPkFc1 ? n + e : (body ? (lane - kPkBody) * n + e : e)];
  }
  // the table row: tree plan (shared by both envs through LDS), joint, geom and H-row constants
  Topo tp0;
  tp0.lpath = rc[0].x; tp0.lsub = rc[0].y; tp0.dsub = rc[0].z; tp0.jump = rc[0].w;
  tp0.lo = __uint_as_float(rc[1].x); tp0.hi = __uint_as_float(rc[1].y); tp0.arm = __uint_as_float(rc[1].z);
  if (el == 0) sm.topo[lane] = tp0;
  const Topo& tp = sm.topo[lane];
  LinkC lc;
#pragma unroll
  for (int k = 0; k < 4; ++k) lc.oq[k] = __uint_as_float(rc[2][k]);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    lc.ax[k] = __uint_as_float(rc[3 + k / 4][k % 4]);
    lc.an[k] = __uint_as_float(rc[3 + (3 + k) / 4][(3 + k) % 4]);
    lc.op[k] = __uint_as_float(rc[3 + (6 + k) / 4][(6 + k) % 4]);
  }
  const float row_gear = __uint_as_float(rc[5].y), row_dq = __uint_as_float(rc[5].z);
  GeomC gc;
  gc.link = (int)rc[6].x; gc.type = (int)rc[6].y; gc.foot = (int)rc[6].z; gc.r = __uint_as_float(rc[6].w);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    gc.p0[k] = __uint_as_float(rc[7][k]);
    gc.p1[k] = __uint_as_float(rc[7 + (3 + k) / 4][(3 + k) % 4]);
  }
  gc.anc = rc[1].w;
  // opaque: the values are not rematerialised from memory inside the substep loop
  asm volatile("" : "+v"(gc.link), "+v"(gc.type), "+v"(gc.foot), "+v"(gc.r), "+v"(gc.anc));
  asm volatile("" : "+v"(gc.p0[0]), "+v"(gc.p0[1]), "+v"(gc.p0[2]), "+v"(gc.p1[0]), "+v"(gc.p1[1]), "+v"(gc.p1[2]));
  const float gain = readlane_f(cur_gain, cur);
  const float term_h = readlane_f(cur_term, cur);  // allsteps_env.py:401, for the epilogue
  if (lane < 3) {
    s.root_pos[lane] = v_rp;
    s.u[lane] = v_rl;
    s.u[3 + lane] = v_ra;
  }
  if (lane < 4) s.root_quat[lane] = v_rq;
  if (lane == 0) { s.ndrop = 0; s.nrows = 0; }
  if (lane < nh) {
    int i = (int)rc[9].w - 1;
    s.qi[i] = v_q;
    s.u[6 + i] = v_qd;
    float a = fminf(fmaxf(v_a, -1.f), 1.f);              // allsteps_env.py:267-268
    s.act[lane] = a;
    s.tau[i] = gain * row_gear * a;                      // allsteps_env.py:273
    s.qt[i] = Kc->act.action_scale * a + row_dq;         // AS_ACT_DC_MOTOR (anymal_c_env.py:73-74)
    if (P.cmd) {  // an action manager's command is the applied effort / the target itself: no gain, gear or clip
      s.tau[i] = v_c;
      s.qt[i] = v_c;
    }
  }
  if (lane < ns3) s.stones[lane] = v_s0;
  if (lane + G < ns3) s.stones[lane + G] = v_s1;
  if (lane < kPkWords) s.pk[lane] = v_pk;
  __syncthreads();
  ts.mark(kStLoad);
  const bool do_physics = P.mode == kModeStep || P.mode == kModePhysics;
  // ---- physics
  if (do_physics) {
    const int substeps = Kc->sim.substeps;  // (through the generic reference it was re-read every substep)
    const ReportDesc* rep = ka->rep;
    // (counted down: `left` substeps follow this one, which is also its slot in the contact report)
    for (int left = substeps - 1; left >= 0; --left) {
      // the opt-in contact report (step_report.h): a wave-uniform test of a launch argument per substep
      // (each test on an opaque copy of the pointer: no predicate of it is formed ahead of the loop and
      // held, spilled, across the substeps)
      const ReportDesc* rp = rep;
      asm volatile("" : "+s"(rp));
      if (rp && left == 0) report_store_qd(rp, n, Kc, s, lane, e, valid);
      substep<NV, SKIP>(K, sm, s, lane, tp, gc, lc, mask, ts);
      rp = rep;
      asm volatile("" : "+s"(rp));
      if (rp) report_store(rp, n, s, lane, e, valid, left);
    }
  }
  // The launch arguments again, through a second opaque copy of that pointer: everything after the
  // substeps reads its pointers and words of the launch by scalar loads here, instead of holding them in SGPRs
  // -- spilled, there are some 70 of them -- across the substep loop.
  KArgs* qa = kargs;
  asm volatile("" : "+s"(qa));
  KArgs& Q = *qa;
  const __attribute__((address_space(4))) as_state_t& sq = Q.st;
  // This lane's reset constants (joint `lane` in cfg order: its link and limits, the start pose plain and
  // mirrored), loaded ahead of the final FK so that their global loads (L2 round trips) run under it
  // instead of heading the reset (the memory clobber keeps them there, not sunk into the reset
  // branch).  The task's reward and the observation use the same link and limits.
  // (the two reset chunks of the table row, allsteps_lane_table.h: the mirror map is resolved there;
  // lanes past the hinges get link 1 and zeros.)  The optional reset draws are the only other global
  // loads after the substeps, issued here as well.
  // (through the generic pointer: loads from the constant address space are invariant, and the clobber
  // below would not hold them here)
  const u32x4* rowg = (const u32x4*)&K.lane[lane];
  const u32x4 rr8 = rowg[8], rr9 = rowg[9];
  const float rs_q = __uint_as_float(rr8.z), rs_qm = __uint_as_float(rr8.w), rs_sg = __uint_as_float(rr9.x);
  const float rs_lo = __uint_as_float(rr9.y), rs_hi = __uint_as_float(rr9.z);
  const int rs_li = (int)rr9.w;
  float rd_m = 0.f, rd_n = 0.f;  // mirror draw, this lane's joint-noise draw
  if (Q.reset_draws && Q.mode != kModePhysics) {
    rd_m = Q.reset_draws[(size_t)e * 22];
    rd_n = Q.reset_draws[(size_t)e * 22 + 1 + lh];
  }
  asm volatile("" ::: "memory");
  if (do_physics) {
    fk<false>(*Kc, s, lane, tp, lc, Kc->max_path);  // FK of the final pose for body_pos_w (articulation_data.py:439)
    if (lane == 0) { s.mask[0] = mask[0]; s.mask[1] = mask[1]; s.mask[2] = mask[2]; s.mask[3] = mask[3]; }
  }
  ts.mark(kStFKFinal);
  if (lane == 0 && !do_physics) { s.mask[0] = mask[0]; s.mask[1] = mask[1]; }
  __syncthreads();
  float bp[9];
  if (do_physics) {
    const int ls[3] = {m.torso_link, m.foot_link[0], m.foot_link[1]};
    for (int b = 0; b < 3; ++b)
      for (int k = 0; k < 3; ++k) bp[3 * b + k] = s.root_pos[k] + s.p[ls[b]][k];
  } else {
    for (int k = 0; k < 9; ++k) bp[k] = __uint_as_float(s.pk[kPkBody + k]);
  }
  // ---- task epilogue (direct_rl_env.py:349-364), on the scalars parked at launch start
  int idx = (int)s.pk[kPkIdx], prev = (int)s.pk[kPkPrev], next = (int)s.pk[kPkNext], count = (int)s.pk[kPkCount];
  int swing = (int)s.pk[kPkSwing], ep_len = (int)s.pk[kPkEpLen];
  float pot = __uint_as_float(s.pk[kPkPot]), old_pot = __uint_as_float(s.pk[kPkOldPot]);
  float fc[2] = {__uint_as_float(s.pk[kPkFc0]), __uint_as_float(s.pk[kPkFc1])};
  uint32_t episode = s.pk[kPkEpisode];
  bool done = false;
  Useful u{};  // tick #1's; its h / roll / pitch serve tick #2 where the pose cannot have changed (below)
  if (Q.mode == kModeStep || Q.mode == kModeTask) {
    ep_len += 1;                                         // direct_rl_env.py:351
    compute_useful(T, s.root_pos, s.root_quat, bp, s.stones, 1, s.mask[0], s.mask[1], idx, prev, next, count,
                   swing, pot, old_pot, fc, true, u);    // allsteps_env.py:397 tick #1
    // lane-parallel pieces of the reward: sum a^2, sum |qd a|, #(|q_scaled| > 0.99)
    float a2 = 0.f, en = 0.f;
    int atlim = 0;
    if (lane < nh) {
      const int li = rs_li;
      float a = s.act[lane];
      a2 = a * a;
      en = fabsf(s.u[6 + li - 1] * a);
      atlim = fabsf(scale_transform(s.qi[li - 1], rs_lo, rs_hi)) > 0.99f;
    }
    a2 = half_sum(a2);
    en = half_sum(en);
    uint64_t bl = __ballot(atlim != 0);
    int nlim = __popcll(bl >> (32 * el) & 0xffffffffull);
    const float* lv = s.u;
    float speed = sqrtf(lv[0] * lv[0] + lv[1] * lv[1] + lv[2] * lv[2]);
    bool time_out = ep_len >= T.max_episode_length - 1;  // allsteps_env.py:399
    bool fell = u.h < term_h;                             // :401
    bool so_fast = speed > 5.0f;                         // :402
    bool died = s.root_pos[2] < T.fall_abs;              // :403
    bool terminated = fell || so_fast || died;
    // allsteps_env.py:347-394
    float progress = pot - old_pot;
    bool roll_v = (u.roll > 0.4f) || (u.roll < -0.4f);
    bool pitch_v = (u.pitch > 0.4f) || (u.pitch < -0.2f);
    float roll_cost = roll_v ? fabsf(u.roll) : 0.f;
    float pitch_cost = pitch_v ? fabsf(u.pitch) : 0.f;
    float speed_cost = speed > 1.6f ? speed - 1.6f : 0.f;
    float action_cost = T.action * sqrtf(a2);
    float energy_cost = T.energy * en;
    float limit_cost = (float)nlim * T.joint_limit;
    bool cond = u.reached && count == 1 && idx < T.num_steps - 1;
    float step_rew = cond ? 50.0f * as_expf(-u.dist_s / 0.25f) : 0.f;  // shared deterministic exp
    bool bonus_c = idx == T.num_steps - 1 && u.body_dist < 0.15f;
    float total = T.alive + progress;
    total = total - roll_cost;
    total = total - pitch_cost;
    total = total - speed_cost;
    total = total - energy_cost;
    total = total - action_cost;
    total = total - limit_cost;
    total = total + step_rew;
    total = total + (bonus_c ? 10.0f : 0.f);
    float rew = terminated ? T.death : total;
    done = terminated || time_out;
    if (valid && lane == 0) {
      Q.reward[e] = rew;
      Q.terminated[e] = terminated ? 1 : 0;
      Q.truncated[e] = time_out ? 1 : 0;
    }
  } else if (Q.mode == kModeReset) {
    done = Q.reset_mask == nullptr || Q.reset_mask[e] != 0;
  }
  if (Q.mode != kModePhysics) {
    // curriculum mean over the tick-#1 indices and the any-reset flag: one atomic per wave into a
    // striped partial sum, the flag by plain store
    const int cidx = valid ? idx : 0;
    const bool vdone = valid && done;
    const int wsum = __builtin_amdgcn_readlane(cidx, 0) + __builtin_amdgcn_readlane(cidx, 32);
    const bool wdone = __any(vdone);
    // contacts the row budget cut in this launch (rare: one same-address atomic per wave that had any)
    const int ndr = valid ? s.ndrop : 0;
    const int wdrop = __builtin_amdgcn_readlane(ndr, 0) + __builtin_amdgcn_readlane(ndr, 32);
    if (threadIdx.x == 0) {
      atomicAdd(&Q.counters[kCntStride * (1 + (int)(blockIdx.x % kCntSlots))], wsum);
      if (wdrop) atomicAdd(&Q.counters[kCntDropped], wdrop);
      if (wdone) Q.counters[0] = 1;
      if (T.regen_footsteps) Q.counters[kCntLevel] = cur;  // same value from every wave
    }
  }
  ts.mark(kStTask);
  // ---- in-kernel reset (allsteps_env.py:481-565)
  const bool any_done = __any(done);  // wave-uniform: both envs of the wave enter the FK together
  // regen_footsteps: the over-half test on the PRE-reset target index (allsteps_env.py:497-500 as
  // intended); k_obs draws the new course once the launch-wide curriculum gate is known
  const bool regen = T.regen_footsteps && Q.mode != kModePhysics && done && idx > T.num_steps / 2;
  if (Q.mode != kModePhysics && any_done) {
    if (done) {
      float dm = rd_m, dn = rd_n;  // the caller's draws (loaded ahead of the final FK), or Philox
      if (!Q.reset_draws) {
        float blk[4];
        philox_block(Q.seed, (uint32_t)(Q.env_offset + e), episode, 0u, kResetTag, blk);
        dm = blk[0];
        if (lane < nh) {  // draw k = 1 + lane lives in block (1 + lane) / 4, slot (1 + lane) % 4
          const int k = 1 + lane;
          philox_block(Q.seed, (uint32_t)(Q.env_offset + e), episode, (uint32_t)(k >> 2), kResetTag, blk);
          const int sl = k & 3;
          dn = sl == 0 ? blk[0] : (sl == 1 ? blk[1] : (sl == 2 ? blk[2] : blk[3]));
        }
      }
      ep_len = 0;
      old_pot = 0.f; pot = 0.f; count = 0; swing = 0; idx = 1; prev = 0; next = 2;
      const bool mirror = dm > 0.5f;
      if (mirror) swing ^= 1;
      if (lane < nh) {
        // joint `lane` (cfg order): running-start pose, mirrored, noise, clip (allsteps_env.py:505-560)
        // (the mirror map, start pose and limits were loaded ahead: rs_*)
        const float sign = mirror ? rs_sg : 1.f;
        float jp = mirror ? rs_qm : rs_q;
        float jv = 0.f * sign;
        int li = rs_li;
        float x = jp + (dn * (T.noise_hi - T.noise_lo) + T.noise_lo);
        float sc = fminf(fmaxf(scale_transform(x, rs_lo, rs_hi), T.clip_lo), T.clip_hi);
        s.qi[li - 1] = unscale_transform(sc, rs_lo, rs_hi);
        s.u[6 + li - 1] = jv;
      }
      if (lane < 3) {
        const float ir[3] = {T.init_root[0], T.init_root[1], T.init_root[2]};  // uniform: scalar loads
        s.root_pos[lane] = lane == 0 ? ir[0] : (lane == 1 ? ir[1] : ir[2]);
        s.u[lane] = 0.f;
        s.u[3 + lane] = 0.f;
      }
      if (lane == 0) {
        float sg = mirror ? -1.f : 1.f;
        s.root_quat[0] = 1.f;
        s.root_quat[1] = 0.f * sg;
        s.root_quat[2] = 0.f * sg;
        s.root_quat[3] = 0.f * sg;
      }
      episode += 1u;
    }
    __syncthreads();
    fk<false>(*Kc, s, lane, tp, lc, Kc->max_path);  // body_pos of the reset pose (write_joint_state_to_sim invalidates FK)
    if (done) {
      const int ls[3] = {m.torso_link, m.foot_link[0], m.foot_link[1]};
      for (int b = 0; b < 3; ++b)
        for (int k = 0; k < 3; ++k) bp[3 * b + k] = s.root_pos[k] + s.p[ls[b]][k];
    }
  }
  __syncthreads();
  // ---- observation with a speculative second tick (allsteps_env.py:326-345, 567).  The reference
  //      re-runs _compute_useful_values for ALL envs when ANY env reset this step -- a launch-wide
  //      condition.  The tick is applied here as if some env reset (true at any realistic env
  //      count); the tick-#1 state and the tick-dependent observation entries (foot contact,
  //      targets) go to a side buffer, and k_obs restores them in a launch where no env reset.
  if (Q.obs) {
    int i2 = idx, p2 = prev, n2 = next, c2 = count, w2 = swing;
    float pot2 = pot, op2 = old_pot, fc2[2] = {fc[0], fc[1]};
    // h, roll and pitch depend on root_quat and bp alone, which only a reset changes between the ticks:
    // a wave without a done env (wave-uniform; 94 % of them) keeps tick #1's instead of a second atan2 /
    // asin / two rem2pi
    Useful u2 = u;
    compute_useful(T, s.root_pos, s.root_quat, bp, s.stones, 1, s.mask[0], s.mask[1], i2, p2, n2, c2, w2, pot2,
                   op2, fc2, true, u2, any_done || !(Q.mode == kModeStep || Q.mode == kModeTask));
    float* ob = s.x.obs;
    uint32_t* side = Q.side;
    if (lane == 0) {
      ob[0] = u2.h;
      ob[1] = u2.roll;
      ob[2] = u2.pitch;
      float vb[3];
      quat_rotate_inverse(s.root_quat, s.u, vb);
      ob[3] = vb[0]; ob[4] = vb[1]; ob[5] = vb[2];
      ob[48] = fc2[0];
      ob[49] = fc2[1];
    }
    if (lane < nh) {
      const int li = rs_li;
      ob[6 + lane] = scale_transform(s.qi[li - 1], rs_lo, rs_hi);
      ob[27 + lane] = fminf(fmaxf(s.u[6 + li - 1] * T.dof_vel_scale, -5.f), 5.f);
    }
    if (lane < 6) {  // lanes 0-2: targets after the second tick, lanes 3-5: after the first
      const int t = lane < 3 ? lane : lane - 3;
      const int ti = lane < 3 ? (t == 0 ? p2 : (t == 1 ? i2 : n2)) : (t == 0 ? prev : (t == 1 ? idx : next));
      const float tw[3] = {s.stones[3 * ti], s.stones[3 * ti + 1], s.stones[3 * ti + 2]};
      float o3[3];
      subtract_frame_transforms(s.root_pos, s.root_quat, tw, o3);
      if (lane < 3) {
        for (int k = 0; k < 3; ++k) ob[50 + 3 * t + k] = o3[k];
      } else if (valid) {
        for (int k = 0; k < 3; ++k) side[(kSideState + 2 + 3 * t + k) * n + e] = __float_as_uint(o3[k]);
      }
    }
    __syncthreads();
    if (valid) {
      float* orow = Q.obs + (size_t)e * AS_OBS_DIM;
      orow[lane] = ob[lane];
      if (lane < AS_OBS_DIM - 32) orow[32 + lane] = ob[32 + lane];
      if (lane == 0) {
        const uint32_t sv[kSideState + 2] = {(uint32_t)idx, (uint32_t)prev, (uint32_t)next, (uint32_t)count,
                                             (uint32_t)swing, __float_as_uint(pot), __float_as_uint(old_pot),
                                             __float_as_uint(fc[0]), __float_as_uint(fc[1]),
                                             __float_as_uint(fc[0]), __float_as_uint(fc[1])};
        for (int k = 0; k < kSideState + 2; ++k) side[k * n + e] = sv[k];
        side[kSideRegen * n + e] = regen ? 1u : 0u;
      }
    }
    idx = i2; prev = p2; next = n2; count = c2; swing = w2;
    pot = pot2; old_pot = op2; fc[0] = fc2[0]; fc[1] = fc2[1];
  }
  ts.mark(kStReset);
  // ---- store
  if (valid) {
    if (lane < 3) {
      sq.root_pos[lane * n + e] = s.root_pos[lane];
      sq.root_lin[lane * n + e] = s.u[lane];
      sq.root_ang[lane * n + e] = s.u[3 + lane];
    }
    if (lane < 4) sq.root_quat[lane * n + e] = s.root_quat[lane];
    if (lane < nh) {
      int i = rs_li - 1;
      sq.q[lane * n + e] = s.qi[i];
      sq.qd[lane * n + e] = s.u[6 + i];
    }
    if (lane < 9) {
      float v = bp[0];
#pragma unroll
      for (int k = 1; k < 9; ++k) v = (lane == k) ? bp[k] : v;
      sq.body_pos[lane * n + e] = v;
    }
    if (lane == 0) {
      // an env reset in this launch starts the next one from the spawn pose in the air: no rows
      // (its fallen-state rows predicted a heavy wave that was not; C3 +1 %, r06q)
      Q.side[kSideCost * n + e] = done ? 0u : (uint32_t)s.nrows;
      sq.contact_mask[e] = s.mask[0];
      sq.contact_mask[n + e] = s.mask[1];
      if (sq.contact_mask_hind) {
        sq.contact_mask_hind[e] = s.mask[2];
        sq.contact_mask_hind[n + e] = s.mask[3];
      }
      if (Q.mode != kModePhysics) {
        sq.idx[e] = idx; sq.prev[e] = prev; sq.next[e] = next; sq.count[e] = count; sq.swing[e] = swing;
        sq.ep_len[e] = ep_len; sq.pot[e] = pot; sq.old_pot[e] = old_pot;
        sq.foot_contact[e] = fc[0]; sq.foot_contact[n + e] = fc[1];
        sq.episode[e] = episode;
      }
    }
  }
  ts.mark(kStStore);
  ts.flush();
}

// The StepArgs of a kernel whose one parameter it is, by value: the explicit arguments start the kernarg segment,
// so it lies at offset 0.  Only such a kernel may call this (k_step and k_step_diag below do, for step_body).
__device__ __forceinline__ KArgs* step_kargs() { return (KArgs*)__builtin_amdgcn_kernarg_segment_ptr(); }

template <int NV, uint64_t SKIP>
__global__ __launch_bounds__(kStepThreads) __attribute__((amdgpu_waves_per_eu(2, 2))) void k_step(StepArgs P) {
  step_body<NV, SKIP, false>(P, step_kargs());
}

// the twin with the diagnostic stamps (as_debug_stamps): launched exactly when StepArgs::stamps is set
template <int NV, uint64_t SKIP>
__global__ __launch_bounds__(kStepThreads) __attribute__((amdgpu_waves_per_eu(2, 2))) void k_step_diag(StepArgs P) {
  step_body<NV, SKIP, true>(P, step_kargs());
}

}  // namespace as

#include "task_kernels.h"
#include "body_state_kernel.h"
#include "contact_forces_kernel.h"
#include "noise_kernels.h"
#include "event_kernels.h"
#include "contact_timer_kernels.h"
#include "ray_caster_kernels.h"
#include "imu_kernels.h"
#include "frame_transformer_kernels.h"
#include "ray_camera_kernels.h"
#include "command_kernels.h"
#include "observation_kernels.h"
#include "reward_kernels.h"
#include "termination_kernels.h"
#include "action_kernels.h"

namespace as {

// ------------------------------------------------------------------------------------------------
// launchers

// NV = 27: the Allsteps walker (6 + 21 hinges); NV = 18: the quadruped of BASELINE C5
// (model/anymal_c.xml, 6 + 12 hinges), stepped through as_physics_step.
bool step_supported_nv(int nv) { return nv == 27 || nv == 18; }

template <int NV, uint64_t SKIP>
static void launch_step_twin(const StepArgs& a, hipStream_t stream) {
  const int blocks = (a.n + EPB - 1) / EPB;
  if (a.stamps)
    hipLaunchKernelGGL((k_step_diag<NV, SKIP>), dim3(blocks), dim3(kStepThreads), 0, stream, a);
  else
    hipLaunchKernelGGL((k_step<NV, SKIP>), dim3(blocks), dim3(kStepThreads), 0, stream, a);
}

// the diagnostic twin exactly when the stamps are on (a.stamps != nullptr), the production kernel otherwise
hipError_t launch_step(const StepArgs& a, int nv, bool sweep_skip, hipStream_t stream) {
  if (nv == 27 && sweep_skip)
    launch_step_twin<27, kSweepSkip27>(a, stream);
  else if (nv == 27)
    launch_step_twin<27, 0ull>(a, stream);
  else if (nv == 18 && sweep_skip)
    launch_step_twin<18, kSweepSkip18>(a, stream);
  else if (nv == 18)
    launch_step_twin<18, 0ull>(a, stream);
  else
    return hipErrorInvalidValue;
  return hipGetLastError();
}

hipError_t launch_obs(const ObsArgs& a, hipStream_t stream) {
  // 64-thread workgroups: one wave per CU spreads the (latency-bound, one env per lane) work over
  // 4x as many CUs and their L1 / address paths
  int blocks = (a.n + 63) / 64;
  hipLaunchKernelGGL(k_obs, dim3(blocks), dim3(64), 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_stones(const StonesArgs& a, hipStream_t stream) {
  int blocks = (a.n + 255) / 256;
  hipLaunchKernelGGL(k_stones, dim3(blocks), dim3(256), 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_quad(const QuadArgs& a, hipStream_t stream) {
  hipLaunchKernelGGL(k_quad<false>, dim3((a.n + kQuadEnvs - 1) / kQuadEnvs), dim3(4 * kQuadEnvs), 0, stream, a,
                     (const uint8_t*)nullptr);
  return hipGetLastError();
}

hipError_t launch_quad_reset_mask(const QuadArgs& a, const uint8_t* mask, hipStream_t stream) {
  hipLaunchKernelGGL(k_quad<true>, dim3((a.n + kQuadEnvs - 1) / kQuadEnvs), dim3(4 * kQuadEnvs), 0, stream, a, mask);
  return hipGetLastError();
}

hipError_t launch_body_state(const BodyArgs& a, hipStream_t stream) {
  const int blocks = (a.n + EPB - 1) / EPB;
  hipLaunchKernelGGL(k_body_state, dim3(blocks), dim3(kStepThreads), 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_contact_forces(const ForcesArgs& a, hipStream_t stream) {
  const int blocks = (a.n + kForcesThreads - 1) / kForcesThreads;
  hipLaunchKernelGGL(k_contact_forces, dim3(blocks, a.depth), dim3(kForcesThreads), 0, stream, a);
  return hipGetLastError();
}

// n << gshift threads (n <= AS_MAX_ENVS = 2^24, gshift <= 6: at most 2^22 workgroups)
hipError_t launch_noise_actions(const NoiseActArgs& a, hipStream_t stream) {
  const int64_t threads = (int64_t)a.n << a.gshift;
  hipLaunchKernelGGL(k_noise_actions, dim3((unsigned)((threads + kNoiseThreads - 1) / kNoiseThreads)),
                     dim3(kNoiseThreads), 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_noise_post(const NoisePostArgs& a, hipStream_t stream) {
  const int64_t threads = (int64_t)a.n << a.gshift;
  hipLaunchKernelGGL(k_noise_post, dim3((unsigned)((threads + kNoiseThreads - 1) / kNoiseThreads)),
                     dim3(kNoiseThreads), 0, stream, a);
  return hipGetLastError();
}

// one thread per env (n <= AS_MAX_ENVS = 2^24: at most 2^16 workgroups)
hipError_t launch_events_interval(const EventsArgs& a, hipStream_t stream) {
  hipLaunchKernelGGL(k_events_interval, dim3((unsigned)((a.n + kEventThreads - 1) / kEventThreads)),
                     dim3(kEventThreads), 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_events_init(const EventsArgs& a, hipStream_t stream) {
  hipLaunchKernelGGL(k_events_init, dim3((unsigned)((a.n + kEventThreads - 1) / kEventThreads)),
                     dim3(kEventThreads), 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_observations(const ObservationsArgs& a, hipStream_t stream) {
  hipLaunchKernelGGL(k_observations, dim3((unsigned)((a.n + kObsTile - 1) / kObsTile)), dim3(kObsThreads), 0, stream,
                     a);
  return hipGetLastError();
}

hipError_t launch_observations_reset(const ObservationsArgs& a, hipStream_t stream) {
  hipLaunchKernelGGL(k_observations_reset, dim3((unsigned)((a.n + kObsTile - 1) / kObsTile)), dim3(kObsThreads), 0,
                     stream, a);
  return hipGetLastError();
}

hipError_t launch_rewards_step(const RewardsArgs& a, hipStream_t stream) {
  hipLaunchKernelGGL(k_rewards_step, dim3((unsigned)((a.n + kRewEnvs - 1) / kRewEnvs)), dim3(kRewThreads), 0, stream,
                     a);
  return hipGetLastError();
}

hipError_t launch_rewards_reset(const RewardsArgs& a, hipStream_t stream) {
  hipLaunchKernelGGL(k_rewards_reset, dim3((unsigned)((a.n + kRewThreads - 1) / kRewThreads)), dim3(kRewThreads), 0,
                     stream, a);
  return hipGetLastError();
}

hipError_t launch_terminations_step(const TerminationsArgs& a, hipStream_t stream) {
  hipLaunchKernelGGL(k_terminations_step, dim3((unsigned)((a.n + kTermEnvs - 1) / kTermEnvs)), dim3(kTermThreads), 0,
                     stream, a);
  return hipGetLastError();
}

hipError_t launch_actions_process(const ActionsArgs& a, hipStream_t stream) {
  const int64_t total = (int64_t)a.n * a.num_cols;
  hipLaunchKernelGGL(k_actions_process, dim3((unsigned)((total + kActionThreads - 1) / kActionThreads)),
                     dim3(kActionThreads), 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_actions_reset(const ActionsArgs& a, hipStream_t stream) {
  const int64_t total = (int64_t)a.n * a.num_cols;
  hipLaunchKernelGGL(k_actions_reset, dim3((unsigned)((total + kActionThreads - 1) / kActionThreads)),
                     dim3(kActionThreads), 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_commands_step(const CommandsArgs& a, hipStream_t stream) {
  hipLaunchKernelGGL(k_commands_step, dim3((unsigned)((a.n + kCommandThreads - 1) / kCommandThreads)),
                     dim3(kCommandThreads), 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_commands_reset(const CommandsArgs& a, hipStream_t stream) {
  hipLaunchKernelGGL(k_commands_reset, dim3((unsigned)((a.n + kCommandThreads - 1) / kCommandThreads)),
                     dim3(kCommandThreads), 0, stream, a);
  return hipGetLastError();
}

// kTimerEnvs envs x kTimerGroup body waves per workgroup (n <= AS_MAX_ENVS = 2^24: at most 2^18 workgroups)
hipError_t launch_contact_timers(const TimersArgs& a, hipStream_t stream) {
  hipLaunchKernelGGL(k_contact_timers, dim3((unsigned)((a.n + kTimerEnvs - 1) / kTimerEnvs)),
                     dim3(kTimerEnvs, kTimerGroup), 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_imu(const ImuArgs& a, hipStream_t stream) {
  const int blocks = (a.n + EPB - 1) / EPB;
  hipLaunchKernelGGL(k_imu, dim3(blocks), dim3(kStepThreads), 0, stream, a);
  return hipGetLastError();
}

hipError_t launch_frame_transformer(const FrameTransformerArgs& a, hipStream_t stream) {
  const int blocks = (a.n + EPB - 1) / EPB;
  hipLaunchKernelGGL(k_frame_transformer, dim3(blocks), dim3(kStepThreads), 0, stream, a);
  return hipGetLastError();
}

// kRayEnvs envs x kRayWaves ray slices per workgroup; the slice length: as few rays as give the grid about
// kRayTargetWaves waves, at least kRayMinChunk (num_rays <= AS_MAX_RAYS: blockIdx.y stays far below its limit)
hipError_t launch_ray_cast(RayArgs a, hipStream_t stream) {
  const int env_waves = (a.n + kRayEnvs - 1) / kRayEnvs;
  const int want = std::max(1, (kRayTargetWaves + env_waves - 1) / env_waves);  // slices per env wave
  a.chunk = std::max(kRayMinChunk, (a.num_rays + want - 1) / want);
  const int slices = (a.num_rays + a.chunk - 1) / a.chunk;
  hipLaunchKernelGGL(k_ray_cast, dim3((unsigned)env_waves, (unsigned)((slices + kRayWaves - 1) / kRayWaves)),
                     dim3(kRayEnvs, kRayWaves), 0, stream, a, a.rays);
  return hipGetLastError();
}

// one env x kCamTile pixels per workgroup; envs over grid y and z (num_rays <= AS_MAX_CAMERA_RAYS: at most 64 tiles)
hipError_t launch_ray_camera(const CamArgs& a, hipStream_t stream) {
  const int tiles = (a.num_rays + kCamTile - 1) / kCamTile;
  const int ey = std::min(a.n, kCamGridY), ez = (a.n + kCamGridY - 1) / kCamGridY;
  hipLaunchKernelGGL(k_ray_camera, dim3((unsigned)tiles, (unsigned)ey, (unsigned)ez), dim3(kCamTile), 0, stream, a,
                     a.root_pos, a.root_quat, a.stones, a.offset, a.dirs);
  return hipGetLastError();
}

__global__ __launch_bounds__(256) void k_zero(int32_t* p, int n) {
  for (int i = threadIdx.x; i < n; i += blockDim.x) p[i] = 0;
}

hipError_t launch_zero(int32_t* p, int n, hipStream_t stream) {
  hipLaunchKernelGGL(k_zero, dim3(1), dim3(256), 0, stream, p, n);
  return hipGetLastError();
}

size_t step_lds_bytes() { return sizeof(Smem) + sizeof(Consts); }

}  // namespace as
