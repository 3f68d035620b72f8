// step_solve.h -- the constrained half of a substep: constraint rows, W = H^-1 J^T, the PGS, integration, and
// substep() itself, which runs the phases of step_dynamics.h and step_collide.h in order.
// Reads the contact list, S, b and u; writes x.k (J rows), rmeta, cdir, rlink, rsign, x.cf and the sensor
// masks, and integrates u, qi, root_pos and root_quat.
#pragma once

#include <hip/hip_runtime.h>

#include "step_collide.h"
#include "step_dynamics.h"
#include "step_lanes.h"
#include "step_scratch.h"

namespace as {

__device__ void tangents(const float* n, float* t1, float* t2) {
  float e[3] = {1.f, 0.f, 0.f};
  if (fabsf(n[0]) > 0.9f) { e[0] = 0.f; e[1] = 1.f; }
  cross3(n, e, t1);
  float inv = 1.0f / sqrtf(dot3(t1, t1));
  for (int k = 0; k < 3; ++k) t1[k] *= inv;
  cross3(n, t1, t2);
}

// Contact-sensor flag of lane c's contact (c < nce, a foot contact): |sum lambda_n n| / dt over the
// contacts c2 < nce with its (foot, stone) pair, in ascending order; NC = the wave's larger nce.  Each
// contact's products lambda_n n and its pair key come from one 16-B LDS row (EnvS::x.cf; the same
// products the per-term form rounded; keys past nce never match), so a term is one read.
template <int NC>
__device__ __forceinline__ void contact_flag(const EnvS& s, int lane, int nce, float dt, uint32_t (&b)[4]) {
  static_assert(NC <= MAXC, "contacts");
  const int cl = lane < MAXC ? lane : 0;
  const int f = s.cfoot[cl], st = s.cstone[cl];
  const int key = __float_as_int(s.x.cf[cl][3]);
  float fx = 0.f, fy = 0.f, fz = 0.f;
  // all rows read first and passed through an empty asm, so that one wait covers every read (left to
  // the scheduler, each read was issued only when the previous term's registers freed: one LDS latency
  // per term)
  v4f t[NC];
#pragma unroll
  for (int c2 = 0; c2 < NC; ++c2) t[c2] = *reinterpret_cast<const v4f*>(s.x.cf[c2]);
  static_assert(NC == 10, "operand list below");
  asm volatile("" : "+v"(t[0]), "+v"(t[1]), "+v"(t[2]), "+v"(t[3]), "+v"(t[4]), "+v"(t[5]), "+v"(t[6]), "+v"(t[7]),
               "+v"(t[8]), "+v"(t[9]));
#pragma unroll
  for (int c2 = 0; c2 < NC; ++c2) {
    const v4f v = t[c2];
    const bool same = __float_as_int(v.w) == key;
    fx += same ? v.x : 0.f;
    fy += same ? v.y : 0.f;
    fz += same ? v.z : 0.f;
  }
  if (lane < nce && f >= 0 && sqrtf(fx * fx + fy * fy + fz * fz) / dt > 1e-4f) b[f & 3] = 1u << st;
}

// Dot product of two padded rows held as packed pairs: two interleaved partial sums (even / odd
// element, fmaf chains ascending; v_pk_fma_f32 is the two fmafs), added at the end.  oracle/physics.c
// dot_pairs is the same arithmetic.
template <int NPR>
__device__ __forceinline__ float dot_pairs(const v2f (&a)[NPR], const v2f (&b)[NPR]) {
  v2f p = v2f{0.f, 0.f};
#pragma unroll
  for (int i = 0; i < NPR; ++i) p = __builtin_elementwise_fma(a[i], b[i], p);
  return p.x + p.y;
}

// W = H^-1 J^T for both envs of the wave on the matrix cores: v_mfma_f32_32x32x1_2b_f32 holds one
// 32 x 32 block per env (block b = lanes 32b..32b+31), K = 1 per instruction, so step k takes lane r's
// J_rk as the A operand (the lane built row r: no data movement) and lane j's (H^-1)_jk as the B
// operand (lane j holds row j of H^-1 after the sweep), and after NV steps block b holds
//   W_r[j] = sum_k J_rk (H^-1)_jk,   an fmaf chain over k ascending (gfx950 f32 MFMA numerics:
// bit for bit D = fma(a_k, b_k, C) per step -- scripts/probes/mfma_2b_probe.hip checks the layout and
// the chain on hardware; oracle/physics.c forms the same chain).  The result's layout (register v of
// block b: row 8(v/4) + 4h + v%4 on lane half h, column j = lane % 32) is brought to "lane j holds W_rj
// for every row r of its own env" by one v_permlane32_swap per register pair (blocks 0 and 1 trade
// their upper / lower halves).  The projections then need W by rows: lane j stores its column into
// the J image (after lane j has read its J column, the PGS's Jc), and
//   lane r forms A_rr = J_r . W_r and the in-triplet projections A_sr = J_s . W_r (r < s; lane s, from
//   the W rows of the two rows before it): each row's PGS coupling x_s A_sr is formed and stored by
//   that lane (no lane reads another lane's LDS result without a barrier in between).
// Cost per substep: NV MFMAs (64 cycles each on the SIMD's matrix pipe), independent of the row
// count; the LDS carries only the transposes.
template <int NV>
__device__ __forceinline__ void w_rows(EnvS& s, int lane, int nrow, const float* Hr, const v2f (&Jr)[LDJ / 2],
                                       float (&Jc)[MAXR], float (&Wc)[MAXR], uint32_t jmask) {
  static_assert(NV < LDJ, "padding column NV");
  static_assert(MAXR <= 32, "rows of one MFMA block");
  constexpr int NQ = (NV + 3) / 4;  // 16-B quads of a row that hold dofs
  float(*M)[LDJ] = s.x.k.Jm;
  const int jc = lane < NV ? lane : NV;  // column NV is +0 in the J image
#pragma unroll
  for (int r = 0; r < MAXR; ++r) Jc[r] = M[r][jc];
  // (an empty volatile asm orders memory operations: the J column reads issue here, and their latency
  // hides under the MFMA chain instead of heading the barrier below)
  float j0 = Jr[0].x;  // the MFMA chain's first operand, through the asm: the chain starts after it
  asm volatile("" : "+v"(j0));
  f32x32 acc = {};
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    const float jk = k == 0 ? j0 : k & 1 ? Jr[k >> 1].y : Jr[k >> 1].x;
    // K step k only when some live row of either env can be nonzero at dof k (jmask, uniform): every
    // other step would add J_rk (H^-1)_jk = +0 x h to an accumulator that started at +0 and so is never
    // -0 -- the same bits (C3 +1.6 %, C2 +0.4 %: r06u)
    if ((jmask >> k) & 1u) acc = __builtin_amdgcn_mfma_f32_32x32x1f32(jk, Hr[k], acc, 0, 0, 0);
  }
  float wr[32];
  mfma_columns(acc, wr);
#pragma unroll
  for (int r = 0; r < MAXR; ++r) Wc[r] = wr[r];
  __syncthreads();  // every lane's J column reads are done
  if (lane < LDJ) {
#pragma unroll
    for (int r = 0; r < MAXR; ++r) M[r][lane] = wr[r];
  }
  __syncthreads();
  v2f jn[2 * NQ];
#pragma unroll
  for (int i = 0; i < 2 * NQ; ++i) jn[i] = Jr[i];
  const int r0 = lane < MAXR ? lane : 0;
  const int r1 = lane >= 1 ? min(lane - 1, MAXR - 1) : 0, r2 = lane >= 2 ? min(lane - 2, MAXR - 1) : 0;
  v2f w0[2 * NQ], w1[2 * NQ], w2[2 * NQ];
#pragma unroll
  for (int q = 0; q < NQ; ++q) {
    const v4f c = *reinterpret_cast<const v4f*>(&M[r0][4 * q]);
    const v4f a = *reinterpret_cast<const v4f*>(&M[r1][4 * q]);
    const v4f b = *reinterpret_cast<const v4f*>(&M[r2][4 * q]);
    w0[2 * q] = c.xy; w0[2 * q + 1] = c.zw;
    w1[2 * q] = a.xy; w1[2 * q + 1] = a.zw;
    w2[2 * q] = b.xy; w2[2 * q + 1] = b.zw;
  }
  const float arr = dot_pairs(jn, w0);  // A_{lane, lane}
  const float a1 = dot_pairs(jn, w1);   // A_{lane, lane-1}
  const float a2 = dot_pairs(jn, w2);   // A_{lane, lane-2}
  if (lane < MAXR) {
    const float x = lane < nrow ? 1.0f / (arr + 1e-9f) : 0.f;
    s.rmeta[lane][0] = x;
    if (lane >= nrow) { s.rmeta[lane][1] = 0.f; s.rmeta[lane][2] = lane % 3 == 2 ? __builtin_inff() : 0.f; }
    // the PGS coupling factors x_s A_sr: row r0 holds x_1 A_10, row r0 + 1 x_2 A_20, row r0 + 2 x_2 A_21
    const int t = lane % 3;
    if (t == 1) s.rmeta[lane - 1][3] = x * a1;
    if (t == 2) {
      s.rmeta[lane - 1][3] = x * a2;
      s.rmeta[lane][3] = x * a1;
    }
  }
}

// PGS sweeps over NG row groups (see substep): rows in order, contacts as (normal, tangent, tangent)
// triplets, then joint limits; lane j holds u_j and every lane of an env all its impulses.  A group
// takes its three velocities J_r . u from the u at its start (three interleaved half-wave reductions)
// and adds the in-group couplings A_sr dlambda_r of the rows before it -- the Gauss-Seidel sweep row
// by row (J_s . (u + W_r dl_r) = J_s . u + A_sr dl_r) with one reduction latency per group.
template <int NG>
__device__ __forceinline__ void pgs_sweeps(const EnvS& s, int iters, float& uj, float (&lamr)[MAXR],
                                           const float (&Jc)[MAXR], const float (&Wc)[MAXR]) {
  typedef __attribute__((address_space(3))) const v4f* lds_v4p;
  lds_v4p meta = (lds_v4p)(&s.rmeta[0][0]);
  // Software-pipelined metadata: group g+1's three rows are read at the head of group g (between two
  // empty volatile asm statements, which order memory operations: the reads issue before group g's
  // reductions start) and consumed after group g+1's reductions, so the LDS latency is hidden by a
  // whole group.  Reading them at the head of their own group left each group waiting on the read
  // (its destination registers were reused as soon as the unused lane-0 bound field died).  The row
  // metadata is the same in every sweep, so the last group reads group 0 for the next sweep.
  v4f n0 = meta[0], n1 = meta[1], n2 = meta[2];
#pragma unroll 1
  for (int it = 0; it < iters; ++it) {
#pragma unroll
    for (int g = 0; g < NG; ++g) {
      const int r = kRowGroup * g;
      // the group's rows pass through the asm: no use of them is hoisted into the previous group
      // (where it would wait on the read), and every field's register -- m0.z too, a bound that row 0
      // of a group never uses -- stays allocated to the read until the read has landed
      v4f m0 = n0, m1 = n1, m2 = n2;
      asm volatile("" : "+v"(meta), "+v"(uj), "+v"(m0), "+v"(m1), "+v"(m2));
      {
        const int rn = g + 1 < NG ? r + kRowGroup : 0;
        n0 = meta[rn];
        n1 = meta[rn + 1];
        n2 = meta[rn + 2];
      }
      asm volatile("" : "+v"(uj));
      float vg[3] = {Jc[r] * uj, Jc[r + 1] * uj, Jc[r + 2] * uj};
      half_sum_n(vg);
      // t_s = lambda_s + (target_s - v_s - sum_{r<s} A_sr dl_r) x_s, with the parts that do not
      // depend on this sweep's impulse changes formed first: the chain from one row's dl to the
      // next row's clamp is a single FMA
      const float k10 = m0.w, k20 = m1.w, k21 = m2.w;  // x_s A_sr, formed after the W pass
      float t1 = fmaf(-vg[1], m1.x, fmaf(m1.y, m1.x, lamr[r + 1]));
      float t2 = fmaf(-vg[2], m2.x, fmaf(m2.y, m2.x, lamr[r + 2]));
      // Row types by group: a contact triplet is (normal, tangent, tangent), every other group holds
      // limit rows (or the zero rows past nrow); contacts come first.  So row 0 always clamps to
      // [0, inf) and its impulse ln bounds only this triplet's tangents, and rows 1 and 2 share one
      // pair of bounds, +-mu ln for a contact triplet and [0, inf) otherwise -- the bounds a per-row
      // clamp forms, bit for bit (fmaf(-0, ln, 0) = +0 for the finite ln >= 0); the two bound
      // parameters were stored with the rows (EnvS::rmeta), so no type test runs in the sweep.
      const float mu_g = m1.z, off_g = m2.z;
      const float l0 = __builtin_amdgcn_fmed3f(fmaf(-vg[0], m0.x, fmaf(m0.y, m0.x, lamr[r])), 0.f, __builtin_inff());
      const float d0 = l0 - lamr[r];
      lamr[r] = l0;
      const float blo = fmaf(-mu_g, l0, 0.f), bhi = fmaf(mu_g, l0, off_g);
      t1 = fmaf(-k10, d0, t1);
      t2 = fmaf(-k20, d0, t2);
      uj = fmaf(Wc[r], d0, uj);
      const float l1 = __builtin_amdgcn_fmed3f(t1, blo, bhi);
      const float d1 = l1 - lamr[r + 1];
      lamr[r + 1] = l1;
      t2 = fmaf(-k21, d1, t2);
      uj = fmaf(Wc[r + 1], d1, uj);
      const float l2 = __builtin_amdgcn_fmed3f(t2, blo, bhi);
      const float d2 = l2 - lamr[r + 2];
      lamr[r + 2] = l2;
      uj = fmaf(Wc[r + 2], d2, uj);
    }
  }
}

template <int NV, uint64_t SKIP, class TS>
__device__ void substep(const Consts& K0, Smem& sm, EnvS& s, int lane0, const Topo& tp0, const GeomC& gc,
                        const LinkC& lc, uint32_t (&mask_out)[4], TS& ts) {
  // Opaque copies of the constants pointer and the lane id: everything derived from them below
  // (model-table loads, LDS addresses, lane masks) is loop-invariant, and without this the
  // compiler hoists all of it out of the substep loop and spills it.
  CK* kp = (CK*)(&K0);
  int lane = lane0;
  asm volatile("" : "+s"(kp), "+v"(lane));
  const Consts& K = *(const Consts*)(kp);
  const Topo& tp = tp0;  // LDS (Smem::topo)
  const as_model_t& m = K.model;
  const int nh = m.num_hinges;
  // A fresh opaque copy of the constants pointer for the phases that read dt (u*, the rows, the integration):
  // each loads its own dt, one short live range per phase.  One load at the top of the substep was held across
  // the H rows' lane masks, the substep's SGPR peak, and spilled and reloaded inside the loop -- as was
  // model.com[0], read by the first FK and again by the integration.
  auto fresh = [kp]() -> const Consts& {
    CK* q = kp;
    asm volatile("" : "+s"(q));
    return *(const Consts*)(q);
  };
  // Scalars of the model loaded in groups just ahead of the phases that use them, each group passed
  // through an empty asm: one wait per group instead of a scalar load and a wait beside each use (a
  // wait on the scalar loads also waits on every LDS read in flight, so each one exposed an LDS
  // latency too).  Short live ranges: held across the whole substep they pushed the epilogue's SGPRs
  // into spills.
  int smp = K.max_path;
  asm volatile("" : "+s"(smp));
  if (K.act.mode == AS_ACT_DC_MOTOR && lane < nh) {  // the actuator runs in every substep (lane = hinge)
    const as_actuator_t& A = K.act;
    s.tau[lane] = as_dc_motor(s.qt[lane], s.qi[lane], s.u[6 + lane], A.stiffness, A.damping, A.saturation_effort,
                              A.effort_limit, A.velocity_limit);
  }
  fk<true>(K, s, lane, tp, lc, smp);  // (its first barrier publishes tau before the dynamics read it)
  ts.mark(kStFK);
  float Sj[6], Fj[6];  // dof lane j: S_j and Ic_link(j) S_j for the H rows
  dynamics<NV>(K, s, lane, tp, K.sim.gravity, Sj, Fj, smp);
  ts.mark(kStLinkQ);
  typedef SweepLayout<NV> SL;
  constexpr int NP = SL::NP;
  float Hr[NP];
  h_row<NV>(s, lane, tp, gc.anc, Sj, Fj, *reinterpret_cast<float(*)[NV]>(Hr));
  ts.mark(kStDyn);
  const float dt = fresh().sim.dt;  // (loaded here, under the sweep: u* below is its first use)
  {
    // into the sweep's round-0 column order with the identity pad rows / columns (register renaming),
    // the sweep, and back: row `lane` of H^-1 in dof order
    float Hs[NP];
#pragma unroll
    for (int k = 0; k < NV; ++k) Hs[SL::pos(SL::padded(k))] = Hr[k];
#pragma unroll
    for (int q = 0; q < NP - NV; ++q) Hs[SL::pos(SL::PAD + q)] = lane == NV + q ? 1.f : 0.f;
    sweep_inverse<NV, SKIP>(s, lane, Hs);  // Hs <- this lane's row of -H^-1
#pragma unroll
    for (int k = 0; k < NV; ++k) Hr[k] = lane < NV ? -Hs[SL::pos(SL::padded(k))] : 0.f;
#pragma unroll
    for (int k = NV; k < NP; ++k) Hr[k] = 0.f;
  }
  ts.mark(kStChol);
  // (the lane id, opaque again here and ahead of the W rows and the integration: a lane mask formed in one phase
  // -- lane < nh, lane >= 1 -- is formed again where a later phase tests it, one VALU compare, not held as an
  // SGPR pair across the phases between and spilled inside the loop)
  asm volatile("" : "+v"(lane));
  // u* = u + dt H^-1 b   (b broadcast from LDS)
  float uj = 0.f;
  {
    float acc = 0.f;
#pragma unroll
    for (int k = 0; k < NV; ++k) acc = fmaf(Hr[k], s.b[k], acc);
    if (lane < NV) {
      uj = fmaf(dt, acc, s.u[lane]);
      s.u[lane] = uj;
    }
  }
  __syncthreads();
  ts.mark(kStSolve);
  // ---- constraints.  Joint-limit rows first counted (every one is kept), then the contacts fill the
  //      remaining rows, at most MAXC; rows are ordered contacts (normal, tangent, tangent), then the
  //      limits (lane h = hinge: lower then upper, in hinge order)
  int lo_v = 0, hi_v = 0;
  float err_lo = 0.f, err_hi = 0.f;
  if (lane < nh) {
    float qv = s.qi[lane], pred = qv + dt * s.u[6 + lane];
    err_lo = tp.lo - qv;
    err_hi = qv - tp.hi;
    lo_v = pred < tp.lo;
    hi_v = pred > tp.hi;
  }
  int ltotal;
  const int lpos = half_scan3(lo_v + hi_v, ltotal);
  const int nlim = ltotal < MAXR ? ltotal : MAXR;
  const int ncap = (MAXR - nlim) / 3 < MAXC ? (MAXR - nlim) / 3 : MAXC;
  float sb = K.sim.baumgarte, ssl = K.sim.slop, smd = K.sim.max_depen_vel, sfr = K.sim.friction, smg = K.sim.margin;
  float sh[3] = {K.sim.stone_half[0], K.sim.stone_half[1], K.sim.stone_half[2]};
  int gcap = K.pair_group_cap;
  asm volatile("" : "+s"(sb), "+s"(ssl), "+s"(smd), "+s"(sfr), "+s"(smg), "+s"(sh[0]), "+s"(sh[1]), "+s"(sh[2]),
               "+s"(gcap));
  const int nc = collide(K, s, lane, ncap, gc, sh, smg, gcap, ts);
  ts.mark(kStCollide);

  if (lane < nc) {  // contact rows 3c..3c+2: normal, tangent 1, tangent 2
    float t1[3], t2[3];
    tangents(s.cn[lane], t1, t2);
    const float* dirs[3] = {s.cn[lane], t1, t2};
    float sp = s.csep[lane];
    const int lk = s.clink[lane] | ((s.clink2[lane] + 1) << 8);
    for (int d = 0; d < 3; ++d) {
      int r = 3 * lane + d;
      for (int k = 0; k < 3; ++k) s.cdir[lane][d][k] = dirs[d][k];
      s.rlink[r] = lk;
      s.rsign[r] = 0.f;
      // one division for both branches: (sp < 0 ? min(b max(-sp - slop, 0) / dt, vmax) : -sp / dt)
      const float num = sp < 0.f ? sb * fmaxf(-sp - ssl, 0.f) : -sp;
      const float tv = num / dt;
      s.rmeta[r][1] = d == 0 ? (sp < 0.f ? fminf(tv, smd) : tv) : 0.f;
      s.rmeta[r][2] = d == 1 ? sfr : 0.f;
    }
  }
  const int crow = 3 * nc;
  int slot = crow + lpos;
  for (int sd = 0; sd < 2; ++sd) {
    int viol = sd == 0 ? lo_v : hi_v;
    if (!viol) continue;
    if (slot < MAXR) {
      float err = sd == 0 ? err_lo : err_hi;
      s.rlink[slot] = -1 - (6 + lane);
      s.rsign[slot] = sd == 0 ? 1.f : -1.f;
      const float tv = (err > 0.f ? sb * err : err) / dt;  // one division, both branches
      s.rmeta[slot][1] = err > 0.f ? fminf(tv, smd) : tv;
      s.rmeta[slot][2] = slot % 3 == 2 ? __builtin_inff() : 0.f;
    }
    ++slot;
  }
  const int nrow = crow + nlim;  // uniform over the env's half-wave
  ts.count(nrow, nc);
  if (lane == 0) s.nrows += nrow;  // (the last substep's rows, or the peak, predict no better: r06j)
  const int maxrow = max(__builtin_amdgcn_readlane(nrow, 0), __builtin_amdgcn_readlane(nrow, 32));
  __syncthreads();  // the row metadata above, for the J build
  // Issue priority by constraint load: the two waves of a SIMD are arbitrated by priority, then
  // age, so a contact-heavy wave that happens to be the younger one would get only the leftover
  // issue slots and set the launch's tail.  The heavier wave of the pair takes precedence for the
  // rest of this substep and the fixed-cost phases of the next (scalar branch: s_setprio is not
  // masked by EXEC, so exactly one of them may execute).
  {
    const int lvl = __builtin_amdgcn_readfirstlane(maxrow) / kPrioRows;
    if (lvl >= 3) __builtin_amdgcn_s_setprio(3);
    else if (lvl == 2) __builtin_amdgcn_s_setprio(2);
    else if (lvl == 1) __builtin_amdgcn_s_setprio(1);
    else __builtin_amdgcn_s_setprio(0);
  }
  // ---- J rows, one lane per row (lane r < MAXR), kept in LDS [row][dof]: a contact row is
  //      J_rj = S_j . f6_r for the dofs whose link lies on the path root..link(r) (lpath of the
  //      row's link; dof j < 6 moves every link), minus the same on the second link's path for a
  //      self contact; a limit row is +-1 at its dof.  Every row < MAXR is written (zero past nrow),
  //      all rows at once: no per-row LDS round trip, no loop.  Lane r keeps its row in registers
  //      for W_r (w_rows).
  v2f Jr[LDJ / 2];
  uint32_t jmask = ~0u;
  {
    const int rr = lane < MAXR ? lane : 0;
    const int c = rr / 3, u = rr - 3 * c;
    const int lk = s.rlink[rr];
    const float sg = s.rsign[rr];
    float P[3], f6[6];  // spatial force direction [P x d; d]
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      P[k] = s.cpt[c][k];
      f6[3 + k] = s.cdir[c][u][k];
    }
    // lane j's motion-subspace row for the MFMA below, read with the row metadata; the empty volatile
    // asm orders memory operations, so these reads issue before the path-mask reads that depend on lk
    // (one LDS latency for both instead of one after the other)
    const int jo = lane < NV ? lane : 0;
    const v4f s0 = *reinterpret_cast<const v4f*>(&s.S[jo][0]);
    const v4f s1 = *reinterpret_cast<const v4f*>(&s.S[jo][4]);
    asm volatile("");
    cross3(P, f6 + 3, f6);
    const bool con = lk >= 0;
    const int l2 = (lk >> 8) - 1;
    // Every lane loads and computes everything; the selects are bit masks (exact: x & ~0 = x,
    // x & 0 = +0), so that no branch around the loads serialises one LDS round trip per column.
    const uint32_t pm1 = sm.topo[con ? lk & 31 : 0].lpath & (con ? ~0u : 0u);
    const uint32_t pm2 = sm.topo[con && l2 >= 0 ? l2 & 31 : 0].lpath & (con && l2 >= 0 ? ~0u : 0u);
    const uint32_t live = lane < nrow ? ~0u : 0u;
    // S_j . f6_r for every (dof j, row r) of both envs: six K steps of the two-block MFMA (A: lane j's
    // own motion subspace row, B: lane r's f6), an fmaf chain over the components (oracle chain6);
    // after the column shuffle lane r holds its row's products for every dof
    float Pj[32];
    {
      const float z = lane < NV ? 1.f : 0.f;
      const float Sa[6] = {s0.x * z, s0.y * z, s0.z * z, s0.w * z, s1.x * z, s1.y * z};
      f32x32 acc = {};
#pragma unroll
      for (int a = 0; a < 6; ++a) acc = __builtin_amdgcn_mfma_f32_32x32x1f32(Sa[a], f6[a], acc, 0, 0, 0);
      mfma_columns(acc, Pj);
    }
#pragma unroll
    for (int q = 0; q < LDJ / 4; ++q) {
      float jq[4];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int j = 4 * q + e;
        if (j < NV) {
          const uint32_t jb = __float_as_uint(Pj[j]);
          const int lnk = j < 6 ? 0 : j - 5;  // the link dof j moves with
          // contact row: (on path 1 ? jcon : 0) - (on path 2 ? jcon : 0), +0 on a limit row (pm = 0);
          // limit row: sign at its dof, +0 elsewhere and on every contact row (lk >= 0 > -1 - lk)
          const float jc1 = __uint_as_float(jb & (0u - ((pm1 >> lnk) & 1u)));
          const float jc2 = __uint_as_float(jb & (0u - ((pm2 >> lnk) & 1u)));
          const uint32_t jl = __float_as_uint(sg) & (-1 - lk == j ? ~0u : 0u);
          jq[e] = __uint_as_float(((__float_as_uint(jc1 - jc2)) | jl) & live);
        } else {
          jq[e] = 0.f;
        }
      }
      Jr[2 * q] = v2f{jq[0], jq[1]};
      Jr[2 * q + 1] = v2f{jq[2], jq[3]};
      if (lane < MAXR) *reinterpret_cast<v4f*>(&s.x.k.Jm[lane][4 * q]) = v4f{jq[0], jq[1], jq[2], jq[3]};
    }
    // the dofs any live row of either env can be nonzero at (structural: its links' root paths, or its
    // limit dof), OR-reduced over the wave: W's MFMA K steps outside it add +0 products only
    const uint32_t pm = pm1 | pm2;
    uint32_t dm = ((pm & 1u) ? 0x3Fu : 0u) | ((pm >> 1) << 6);
    if (!con && lane < MAXR) dm = 1u << ((-1 - lk) & 31);
    dm = lane < nrow ? dm : 0u;
    uint32_t dd = 0u;
    half_or2(dm, dd);
    jmask = (uint32_t)__builtin_amdgcn_readlane((int)dm, 0) | (uint32_t)__builtin_amdgcn_readlane((int)dm, 32);
  }
  __syncthreads();
  ts.mark(kStRows);
  // W = H^-1 J^T, A_rr and the in-triplet couplings (w_rows: one row per lane); lane j's W and J
  // columns go to registers for the PGS.  Hr is zero on lanes >= NV.
  float Wc[MAXR], Jc[MAXR];
  asm volatile("" : "+v"(lane));
  w_rows<NV>(s, lane, nrow, Hr, Jr, Jc, Wc, jmask);
  __syncthreads();
  ts.mark(kStWsolve);
  // ---- projected Gauss-Seidel (lane j holds u_j; every lane of an env holds all its impulses).
  // Rows in order: contacts as (normal, tangent, tangent) triplets, then joint limits; a tangent
  // row's bound uses the impulse of the most recent normal row (ln).  Lane j's J / W columns of
  // every row sit in registers (kept from the W pass).  A group of three rows takes the three
  // velocities J_r . u from the u at its start (three independent reductions) and adds the
  // in-group coupling A_sr dlambda_r of the rows before it, which is the Gauss-Seidel sweep row by
  // row (J_s . (u + W_r dl_r) = J_s . u + A_sr dl_r) with one reduction latency per group instead
  // of one per row.  The row loop is unrolled with an exit per group; rows in [maxrow, group end)
  // have zero J / W / metadata and leave everything unchanged.
  // (with the sweep count, in one group under the sweeps: the scalars of the flags and the integration)
  const Consts& Ki = fresh();
  const int iters = Ki.sim.pgs_iters;
  const float dti = Ki.sim.dt, mjv = Ki.sim.max_joint_vel;
  const int nhi = Ki.model.num_hinges;
  const float com0[3] = {Ki.model.com[0][0], Ki.model.com[0][1], Ki.model.com[0][2]};
  float lamr[MAXR];
#pragma unroll
  for (int r = 0; r < MAXR; ++r) lamr[r] = 0.f;
  // one instantiation per group count (maxrow is wave-uniform): the groups run without a skip test,
  // so the sweep state needs no copies at per-group joins
  static_assert(MAXR / kRowGroup == 10, "group-count dispatch");
  switch ((__builtin_amdgcn_readfirstlane(maxrow) + kRowGroup - 1) / kRowGroup) {
    case 1: pgs_sweeps<1>(s, iters, uj, lamr, Jc, Wc); break;
    case 2: pgs_sweeps<2>(s, iters, uj, lamr, Jc, Wc); break;
    case 3: pgs_sweeps<3>(s, iters, uj, lamr, Jc, Wc); break;
    case 4: pgs_sweeps<4>(s, iters, uj, lamr, Jc, Wc); break;
    case 5: pgs_sweeps<5>(s, iters, uj, lamr, Jc, Wc); break;
    case 6: pgs_sweeps<6>(s, iters, uj, lamr, Jc, Wc); break;
    case 7: pgs_sweeps<7>(s, iters, uj, lamr, Jc, Wc); break;
    case 8: pgs_sweeps<8>(s, iters, uj, lamr, Jc, Wc); break;
    case 9: pgs_sweeps<9>(s, iters, uj, lamr, Jc, Wc); break;
    case 10: pgs_sweeps<10>(s, iters, uj, lamr, Jc, Wc); break;
    default: break;
  }
  // contact c's normal impulse (row 3c; every lane of an env holds all its impulses) times its normal,
  // and its (foot, stone) key, one 16-B row per contact for the flags; contacts past the solved
  // normal rows (nce) get a key no contact has
  const int nce = min(nc, (nrow + kRowGroup - 1) / kRowGroup);  // contacts whose normal row was solved
  if (lane < NV) s.u[lane] = uj;
  if (lane < MAXC) {
    float ln = 0.f;
#pragma unroll
    for (int c = 0; c < MAXC; ++c) ln = lane == c ? lamr[3 * c] : ln;
    ln = 3 * lane < nrow ? ln : 0.f;
    const int key = lane < nce ? ((s.cfoot[lane] + 1) << 8) | (s.cstone[lane] + 1) : -1;
    *reinterpret_cast<v4f*>(s.x.cf[lane]) =
        v4f{ln * s.cn[lane][0], ln * s.cn[lane][1], ln * s.cn[lane][2], __int_as_float(key)};
  }
  __syncthreads();
  ts.mark(kStPGS);
  // ---- contact-sensor flags of this substep (force_matrix_w = impulse / dt, > eps): lane c sums
  //      lambda_n n over the contacts with its (foot, stone) pair in ascending order, and the
  //      per-foot stone bits are OR-reduced over the half-wave
  asm volatile("" : "+v"(lane));
  {
    // All MAXC terms (one 16-B read each; the terms past an env's own count add +0 to a sum that is
    // never -0: the same bits) and no per-count dispatch: the flags, the hind-feet masks (zero for a
    // biped) and the root update below are one basic block, so the scheduler interleaves the root
    // update's serial chain with the flag sums.
    uint32_t b[4] = {0u, 0u, 0u, 0u};
    contact_flag<MAXC>(s, lane, nce, dti, b);
    half_or2(b[0], b[1]);
    half_or2(b[2], b[3]);
#pragma unroll
    for (int k = 0; k < 4; ++k) mask_out[k] = b[k];
  }
  // ---- integrate.  The root update is formed by every lane of the env (no lane-0 branch; the
  //      small-angle case by selects, the same values) and stored by lane 0
  float rq[4], rp[3];
  {
    const float* u = s.u;
    float c0w[3];
    for (int k = 0; k < 3; ++k) c0w[k] = fmaf(dti, u[k], s.root_pos[k] + s.c0[k]);
    const float* w = u + 3;
    const float wn = sqrtf(dot3(w, w));
    const float th = wn * dti;
    float sn, cs;
    as_sincosf(0.5f * th, &sn, &cs);
    const float sc = sn / wn;
    const bool big = th > 1e-12f;
    const float dq[4] = {big ? cs : 1.f, big ? w[0] * sc : 0.5f * dti * w[0], big ? w[1] * sc : 0.5f * dti * w[1],
                         big ? w[2] * sc : 0.5f * dti * w[2]};
    const float* q0 = s.root_quat;
    float nq[4] = {dq[0] * q0[0] - dq[1] * q0[1] - dq[2] * q0[2] - dq[3] * q0[3],
                   dq[0] * q0[1] + dq[1] * q0[0] + dq[2] * q0[3] - dq[3] * q0[2],
                   dq[0] * q0[2] - dq[1] * q0[3] + dq[2] * q0[0] + dq[3] * q0[1],
                   dq[0] * q0[3] + dq[1] * q0[2] - dq[2] * q0[1] + dq[3] * q0[0]};
    const float qn = 1.0f / sqrtf(nq[0] * nq[0] + nq[1] * nq[1] + nq[2] * nq[2] + nq[3] * nq[3]);
    for (int k = 0; k < 4; ++k) rq[k] = nq[k] * qn;
    float Rn[9], cl[3];
    quat_to_mat(rq, Rn);
    matvec3(Rn, com0, cl);
    for (int k = 0; k < 3; ++k) rp[k] = c0w[k] - cl[k];
  }
  if (lane < nhi) {
    float v = fminf(fmaxf(s.u[6 + lane], -mjv), mjv);
    s.u[6 + lane] = v;
    s.qi[lane] = fmaf(dti, v, s.qi[lane]);
  }
  if (lane == 0) {
    for (int k = 0; k < 4; ++k) s.root_quat[k] = rq[k];
    for (int k = 0; k < 3; ++k) s.root_pos[k] = rp[k];
  }
  __syncthreads();
  ts.mark(kStIntegrate);
}

}  // namespace as
