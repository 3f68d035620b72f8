// step_dynamics.h -- the unconstrained half of a substep: FK, link dynamics, the H rows and the H^-1 sweep.
// Reads EnvS root_quat / qi / u / tau; writes R, p, c0, S, b and the dynamics scratch x.d, then x.k (h_row's
// transposed copy) and x.sw (the sweep's rows), both aliasing x.d.  H^-1 stays in the caller's registers.
#pragma once

#include <hip/hip_runtime.h>

#include "step_lanes.h"
#include "step_scratch.h"

namespace as {

// FK by ancestor-path walks.  Local joint transforms are formed in parallel (lane = link); then
// lane i composes the transforms on its own path root -> i, which is the same sequence of products
// a level-by-level pass would form (R_i = R_parent Rl_i, p_i = p_parent + R_parent t_i), with no
// level barriers: the tree depth only sets the length of the longest lane's loop.
// kDyn: also the link's spatial quantities for the dynamics (COM, spatial inertia at O, motion
// subspace of its hinge, S_i qd_i) from the registers of the walk, and the six root columns.
// Per-lane joint constants of the local transform (lane = link), read once per launch and kept in
// registers across the substeps (as lane-varying global loads they were an L2 round trip at the head
// of every substep's FK)
struct LinkC {
  float oq[4], ax[3], an[3], op[3];
};
__device__ __forceinline__ LinkC load_link(const Consts& K, int lane) {
  const as_model_t& m = K.model;
  const int i = lane >= 1 && lane < m.num_links ? lane : 0;
  LinkC c;
#pragma unroll
  for (int k = 0; k < 4; ++k) c.oq[k] = m.offset_quat[i][k];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    c.ax[k] = m.axis[i][k];
    c.an[k] = m.anchor[i][k];
    c.op[k] = m.offset_pos[i][k];
  }
  return c;
}

// KT: Consts in the generic or the constant address space (k_step's final FKs: uniform scalar loads).
template <bool kDyn, class KT>
__device__ __forceinline__ void fk(KT& K, EnvS& s, int lane, const Topo& tp, LinkC lc, int max_path) {
  auto& m = K.model;
  const int nl = m.num_links;
  DynScratch& d = s.x.d;
  // opaque per call: nothing derived from them is hoisted out of the substep loop
  asm volatile("" : "+v"(lc.oq[0]), "+v"(lc.oq[1]), "+v"(lc.oq[2]), "+v"(lc.oq[3]), "+v"(lc.ax[0]),
               "+v"(lc.ax[1]), "+v"(lc.ax[2]));
  asm volatile("" : "+v"(lc.an[0]), "+v"(lc.an[1]), "+v"(lc.an[2]), "+v"(lc.op[0]), "+v"(lc.op[1]),
               "+v"(lc.op[2]));
  // lane i: its joint's local transform A = (Rl, tl) (rotation row-major, translation), the identity
  // on the root lane; then pointer jumping over the tree (fk_rounds rounds): A_i <- A_a o A_i with a
  // the 2^r-th ancestor of i (the root's identity past the path), so after round r A_i is the product
  // of the 2^(r+1) transforms ending at i, and after the last one the whole path root -> i -- three
  // dependent compositions for the walker's 8-link paths instead of eight.  (Ra, ta) o (Rb, tb) =
  // (Ra Rb, ta + Ra tb), as_matmul3 / as_matvec3 operations; oracle/physics.c kinematics forms the same
  // products in the same association.
  float A[12];
#pragma unroll
  for (int k = 0; k < 12; ++k) A[k] = k == 0 || k == 4 || k == 8 ? 1.f : 0.f;
  if (lane >= 1 && lane < nl) {
    const int i = lane;
    float Roff[9], Rj[9], Ro[3], t[3], tmp[3];
    quat_to_mat(lc.oq, Roff);
    axis_angle_mat(lc.ax, s.qi[i - 1], Rj);
    matmul3(Roff, Rj, A);
    matvec3(Rj, lc.an, Ro);
    for (int k = 0; k < 3; ++k) t[k] = lc.an[k] - Ro[k];
    matvec3(Roff, t, tmp);
    for (int k = 0; k < 3; ++k) A[9 + k] = tmp[k] + lc.op[k];
  }
  __syncthreads();  // (also publishes the actuator's tau before the dynamics read it)
  {
    const int rounds = __builtin_amdgcn_readfirstlane(K.fk_rounds);
    const uint32_t jw = tp.jump;
    typedef __attribute__((address_space(3))) v4f* lds_v4p_t;
    for (int r = 0; r < rounds; ++r) {
      // publish this round's A (rows of 12 floats: three 16-B stores), read the ancestor's.  One wave:
      // its LDS operations complete in issue order, so the reads see this round's stores and the next
      // round's stores cannot overtake them; the empty asm keeps the compiler from reordering them
      if (lane < nl) {
        lds_v4p_t own = (lds_v4p_t)(&d.Rl[lane][0]);
        own[0] = v4f{A[0], A[1], A[2], A[3]};
        own[1] = v4f{A[4], A[5], A[6], A[7]};
        own[2] = v4f{A[8], A[9], A[10], A[11]};
      }
      asm volatile("" ::: "memory");
      const int anc = (jw >> (8 * r)) & 0xff;
      const lds_v4p_t ar = (lds_v4p_t)(&d.Rl[anc][0]);
      const v4f q0 = ar[0], q1 = ar[1], q2 = ar[2];
      asm volatile("" ::: "memory");
      const float Ra[9] = {q0.x, q0.y, q0.z, q0.w, q1.x, q1.y, q1.z, q1.w, q2.x};
      const float ta[3] = {q2.y, q2.z, q2.w};
      float Rn[9], w[3];
      matmul3(Ra, A, Rn);
      matvec3(Ra, A + 9, w);
#pragma unroll
      for (int k = 0; k < 9; ++k) A[k] = Rn[k];
#pragma unroll
      for (int k = 0; k < 3; ++k) A[9 + k] = ta[k] + w[k];
    }
  }
  float R0[9];
  quat_to_mat(s.root_quat, R0);
  if (lane < nl) {
    // the world pose: R = R0 A_R, p = R0 A_t (relative to the root origin)
    float R[9], p[3];
    matmul3(R0, A, R);
    matvec3(R0, A + 9, p);
#pragma unroll
    for (int k = 0; k < 9; ++k) s.R[lane][k] = R[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) s.p[lane][k] = p[k];
    if constexpr (kDyn) {
      const int i = lane;
      float cw[3];
      matvec3(R, m.com[i], cw);
      const float c[3] = {p[0] + cw[0], p[1] + cw[1], p[2] + cw[2]};
      d.c[i][0] = c[0]; d.c[i][1] = c[1]; d.c[i][2] = c[2];
      const float* Il = m.inertia[i];
      const float Im[9] = {Il[0], Il[3], Il[4], Il[3], Il[1], Il[5], Il[4], Il[5], Il[2]};
      const float Rt[9] = {R[0], R[3], R[6], R[1], R[4], R[7], R[2], R[5], R[8]};
      float T[9], Iw[9];
      matmul3(R, Im, T);
      matmul3(T, Rt, Iw);
      const float mass = m.mass[i], cc = dot3(c, c);
      float* B = d.Ib[i];
      B[0] = mass;
      B[1] = mass * c[0]; B[2] = mass * c[1]; B[3] = mass * c[2];
      B[4] = Iw[0] + mass * (cc - c[0] * c[0]);
      B[5] = Iw[4] + mass * (cc - c[1] * c[1]);
      B[6] = Iw[8] + mass * (cc - c[2] * c[2]);
      B[7] = Iw[1] - mass * c[0] * c[1];
      B[8] = Iw[2] - mass * c[0] * c[2];
      B[9] = Iw[5] - mass * c[1] * c[2];
      if (i > 0) {
        float a[3], o[3];
        matvec3(R, lc.ax, a);
        matvec3(R, lc.an, o);
        for (int k = 0; k < 3; ++k) o[k] += p[k];
        float S[6] = {a[0], a[1], a[2], 0.f, 0.f, 0.f};
        cross3(o, a, S + 3);
        const float qd = s.u[6 + i - 1];
        *reinterpret_cast<v4f*>(&s.S[6 + i - 1][0]) = v4f{S[0], S[1], S[2], S[3]};
        *reinterpret_cast<v4f*>(&s.S[6 + i - 1][4]) = v4f{S[4], S[5], 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < 6; ++k) d.Sq[i][k] = S[k] * qd;
      }
    }
  }
  if constexpr (kDyn) {
    if (lane == kZeroRow) {  // the walks' +0 rows (see take_bit_z)
      // (the zero in a VGPR: as a scalar constant it was hoisted out of the substep loop, an SGPR held across
      // every phase and spilled inside the loop)
      float z = 0.f;
      asm volatile("" : "+v"(z));
#pragma unroll
      for (int k = 0; k < 10; ++k) d.Ib[kZeroRow][k] = z;
#pragma unroll
      for (int k = 0; k < 6; ++k) d.Sq[kZeroRow][k] = z;
    }
  }
  if constexpr (kDyn) {
    // root columns need the root COM c0 = R0 com_0 (p_0 = 0): every lane forms it itself
    float c0[3];
    matvec3(R0, m.com[0], c0);
    if (lane < 3) s.c0[lane] = c0[lane];
    if (lane < 6) {
      float S[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      const int k = lane % 3;
      if (lane < 3) {
        S[3 + k] = 1.f;
      } else {
        float e[3] = {0.f, 0.f, 0.f};
        e[k] = 1.f;
        S[k] = 1.f;
        cross3(c0, e, S + 3);
      }
      *reinterpret_cast<v4f*>(&s.S[lane][0]) = v4f{S[0], S[1], S[2], S[3]};
      *reinterpret_cast<v4f*>(&s.S[lane][4]) = v4f{S[4], S[5], 0.f, 0.f};
    }
  }
  __syncthreads();
}

// Two-block f32 MFMA (v_mfma_f32_32x32x1_2b_f32): one 32 x 32 block per env (block b = lanes
// 32b..32b+31), K = 1 per instruction, lane l supplying A[l % 32][k] and B[k][l % 32] of its own env;
// the result is bit for bit an fmaf chain over k (scripts/probes/mfma_2b_probe.hip).  Register v of
// block b holds row 8(v/4) + 4h + v%4 on lane half h, column lane % 32; one v_permlane32_swap per
// register pair (blocks 0 and 1 trade halves) leaves lane n with column n of its own env's block.
typedef float f32x32 __attribute__((ext_vector_type(32)));
__device__ __forceinline__ void mfma_columns(const f32x32& acc, float (&col)[32]) {
#pragma unroll
  for (int v = 0; v < 16; ++v) {
    const auto p = __builtin_amdgcn_permlane32_swap(__float_as_int(acc[v]), __float_as_int(acc[16 + v]), false, false);
    const int r0 = 8 * (v >> 2) + (v & 3);
    col[r0] = __int_as_float(p[0]);
    col[r0 + 4] = __int_as_float(p[1]);
  }
}

// RNEA bias forces (qdd = 0) and composite inertias by path / subtree walks (lanes = links):
//   V_i  = V_0 + sum_{l on path, root->i} S_l qd_l            (= V_parent + S_i qd_i)
//   A_i  = A_0 + sum_{l on path} V_l x_m S_l qd_l             (= A_parent + V_i x S_i qd_i)
//   f_i  = I_i A_i + V_i x_f I_i V_i - gravity wrench
//   F_i  = sum_{l in subtree(i) (i included), ascending} f_l,  likewise Ic_i from the I_l
// The subtree sums are one matrix product per env on the matrix cores: with X the 16 x LMAX table of
// every link's (f, I) and M_il = [l in subtree(i)], the two-block f32 MFMA forms (X M^T) over LMAX K
// steps, an fmaf chain over l ascending from +0 for every (quantity, link) -- the root's row is the
// whole tree (oracle/physics.c subtree_sums restates the chain).  Then per dof j: C_j = S_j . F_link(j),
// b_j = tau_j - C_j (returned, also in LDS), Fh_j = Ic_link(j) S_j.
template <int NV>
__device__ __forceinline__ float dynamics(const Consts& K, EnvS& s, int lane, const Topo& tp, float gravity,
                                          float (&Sj)[6], float (&Fj)[6], int max_path) {
  const as_model_t& m = K.model;
  const int nl = m.num_links, nv = K.nv;
  DynScratch& d = s.x.d;
  float V[6], A[6];
  {
    const float* u = s.u;
    float wxc[3], vxw[3];
    cross3(s.c0, u + 3, wxc);
    cross3(u, u + 3, vxw);
    for (int k = 0; k < 3; ++k) {
      V[k] = u[3 + k];
      V[3 + k] = u[k] + wxc[k];
      A[k] = 0.f;
      A[3 + k] = vxw[k];
    }
  }
  if (lane < nl) {
    path_sum<6, 4>(tp.lpath & ~1u, max_path, V, d.Sq);
    if (lane > 0) {
      float Sq[6], cr[6];
#pragma unroll
      for (int k = 0; k < 6; ++k) Sq[k] = d.Sq[lane][k];
      crm(V, Sq, cr);
#pragma unroll
      for (int k = 0; k < 6; ++k) d.b.cr[lane][k] = cr[k];
    }
  }
  if (lane == kZeroRow) {  // the walks' +0 row (see take_bit_z); FK's Rl, which b aliases, is dead
    float z = 0.f;  // (a VGPR zero, as in fk)
    asm volatile("" : "+v"(z));
#pragma unroll
    for (int k = 0; k < 6; ++k) d.b.cr[kZeroRow][k] = z;
  }
  __syncthreads();
  float f[6], Ib[10];
  if (lane < nl) {
    path_sum<6, 4>(tp.lpath & ~1u, max_path, A, d.b.cr);
#pragma unroll
    for (int k = 0; k < 10; ++k) Ib[k] = d.Ib[lane][k];
    float IA[6], IV[6], x[6];
    inertia_mul(Ib, A, IA);
    inertia_mul(Ib, V, IV);
    crf(V, IV, x);
    const float mg[3] = {0.f, 0.f, Ib[0] * gravity};
    float cxmg[3];
    cross3(d.c[lane], mg, cxmg);
    for (int k = 0; k < 3; ++k) {
      f[k] = IA[k] + x[k] - cxmg[k];
      f[3 + k] = IA[3 + k] + x[3 + k] - mg[k];
    }
  }
  // every link's (f, I) into the transposed table; links past nl (and the lanes up to LMAX) add +0
  if (lane < LMAX) {
    const bool lv = lane < nl;
#pragma unroll
    for (int k = 0; k < 6; ++k) d.xt[k][lane & 1][lane >> 1] = lv ? f[k] : 0.f;
#pragma unroll
    for (int k = 0; k < 10; ++k) d.xt[6 + k][lane & 1][lane >> 1] = lv ? Ib[k] : 0.f;
  }
  __syncthreads();
  {
    // Both envs in one single-block v_mfma_f32_32x32x2_f32 (K = 2 per instruction, an fmaf chain over
    // its two K entries in order: scripts/probes/mfma_x2_probe.hip): row r = 16 env + quantity, column
    // = link i, instruction t takes link slots 2t (lanes 0-31) and 2t + 1 (lanes 32-63).  A operand:
    // lane l supplies X_env(r)[r % 16][2t + l / 32] (r = l % 32, the env's table in LDS); B operand:
    // lane l supplies M_{i, 2t + l / 32}, i = l % 32.  D row r, column i sits at register v of lane
    // half h with r = 8 (v / 4) + 4 h + v % 4: one v_permlane32_swap per register pair leaves lane
    // (env e, link i) with its 16 sums.
    const int tid = threadIdx.x, h = tid >> 5, r = tid & 31;
    EnvS* envs = &s - h;  // sm.env[0]
    const float* xr = envs[r >> 4].x.d.xt[r & 15][h];
    const uint32_t sub = (lane < nl ? tp.lsub : 0u) >> h;
    float xa[LMAX / 2];
    // the three 16-B reads issued together and passed through an empty asm (one wait): left to the
    // scheduler, each read reused the previous one's registers and waited under the MFMA chain
    static_assert(LMAX / 2 == 12, "three quads");
    v4f xq[3];
#pragma unroll
    for (int t = 0; t < 3; ++t) xq[t] = *reinterpret_cast<const v4f*>(xr + 4 * t);
    asm volatile("" : "+v"(xq[0]), "+v"(xq[1]), "+v"(xq[2]));
#pragma unroll
    for (int t = 0; t < 3; ++t) {
      xa[4 * t] = xq[t].x; xa[4 * t + 1] = xq[t].y; xa[4 * t + 2] = xq[t].z; xa[4 * t + 3] = xq[t].w;
    }
    typedef float f32x16 __attribute__((ext_vector_type(16)));
    f32x16 acc = {};
    // only the instructions that hold a link: num_links = NV - 5 (as_create: one hinge per non-root
    // link), and a slot past it adds +0 products to an accumulator that started at +0 -- the same bits
    // (the walker's 22 links use 11 of the 12 steps, the quadruped's 13 links 7)
    constexpr int kSubSteps = (NV - 5 + 1) / 2;
    static_assert(kSubSteps <= LMAX / 2, "link slots");
#pragma unroll
    for (int t = 0; t < kSubSteps; ++t)
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(xa[t], (float)((sub >> (2 * t)) & 1u), acc, 0, 0, 0);
    float col[16];
#pragma unroll
    for (int w = 0; w < 8; ++w) {
      const auto pr = __builtin_amdgcn_permlane32_swap(__float_as_int(acc[w]), __float_as_int(acc[8 + w]), false, false);
      const int q0 = 8 * (w >> 2) + (w & 3);
      col[q0] = __int_as_float(pr[0]);
      col[q0 + 4] = __int_as_float(pr[1]);
    }
    if (lane < nl) {  // lane i: F_i (0..5), Ic_i (6..15)
#pragma unroll
      for (int k = 0; k < 6; ++k) d.Sq[lane][k] = col[k];  // Sq is dead: F_i
#pragma unroll
      for (int k = 0; k < 10; ++k) d.Ic[lane][k] = col[6 + k];
    }
  }
  __syncthreads();
  float bj = 0.f;
  if (lane < nv) {
    const int j = lane;
    const int link = j < 6 ? 0 : j - 5;
    float F[6], Ic[10], S[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) F[k] = d.Sq[link][k];
#pragma unroll
    for (int k = 0; k < 10; ++k) Ic[k] = d.Ic[link][k];
#pragma unroll
    for (int k = 0; k < 6; ++k) S[k] = s.S[j][k];
    const float Cj = dot6(S, F);
    bj = (j < 6 ? 0.f : s.tau[j - 6]) - Cj;
    s.b[j] = bj;
    inertia_mul(Ic, S, Fj);
#pragma unroll
    for (int k = 0; k < 6; ++k) Sj[k] = S[k];
  } else {
    if (lane < 32) s.b[lane] = 0.f;
#pragma unroll
    for (int k = 0; k < 6; ++k) Sj[k] = Fj[k] = 0.f;
  }
  __syncthreads();
  return bj;
}

// Row j of the joint-space inertia H (lane j):
//   H_jk = S_k . (Ic_link(j) S_j)  if dof k is on the path of link(j) (k ancestor-or-self),
//        = S_j . (Ic_link(k) S_k)  if dof j is on the path of link(k),   else 0;  + armature.
// Every product P_kj = S_k . Fh_j (Fh_j = Ic_link(j) S_j) comes from six K steps of the two-block
// f32 MFMA (one block per env; A: lane k's S_k, B: lane j's Fh_j, both in registers from dynamics):
// P_kj is an fmaf chain over the six spatial components (oracle/physics.c chain6).  After the
// column shuffle lane j holds P_kj for every k: the path-side entries of its row.  Lane j publishes
// its row masked to its path, (k on path(j)) ? P_kj (+ armature on the diagonal) : +0, in LDS; the
// other side is the transposed entry of that matrix (lane k's P_jk for j on path(k)), one b32 read
// per column.  Lanes past NV read the all-zero padding column NV.
template <int NV>
__device__ __forceinline__ void h_row(EnvS& s, int lane, const Topo& tp, uint32_t anc_j, const float (&Sj)[6],
                                      const float (&Fj)[6], float (&Hr)[NV]) {
  static_assert(NV < LDJ, "padding column");
  // opaque per substep: the 27 column masks derived from it would otherwise be hoisted out of the
  // substep loop as SGPR pairs and spilled to VGPR lanes (a readlane per column per substep)
  asm volatile("" : "+v"(anc_j));
  const int j = lane < NV ? lane : 0;
  f32x32 acc = {};
#pragma unroll
  for (int a = 0; a < 6; ++a) acc = __builtin_amdgcn_mfma_f32_32x32x1f32(Sj[a], Fj[a], acc, 0, 0, 0);
  float col[32];
  mfma_columns(acc, col);
  const float arm = tp.arm;
  const uint32_t on = lane < NV ? anc_j : 0u;
#pragma unroll
  for (int k = 0; k < NV; ++k) {
    const float h = k == j ? col[k] + arm : col[k];
    Hr[k] = (on >> k) & 1u ? h : 0.f;
  }
  float(*M)[LDJ] = s.x.k.Jm;
  if (lane < NV) {
#pragma unroll
    for (int q = 0; q < LDJ / 4; ++q) {
      float e[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) e[c] = 4 * q + c < NV ? Hr[4 * q + c] : 0.f;
      *reinterpret_cast<v4f*>(&M[lane][4 * q]) = v4f{e[0], e[1], e[2], e[3]};
    }
  }
  // the root's six dofs are on every dof's path (ancmask bits 0-5, as_create), so their entries are
  // never taken from the transpose: those reads and selects are not issued (lanes >= NV keep the +0 of
  // the select above, as before)
  constexpr int kRootDofs = 6;
  const int jj = lane < NV ? lane : NV;
  float t[NV];
#pragma unroll
  for (int k = kRootDofs; k < NV; ++k) t[k] = M[k][jj];
  // (a register value, not a load: a select between two loads becomes a load from a selected
  // address, which puts Hr in scratch)
#pragma unroll
  for (int k = kRootDofs; k < NV; ++k) {
    asm volatile("" : "+v"(t[k]));
    Hr[k] = (on >> k) & 1u ? Hr[k] : t[k];
  }
}

// H^-1 by the block sweep operator on BxB pivot blocks, with column rotation (same arithmetic as
// oracle/physics.c sweep_inverse).  H is padded to an order NP (a multiple of B) with identity rows
// and columns.  Lane i holds row i in Hr, rotated so that the current pivot columns are always
// Hr[0..B-1]: a round shifts every row left by B and appends the B new pivot-column entries, so the
// register row is only indexed by compile-time constants, no per-column select is needed and (B
// even) pairs stay aligned for packed FMAs.  Round on pivots P = {p..p+B-1}, D = (H_PP)^-1:
//   the pivot lanes publish their rows without the pivot columns (Q) and H_PP (Pb);
//   every lane forms D (in-register sweep of the uniform BxB block);
//   row'_j = alpha row_j - sum_c beta_c Q_cj, new pivot-column entries = beta, with
//     (alpha, beta) = (1, a_iP D)  for i not in P   (a_ij - a_iP D a_Pj;  a_iP <- a_iP D)
//     (alpha, beta) = (0, -D_t)    for pivot lane t (D a_Pj;  a_PP <- -D).
// After all rounds the rotation is back to the identity and the rows hold -H^-1.
// 4x4 SPD inverse by 2x2 blocks (Schur complement): two 2x2 determinant inverses instead of four
// sequential pivots, so the chain on each sweep round's critical path is two divisions deep.
//   M = [A B; C D]:  Ai = A^-1, X = Ai B, Y = C Ai, S = D - C X, Si = S^-1,
//   M^-1 = [Ai + (X Si) Y, -(X Si); -(Si Y), Si]       (oracle/physics.c block_inverse: same order)
// The 2x2 blocks are kept as rows of packed pairs: a row of a product is one v_pk_mul + one
// v_pk_fma (per element the same mul and fmaf as the scalar form), the Schur difference and the
// final sum one v_pk_add each.
__device__ __forceinline__ void inv2(float a, float b, float c, float d, v2f (&o)[2]) {
  const float id = 1.0f / fmaf(a, d, -(b * c));
  o[0] = v2f{d, -b} * v2f{id, id};
  o[1] = v2f{-c, a} * v2f{id, id};
}
__device__ __forceinline__ void mul2(const v2f (&x)[2], const v2f (&y)[2], v2f (&o)[2]) {
#pragma unroll
  for (int i = 0; i < 2; ++i)
    o[i] = __builtin_elementwise_fma(v2f{x[i].y, x[i].y}, y[1], v2f{x[i].x, x[i].x} * y[0]);
}
template <int B>
__device__ __forceinline__ void block_inverse(float (&M)[B][B]) {  // M <- M^-1 (SPD)
  static_assert(B == 4, "2x2-block Schur inverse");
  const v2f A[2] = {v2f{M[0][0], M[0][1]}, v2f{M[1][0], M[1][1]}};
  const v2f Bm[2] = {v2f{M[0][2], M[0][3]}, v2f{M[1][2], M[1][3]}};
  const v2f C[2] = {v2f{M[2][0], M[2][1]}, v2f{M[3][0], M[3][1]}};
  const v2f D[2] = {v2f{M[2][2], M[2][3]}, v2f{M[3][2], M[3][3]}};
  v2f Ai[2], X[2], Y[2], CX[2], S[2], Si[2], XS[2], XSY[2], SY[2];
  inv2(A[0].x, A[0].y, A[1].x, A[1].y, Ai);
  mul2(Ai, Bm, X);
  mul2(C, Ai, Y);
  mul2(C, X, CX);
#pragma unroll
  for (int i = 0; i < 2; ++i) S[i] = D[i] - CX[i];
  inv2(S[0].x, S[0].y, S[1].x, S[1].y, Si);
  mul2(X, Si, XS);
  mul2(XS, Y, XSY);
  mul2(Si, Y, SY);
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const v2f top = Ai[i] + XSY[i];
    M[i][0] = top.x; M[i][1] = top.y;
    M[i][2] = -XS[i].x; M[i][3] = -XS[i].y;
    M[2 + i][0] = -SY[i].x; M[2 + i][1] = -SY[i].y;
    M[2 + i][2] = Si[i].x; M[2 + i][3] = Si[i].y;
  }
}

// The sweep's layout (include/as_detmath.h AS_SWEEP_PAD): the NV dofs padded to NP with identity rows /
// columns at padded index PAD, the NB = NP / 4 pivot blocks swept LAST block first (the limbs before the
// root).  A lane keeps ITS dof's row (lane k < NV: dof k, padded row padded(k); lane NV + q: pad row
// PAD + q), so no row moves between lanes; the columns start in the round-0 rotated order -- blocks
// NB - 1, NB - 2, ..., 0, natural order inside a block -- which the rotation below returns to after the
// last round.  SKIP bit r (NB - 1) + jb: in round r the pivot rows are exactly zero in column quad jb
// (as_create's structural check, sweep_skip_mask): that quad's update is the identity and is not issued
// (the pivot rows' zeros are +0 and stay +0, so every skipped fmaf would have returned its addend bit for
// bit; the oracle performs them).
template <int NV>
struct SweepLayout {
  static constexpr int NP = (NV + kSweepB - 1) / kSweepB * kSweepB;
  static constexpr int NB = NP / kSweepB;
  static constexpr int NQ = NB - 1;
  static constexpr int PAD = AS_SWEEP_PAD(NV);
  static constexpr int padded(int k) { return k < PAD ? k : k + (NP - NV); }
  static constexpr int pos(int P) { return (NB - 1 - P / kSweepB) * kSweepB + P % kSweepB; }  // round-0 register
};

// Software-pipelined and branch-free.  Every lane publishes its whole rotated row each round (no
// pivot-lane branch: the sweep is one basic block, so the scheduler can interleave across rounds), and
// its new leading quad -- the next round's pivot columns -- first: right after that store every lane
// reads the next pivot block back and inverts it, and the 4x4 inverse's division chain overlaps the
// round's remaining column updates instead of heading the next round.  Per element the operations
// and their order are those of oracle/physics.c sweep_inverse: only the issue order changes.
template <int NV, uint64_t SKIP>
__device__ void sweep_inverse(EnvS& s, int lane, float (&Hr)[SweepLayout<NV>::NP]) {
  typedef SweepLayout<NV> L;
  constexpr int NP = L::NP, NB = L::NB, NQ = L::NQ, B = kSweepB;
  static_assert(B == 4, "16-B pivot rows");
  static_assert(NP <= 28, "row buffer stride");
  static_assert(NQ * NB <= 64, "skip mask bits");
  // this lane's padded row
  const int prow = lane < NV ? (lane < L::PAD ? lane : lane + (NP - NV)) : (lane < NP ? L::PAD + (lane - NV) : lane);
  // LDS operations of a wave complete in issue order: a round's stores cannot overtake the previous
  // round's reads of the same rows.  Explicit 16-B accesses on a native 4-vector type (float4 is a
  // struct whose copies SROA splits into b96 + b32 pairs)
  float(*Rw)[28] = s.x.sw.rows;
  v4f* own = reinterpret_cast<v4f*>(Rw[prow]);
  // a row quad is stored only if the next round reads it: round r reads quad jb of its pivot rows
  // unless SKIP says those are +0 (the rows are LDS scratch, dead after the sweep)
#pragma unroll
  for (int j = 0; j < NP; j += 4)
    if (j == 0 || !((SKIP >> (j / 4 - 1)) & 1ull)) own[j / 4] = v4f{Hr[j], Hr[j + 1], Hr[j + 2], Hr[j + 3]};
  __syncthreads();
  float D[B][B];
#pragma unroll
  for (int a = 0; a < B; ++a) {
    const v4f d = *reinterpret_cast<const v4f*>(Rw[(NB - 1) * B + a]);
    D[a][0] = d.x; D[a][1] = d.y; D[a][2] = d.z; D[a][3] = d.w;
  }
  block_inverse<B>(D);
  // unrolled over the rounds: the column rotation is then register renaming and the pivot lanes /
  // padding / skipped quads are known per round
#pragma unroll
  for (int r = 0; r < NB; ++r) {
    const int p = (NB - 1 - r) * B;  // the pivot block's padded rows
    const int t = prow - p;
    const bool piv = (unsigned)t < (unsigned)B;
    // the pivot rows' other columns (stored last round, or above for r = 0); a skipped quad's are
    // never read
    v4f x[NQ][B];
#pragma unroll
    for (int jb = 0; jb < NQ; ++jb)
#pragma unroll
      for (int c = 0; c < B; ++c)
        if (!((SKIP >> (r * NQ + jb)) & 1ull)) x[jb][c] = *reinterpret_cast<const v4f*>(&Rw[p + c][B + 4 * jb]);
    // packed pairs written out (the file is built without the SLP vectorizer, which elsewhere paid
    // for its pairs with register moves); per element the same operations in the same order
    float alpha = 1.f, beta[B];
    v2f vb[B / 2] = {v2f{0.f, 0.f}, v2f{0.f, 0.f}};
#pragma unroll
    for (int e = 0; e < B; ++e)
#pragma unroll
      for (int c2 = 0; c2 < B / 2; ++c2)
        vb[c2] = __builtin_elementwise_fma(v2f{Hr[e], Hr[e]}, v2f{D[e][2 * c2], D[e][2 * c2 + 1]}, vb[c2]);
#pragma unroll
    for (int c = 0; c < B; ++c) {
      const float v = c & 1 ? vb[c / 2].y : vb[c / 2].x;
      float pv = -D[0][c];
#pragma unroll
      for (int e = 1; e < B; ++e) pv = t == e ? -D[e][c] : pv;
      beta[c] = piv ? pv : v;
    }
    if (piv) alpha = 0.f;
    float Dn[B][B];
#pragma unroll
    for (int jb = 0; jb < NQ; ++jb) {
      const int j = B + 4 * jb;
      v2f lo, hi;
      if ((SKIP >> (r * NQ + jb)) & 1ull) {
        // the pivot rows are +0 in this quad: alpha a - sum (+-0) = a, for the pivot lanes too (their
        // own entries here are those +0)
        lo = v2f{Hr[j], Hr[j + 1]};
        hi = v2f{Hr[j + 2], Hr[j + 3]};
      } else {
        lo = v2f{alpha, alpha} * v2f{Hr[j], Hr[j + 1]};
        hi = v2f{alpha, alpha} * v2f{Hr[j + 2], Hr[j + 3]};
#pragma unroll
        for (int c = 0; c < B; ++c) {
          lo = __builtin_elementwise_fma(v2f{-beta[c], -beta[c]}, x[jb][c].xy, lo);
          hi = __builtin_elementwise_fma(v2f{-beta[c], -beta[c]}, x[jb][c].zw, hi);
        }
      }
      Hr[j - B] = lo.x; Hr[j + 1 - B] = lo.y; Hr[j + 2 - B] = hi.x; Hr[j + 3 - B] = hi.y;
      if (jb == 0 && r + 1 < NB) {
        // the next round's pivot block (padded rows p - B ..): published, read back and inverted under
        // the rest of the round
        own[0] = v4f{lo.x, lo.y, hi.x, hi.y};
        __builtin_amdgcn_wave_barrier();  // one wave: the store above reaches LDS before these reads
#pragma unroll
        for (int a = 0; a < B; ++a) {
          const v4f d = *reinterpret_cast<const v4f*>(Rw[p - B + a]);
          Dn[a][0] = d.x; Dn[a][1] = d.y; Dn[a][2] = d.z; Dn[a][3] = d.w;
        }
        block_inverse<B>(Dn);
      }
    }
#pragma unroll
    for (int c = 0; c < B; ++c) Hr[NP - B + c] = beta[c];
    if (r + 1 < NB) {
#pragma unroll
      for (int j = B; j < NP; j += 4)
        if (!((SKIP >> ((r + 1) * NQ + j / 4 - 1)) & 1ull)) own[j / 4] = v4f{Hr[j], Hr[j + 1], Hr[j + 2], Hr[j + 3]};
      __builtin_amdgcn_wave_barrier();
#pragma unroll
      for (int a = 0; a < B; ++a)
#pragma unroll
        for (int c = 0; c < B; ++c) D[a][c] = Dn[a][c];
    }
  }
  __syncthreads();
}

}  // namespace as
