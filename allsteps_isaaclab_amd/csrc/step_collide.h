// step_collide.h -- the contact search of a substep: robot geoms against the stone boxes, and geom self pairs.
// Reads EnvS R, p, stones and root_pos; writes the candidate stones (cand), the contact list (cpt, cn, csep,
// clink, clink2, cstone, cfoot), ndrop and its scratch x.col.  Returns the env's contact count.
#pragma once

#include <hip/hip_runtime.h>

#include "allsteps_pair_group.h"
#include "step_lanes.h"
#include "step_scratch.h"

namespace as {

// ------------------------------------------------------------------------------------------------
// contacts: robot geoms vs axis-aligned stone boxes

__device__ void emit_contact(EnvS& s, int slot, int ncap, int link, int link2, int stone, int foot, const float* P,
                             const float* n, float sep, float r) {
  if (slot >= ncap) return;
  s.clink[slot] = link; s.clink2[slot] = link2; s.cstone[slot] = stone; s.cfoot[slot] = foot; s.csep[slot] = sep;
  for (int k = 0; k < 3; ++k) { s.cn[slot][k] = n[k]; s.cpt[slot][k] = P[k] - n[k] * r; }
}

// Per-lane constants read from the lane table (allsteps_lane_table.h) once per launch and kept in
// registers across the substeps (lane-varying global loads every substep were an L2 round trip at the
// head of collide and of the H rows): the geom of lane g, and the H-row masks of dof lane j.
struct GeomC {
  int link, type, foot;
  float r, p0[3], p1[3];
  uint32_t anc;  // h_row: dofs on the path of dof j's link
};
// as_capsule_contact (include/as_detmath.h) without branches: every lane forms the three quotients of
// the main path (s, then t, then the clamped-end s) and selects; the degenerate cases (a sphere: a or e
// <= eps) reuse the same quotients with their own numerators.  The values selected are the same
// operations on the same operands as the branchy form, so the same bits; a wave whose pairs take
// different branches runs three divisions instead of up to six.
__device__ __forceinline__ float capsule_contact_sel(const float* a1, const float* b1, float r1, const float* a2,
                                                     const float* b2, float r2, float* P, float* n) {
  float d1[3], d2[3], r[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    d1[k] = b1[k] - a1[k];
    d2[k] = b2[k] - a2[k];
    r[k] = a1[k] - a2[k];
  }
  const float a = as_dot3(d1, d1), e = as_dot3(d2, d2), f = as_dot3(d2, r);
  const float eps = 1e-12f;
  const bool pa = a <= eps, pe = e <= eps, gen = !pa && !pe;
  const float c = as_dot3(d1, r);
  const float b = as_dot3(d1, d2);
  const float den = fmaf(a, e, -(b * b));
  const float sm = den > 0.f ? as_clamp01(fmaf(b, f, -(c * e)) / den) : 0.f;
  const float tq = (pa ? f : fmaf(b, sm, f)) / e;
  const bool lo = gen && tq < 0.f, hi = gen && tq > 1.f;
  const float sq = as_clamp01((hi ? b - c : -c) / a);
  const float s = pa ? 0.f : (pe || lo || hi) ? sq : sm;
  const float t = pa ? (pe ? 0.f : as_clamp01(tq)) : pe ? 0.f : lo ? 0.f : hi ? 1.f : tq;
  float c1[3], c2[3], w[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    c1[k] = fmaf(s, d1[k], a1[k]);
    c2[k] = fmaf(t, d2[k], a2[k]);
    w[k] = c1[k] - c2[k];
  }
  const float dist = sqrtf(as_dot3(w, w));
  const bool nz = dist > 1e-9f;
  const float inv = 1.0f / dist;
  n[0] = nz ? w[0] * inv : 0.f;
  n[1] = nz ? w[1] * inv : 0.f;
  n[2] = nz ? w[2] * inv : 1.f;
  const float sep = dist - r1 - r2;
  const float off = fmaf(0.5f, sep, r2);
#pragma unroll
  for (int k = 0; k < 3; ++k) P[k] = fmaf(off, n[k], c2[k]);
  return sep;
}

// At most ncap contacts, in priority order (oracle/physics.c collide() emits the same list); every
// pair is still tested past the cap, and the contacts found beyond it are counted in s.ndrop:
//   1. the priority geoms (the feet: geoms [0, num_priority_geoms)) against the candidate stones,
//      stone-major, geom-minor;  2. every other geom against the candidate stones, likewise;
//   3. robot self-contacts, one per self-collision pair in table order.
// gcap: the largest pass-B group level (Consts::pair_group_cap); ts: the diagnostic pair / level counts.
template <class TS>
__device__ __forceinline__ int collide(const Consts& K, EnvS& s, int lane, int ncap, const GeomC& gc, const float* h,
                                       float margin, int gcap, TS& ts) {
  const as_model_t& m = K.model;
  const int nst = K.task.num_steps, ng = m.num_geoms, npri = m.num_priority_geoms, nsp = m.num_self_pairs;
  // self-collision pair words of this lane (pairs lane, lane + 32, ...), loaded first so that their
  // latency hides behind the stone contacts
  constexpr int kSelfW = AS_MAX_SELF_PAIRS / G;
  int spw[kSelfW];
#pragma unroll
  for (int i = 0; i < kSelfW; ++i) spw[i] = G * i + lane < nsp ? m.self_pair[G * i + lane] : 0;
  // geom segment in the O frame (lane = geom), formed once for all candidate stones
  const bool gv = lane < ng;
  const int link = gc.link, gtype = gc.type, foot = gc.foot;
  const float r = gc.r;
  float a[3], bb[3];
  {
    float t0[3], t1[3];
    matvec3(s.R[link], gc.p0, t0);
    matvec3(s.R[link], gc.p1, t1);
    for (int k = 0; k < 3; ++k) { a[k] = s.p[link][k] + t0[k]; bb[k] = s.p[link][k] + t1[k]; }
  }
  const float L = sqrtf((bb[0] - a[0]) * (bb[0] - a[0]) + (bb[1] - a[1]) * (bb[1] - a[1]) +
                        (bb[2] - a[2]) * (bb[2] - a[2]));
  const float mid[3] = {0.5f * (a[0] + bb[0]), 0.5f * (a[1] + bb[1]), 0.5f * (a[2] + bb[2])};
  // broadphase (lane = stone): stone boxes that come within the contact margin of the robot's
  // bounding box (union of the geoms' boxes).  Conservative: every pair the narrowphase would
  // turn into a contact survives, so the contact set and order match the oracle's.
  // the six extents reduced in three pairs, the maxima as minima of the negated values (exact)
  float blo[3], bhi[3], ext[6];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const float e = gtype == 0 ? a[k] : fminf(a[k], bb[k]);
    const float f = gtype == 0 ? a[k] : fmaxf(a[k], bb[k]);
    ext[k] = gv ? e - r : 1e30f;
    ext[3 + k] = gv ? -(f + r) : 1e30f;
  }
  half_min_n(ext);
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    blo[k] = ext[k] - margin;
    bhi[k] = -ext[3 + k] + margin;
  }
  bool isc = false;
  float cst[3] = {0.f, 0.f, 0.f};
  if (lane < nst) {
    isc = true;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      cst[k] = s.stones[3 * lane + k] - s.root_pos[k];
      isc = isc && (cst[k] - h[k] <= bhi[k]) && (cst[k] + h[k] >= blo[k]);
    }
  }
  uint64_t bal = __ballot(isc);
  const int half = (threadIdx.x >> 5) & 1;
  uint32_t mine = (uint32_t)(bal >> (32 * half));
  if (isc) {
    const int pos = __popc(mine & ((1u << lane) - 1u));
    s.cand[pos] = lane;
    // the candidate's relative center for pass A (one 16-B broadcast read per candidate there)
    *reinterpret_cast<v4f*>(s.x.col.cc[pos]) = v4f{cst[0], cst[1], cst[2], 0.f};
  }
  const int ncand = __popc(mine);
  // narrowphase in two passes.  (A) lane = geom, loop over the candidate stones (once for the
  // priority geoms, once for the rest): the cheap bounding test (spheres: the exact separation)
  // appends the surviving (stone, geom) pairs to a list in LDS, in emission order.  (B) lane = pair,
  // in chunks of kPairsPerChunk: the exact test (capsules: slope bisection for the segment's closest
  // point) and the contacts, emitted in list order by a prefix sum.  A chunk is flushed as soon as
  // either env of the wave has kPairsPerChunk pairs pending, by both envs together (the other one
  // flushes its partial list: chunk boundaries change neither the contacts nor their order, and one
  // flush for the wave replaces one per env under divergence), so the list never exceeds 32 + 22
  // entries; the search runs over every pair even past ncap contacts (the surplus is counted, not
  // emitted).  When the wave's larger pending count is at most 8 -- nearly always: the last flush of a
  // substep -- a pair gets a group of lanes instead of one (flush_grp below).
  {
    float* gs = s.x.col.g[lane];  // staging of this lane's geom for pass B and the self pairs
    if (gv) {
      gs[0] = a[0]; gs[1] = a[1]; gs[2] = a[2];
      gs[3] = bb[0]; gs[4] = bb[1]; gs[5] = bb[2];
      gs[6] = r;
      gs[7] = __int_as_float(gtype | ((foot + 1) << 4) | (link << 8));
      *reinterpret_cast<v4f*>(s.x.col.bs[lane]) = v4f{mid[0], mid[1], mid[2], 0.5f * L + r};
    }
  }
  int* pl = s.x.col.pl;
  int pend = 0, base = 0;
  auto flush = [&](int npairs) {  // pass B over pl[0, npairs) (npairs <= kPairsPerChunk), shift the rest
    int cnt = 0, plink = 0, pst = 0, pfoot = -1;
    float P0[3], N0[3], P1[3], N1[3], P2[3], N2[3], SEP0 = 0.f, SEP1 = 0.f, SEP2 = 0.f, pr = 0.f;
    const bool act = lane < npairs;
    const int e = act ? pl[lane] : 0;  // (an env with nothing pending flushes too: stone 0, geom 0)
    const int gi = e & 0xff;
    pst = e >> 8;
    const float* gq = s.x.col.g[gi];
    const float A[3] = {gq[0], gq[1], gq[2]}, Bb[3] = {gq[3], gq[4], gq[5]};
    pr = gq[6];
    const int meta = __float_as_int(gq[7]);
    const int pty = meta & 15;
    pfoot = ((meta >> 4) & 15) - 1;
    plink = meta >> 8;
    float c[3];
    for (int k = 0; k < 3; ++k) c[k] = s.stones[3 * pst + k] - s.root_pos[k];
    // capsule: minimum of the (convex) signed distance along the segment by bisection on the sign
    // of its slope.  Runs for every lane (the result is only used by capsule pairs); unrolled by 4
    // (by 2: +0.6 % step time, profiles/r06z7_ab_flush_unroll.log).
    float lo = 0.f, hi = 1.f;
#pragma unroll 4
    for (int it = 0; it < kBisectIters; ++it) {
      const float t = 0.5f * (lo + hi);
      const bool up = sd_box_slope(A, Bb, t, c, h) > 0.f;
      hi = up ? t : hi;
      lo = up ? lo : t;
    }
    if (act) {
      // the segment's first point: the sphere's test and the capsule's t = 0 end are the same value
      float n0[3];
      const float s0 = sd_box(A, c, h, n0) - pr;
      if (pty == 0) {
        if (s0 < margin) {
          for (int k = 0; k < 3; ++k) { P0[k] = A[k]; N0[k] = n0[k]; }
          SEP0 = s0;
          cnt = 1;
        }
      } else {
        float n1[3];
        float s1 = sd_box(Bb, c, h, n1) - pr;
        float ts = 0.5f * (lo + hi), Ps[3], ns[3];
        for (int k = 0; k < 3; ++k) Ps[k] = A[k] + ts * (Bb[k] - A[k]);
        float ss = sd_box(Ps, c, h, ns) - pr;
        bool e0 = s0 < margin, e1 = s1 < margin;
        bool es = ss < margin && ss < fminf(s0, s1) - 0.002f;
        // pack the emitted contacts in (t=0, t=1, t*) order into slots 0..2
        for (int k = 0; k < 3; ++k) { P0[k] = A[k]; N0[k] = n0[k]; }
        SEP0 = s0;
        if (e0) {
          for (int k = 0; k < 3; ++k) { P1[k] = Bb[k]; N1[k] = n1[k]; P2[k] = Ps[k]; N2[k] = ns[k]; }
          SEP1 = s1; SEP2 = ss;
          if (!e1) { for (int k = 0; k < 3; ++k) { P1[k] = Ps[k]; N1[k] = ns[k]; } SEP1 = ss; }
        } else {
          for (int k = 0; k < 3; ++k) { P0[k] = Bb[k]; N0[k] = n1[k]; P1[k] = Ps[k]; N1[k] = ns[k]; }
          SEP0 = s1; SEP1 = ss;
          if (!e1) { for (int k = 0; k < 3; ++k) { P0[k] = Ps[k]; N0[k] = ns[k]; } SEP0 = ss; }
        }
        cnt = (int)e0 + (int)e1 + (int)es;
      }
    }
    int total;
    const int slot = base + half_scan3(cnt, total);
    if (cnt > 0) emit_contact(s, slot, ncap, plink, -1, pst, pfoot, P0, N0, SEP0, pr);
    if (cnt > 1) emit_contact(s, slot + 1, ncap, plink, -1, pst, pfoot, P1, N1, SEP1, pr);
    if (cnt > 2) emit_contact(s, slot + 2, ncap, plink, -1, pst, pfoot, P2, N2, SEP2, pr);
    base += total;
    // shift the unprocessed tail (< 32 entries) to the front
    const int rest = pend - npairs;
    const int tail = lane < rest ? pl[npairs + lane] : 0;
    __syncthreads();
    if (lane < rest) pl[lane] = tail;
    pend = rest;
    __syncthreads();
  };
  // Pass B with a group of 2^L lanes per pair (L = 2, 3, 4: pair p at lanes p << L, npairs <= 32 >> L),
  // entered by the whole wave.  A flush above is one lane's serial instruction stream whatever the pair
  // count, and a substep has 1.5 pairs on average; here the idle lanes take that stream
  // apart.  Every value keeps its operations and operands, so the contacts are the same bits:
  //  - the bisection runs L rounds at once (allsteps_pair_group.h): sub-lane k evaluates the slope at its
  //    dyadic point, one ballot hands the group's signs to every lane, each lane walks the L decisions;
  //  - sub-lanes 0, 1, 2 evaluate sd_box at A, at B and at P(t*): one instance in the stream, not three,
  //    and each holds at most one contact.  Lane order within the half is then the emission order
  //    (pair-major; t = 0, t = 1, t*), so the prefix count over lanes gives the slots and one
  //    emit_contact per lane replaces the packing selects and three conditional calls.
  // A sphere pair uses sub-lane 0 only.  L is a runtime value: one copy of the code for the three levels.
  auto flush_grp = [&](int npairs, int L) {
    const int gm = (1 << L) - 1, k = lane & gm, pi = lane >> L;
    const bool act = pi < npairs;
    const int e = act ? pl[pi] : 0;  // (a group without a pair runs on stone 0, geom 0 and emits nothing)
    const int gi = e & 0xff, pst = e >> 8;
    const float* gq = s.x.col.g[gi];
    const float A[3] = {gq[0], gq[1], gq[2]}, Bb[3] = {gq[3], gq[4], gq[5]};
    const float pr = gq[6];
    const int meta = __float_as_int(gq[7]);
    const int pty = meta & 15, pfoot = ((meta >> 4) & 15) - 1, plink = meta >> 8;
    float c[3];
    for (int i = 0; i < 3; ++i) c[i] = s.stones[3 * pst + i] - s.root_pos[i];
    float lo = 0.f, d = 1.f;  // the interval [lo, lo + d]
    const float sc = pair_group_scale(L);
    const int g0 = (threadIdx.x & 63) & ~gm;  // the group's first lane in the wave
#pragma unroll 1
    for (int it = 0; it < kBisectIters; it += L) {
      const float w = d * sc;
      const bool up = sd_box_slope(A, Bb, pair_group_point(lo, w, k), c, h) > 0.f;
      pair_group_walk(lo, w, L, (uint32_t)(__ballot(up) >> g0));  // reads the group's bits 0 .. 2^L - 2
      d = w;
    }
    const float tm = 0.5f * (lo + (lo + d));
    float Q[3], nq[3];
    // (P(t*) formed by every lane, and the sub-lane's point picked by bit masks -- two v_bfi per
    // coordinate: written as ?: the compiler turns each pick into exec-mask diamonds on k; the emission
    // test below in bit operations for the same reason)
    const uint32_t m0 = k == 0 ? ~0u : 0u, m1 = k == 1 ? ~0u : 0u;
    for (int i = 0; i < 3; ++i) {
      const uint32_t ps = __float_as_uint(A[i] + tm * (Bb[i] - A[i]));
      const uint32_t b1 = (__float_as_uint(Bb[i]) & m1) | (ps & ~m1);
      Q[i] = __uint_as_float((__float_as_uint(A[i]) & m0) | (b1 & ~m0));
    }
    const float sv = sd_box(Q, c, h, nq) - pr;
    // sub-lane 2: min(s0, s1) from its two neighbours (row_shr:2, row_shr:1; a group never straddles a row).
    // On sub-lanes 0 and 1 the shifts reach into the previous group, or past the row's start where
    // bound_ctrl gives 0: smin is read on sub-lane 2 alone (sel below), the rest is discarded.
    const float smin = fminf(dpp<0x112>(sv), dpp<0x111>(sv));
    const bool cap = pty != 0;
    const bool sel = (k == 0) | (cap & (k == 1)) | (cap & (k == 2) & (sv < smin - 0.002f));
    const int cnt = (int)(act & (sv < margin) & sel);
    int total;
    const int slot = base + half_scan3(cnt, total);
    if (cnt) emit_contact(s, slot, ncap, plink, -1, pst, pfoot, Q, nq, sv, pr);
    base += total;
    pend -= npairs;  // (the level was chosen to hold every pending pair: nothing to shift)
    __syncthreads();
  };
  static_assert(kBisectIters == kPairGroupIters, "allsteps_pair_group.h: the group rounds cover kBisectIters");
  // wave-uniform: the group level for the wave's larger pending count, and the flush that goes with it
  auto flush_any = [&](int wpend) {
    const int L = pair_group_level(wpend, gcap);
    const int np = pend < kPairsPerChunk ? pend : kPairsPerChunk;
    ts.pairs(np, L);
    if (L) flush_grp(np, L); else flush(np);
  };
  __syncthreads();
  // pass A (lane = geom): one bounding test per (candidate stone, geom), kept as a per-stone mask of
  // the surviving geoms; the masks then become the pair list class by class (feet first),
  // stone-major, geom-minor
  uint32_t* cneed = s.x.col.need;
  const float pa[3] = {gtype == 0 ? a[0] : mid[0], gtype == 0 ? a[1] : mid[1], gtype == 0 ? a[2] : mid[2]};
  const float cap_lim = 0.5f * L + r + margin;
#pragma unroll 1
  for (int ci = 0; ci < ncand; ++ci) {
    const v4f cv = *reinterpret_cast<const v4f*>(s.x.col.cc[ci]);
    const float c[3] = {cv.x, cv.y, cv.z};
    float nr[3];
    // one distance per lane: the sphere's center, or the capsule's midpoint for its bounding test
    const float sd = sd_box(pa, c, h, nr);
    bool need = false;
    if (gv) need = gtype == 0 ? sd - r < margin : sd <= cap_lim;
    const uint32_t bl = (uint32_t)(__ballot(need) >> (32 * half));
    if (lane == 0) cneed[ci] = bl;
  }
  __syncthreads();
  const uint32_t primask = npri >= 32 ? ~0u : (1u << npri) - 1u;
  const int wcand = max(__builtin_amdgcn_readlane(ncand, 0), __builtin_amdgcn_readlane(ncand, 32));
  // Classes 0 and 1 append the pairs; "class" 2 is one empty round that appends nothing and flushes what is
  // left, so that pass B has one call site (one copy of flush / flush_grp in the code) instead of a second
  // one behind the loops.
#pragma unroll 1
  for (int cls = 0; cls < 3; ++cls) {
    const int nci = cls < 2 ? wcand : 1;
#pragma unroll 1
    for (int ci = 0; ci < nci; ++ci) {
      const uint32_t bl = cls < 2 && ci < ncand ? cneed[ci] & (cls == 0 ? primask : ~primask) : 0u;
      if ((bl >> lane) & 1u) pl[pend + __popc(bl & ((1u << lane) - 1u))] = (s.cand[ci] << 8) | lane;
      pend += __popc(bl);  // no barrier: the single wave's LDS operations complete in issue order
      // wave-uniform flush decision (see above); the candidate loop runs to the wave's larger count
      const int wpend = max(__builtin_amdgcn_readlane(pend, 0), __builtin_amdgcn_readlane(pend, 32));
      // while appending: a full chunk; in the closing round: whatever is pending (fewer than kPairsPerChunk
      // in either env, since every full chunk was flushed as it filled: exactly one flush, of everything)
      const bool appending = cls < 2;
      if (appending ? wpend >= kPairsPerChunk : wpend > 0) flush_any(wpend);
    }
  }
  // self-contacts.  (A) lane = pair: the bounding-sphere filter; the surviving pairs are appended to
  // the pending list in table order.  (B) lane = pending pair, in chunks of G: the capsule-capsule
  // closest points (capsule_contact_sel: as_detmath.h's as_capsule_contact, which the oracle runs, in
  // selects), emitted in list order.
  pend = 0;
  auto flush_self = [&](int npairs) {
    const bool act = lane < npairs;
    const int e = pl[act ? lane : 0];
    const int g1 = e & 0xff, g2 = e >> 8;
    int cnt = 0, l1 = 0, l2 = 0;
    float P[3], n[3], sep = 0.f;
    if (act) {
      const float* q1 = s.x.col.g[g1];
      const float* q2 = s.x.col.g[g2];
      sep = capsule_contact_sel(q1, q1 + 3, q1[6], q2, q2 + 3, q2[6], P, n);
      cnt = sep < margin;
      l1 = __float_as_int(q1[7]) >> 8;
      l2 = __float_as_int(q2[7]) >> 8;
    }
    int total;
    const int slot = base + half_scan3(cnt, total);
    if (cnt) emit_contact(s, slot, ncap, l1, l2, -1, -1, P, n, sep, 0.f);
    base += total;
    const int rest = pend - npairs;
    const int tail = lane < rest ? pl[npairs + lane] : 0;
    __syncthreads();
    if (lane < rest) pl[lane] = tail;
    pend = rest;
    __syncthreads();
  };
  // all filter tests first (their LDS reads overlap), then the list is appended to without a
  // barrier per word (LDS operations of the single wave complete in issue order)
  // Every lane reads both spheres of every word (a word past nsp reads geom 0's twice: spw = 0) and
  // the reads are passed through an empty asm, four words at a time: each batch waits once.  (With
  // `pv && test` the compiler put each word's reads behind a branch on pv and waited on them word by
  // word: one LDS latency per word.)
  // Batches past the table (the quadruped's 66 pairs fill one of the two) are skipped by a scalar
  // branch; their words stay empty.
  uint32_t hbl[kSelfW];
  static_assert(kSelfW % 4 == 0, "batches of four words");
#pragma unroll
  for (int i = 0; i < kSelfW; ++i) hbl[i] = 0u;
#pragma unroll
  for (int i0 = 0; i0 < kSelfW; i0 += 4) {
    if (G * i0 >= nsp) break;
    v4f s1[4], s2[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      s1[i] = *reinterpret_cast<const v4f*>(s.x.col.bs[spw[i0 + i] & 0xff]);
      s2[i] = *reinterpret_cast<const v4f*>(s.x.col.bs[spw[i0 + i] >> 8]);
    }
    asm volatile("" : "+v"(s1[0]), "+v"(s1[1]), "+v"(s1[2]), "+v"(s1[3]), "+v"(s2[0]), "+v"(s2[1]), "+v"(s2[2]),
                 "+v"(s2[3]));
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const bool pv = G * (i0 + i) + lane < nsp;
      const float m1[3] = {s1[i].x, s1[i].y, s1[i].z}, m2[3] = {s2[i].x, s2[i].y, s2[i].z};
      const bool hit = as_sphere_bound(m1, s1[i].w, m2, s2[i].w, margin);
      hbl[i0 + i] = (uint32_t)(__ballot(pv & hit) >> (32 * half));
    }
  }
  // The survivors' list positions in table order (word-major, lane-minor) by prefix counts, and all
  // of them written at once when neither env has more than the list holds (64; a random-action run
  // has 7 on average, 31 at p99.9: DESIGN §4), then tested 32 at a time -- the same chunks and
  // contact order as appending word by word.  More survivors: word by word, flushing every 32.
  const uint32_t lt = (1u << lane) - 1u;
  int tot = 0, at[kSelfW];
#pragma unroll
  for (int i = 0; i < kSelfW; ++i) {
    at[i] = tot + __popc(hbl[i] & lt);
    tot += __popc(hbl[i]);
  }
  if (max(__builtin_amdgcn_readlane(tot, 0), __builtin_amdgcn_readlane(tot, 32)) <= 64) {
#pragma unroll
    for (int i = 0; i < kSelfW; ++i)
      if ((hbl[i] >> lane) & 1u) pl[at[i]] = spw[i];
    pend = tot;
    while (pend > 0) flush_self(pend < G ? pend : G);
  } else {
    // a rolled loop (one copy of flush_self: code size is instruction-cache footprint); word i of
    // the register arrays by a select chain
#pragma unroll 1
    for (int i = 0; i < kSelfW; ++i) {
      if (G * i >= nsp) break;
      uint32_t bl = hbl[0];
      int w = spw[0];
#pragma unroll
      for (int k = 1; k < kSelfW; ++k) {
        bl = i == k ? hbl[k] : bl;
        w = i == k ? spw[k] : w;
      }
      if ((bl >> lane) & 1u) pl[pend + __popc(bl & lt)] = w;
      pend += __popc(bl);
      if (pend >= G) flush_self(G);
    }
    if (pend > 0) flush_self(pend);
  }
  // the search runs to the end: contacts past the cap are found, not emitted, and counted
  if (lane == 0 && base > ncap) s.ndrop += base - ncap;
  __syncthreads();
  return base < ncap ? base : ncap;  // uniform over the env's half-wave
}

}  // namespace as
