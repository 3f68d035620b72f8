// allsteps_consts.h -- the constants block of the step kernels and everything the host derives for it:
// the model checks, the tree plan every tree pass of k_step trusts, and the structural H^-1 sweep.
//
// Plain C++ with no HIP dependency: a host program can build and check the plan (tests/tree_plan_check.cpp).
// as_create and as_sweep_plan (allsteps_abi.hip) are the callers; the kernels only read Consts.
#pragma once

#include <stdint.h>

#include <algorithm>
#include <string>

#include "../../include/allsteps.h"
#include "../../include/as_detmath.h"  // AS_SWEEP_PAD (under hipcc its AS_HD wants hip_runtime.h first: allsteps_kernels.h)
#include "allsteps_lane_table.h"

#define AS_MAX_RAYS 1024  // rays of one as_ray_cast call (a ray-caster sensor's pattern)

namespace as {

constexpr int kMaxLinks = 24;  // LDS sizing of the step kernel (walker: 22 links)
constexpr int kMaxDofs = 6 + kMaxLinks - 1;
constexpr int kSweepB = 4;        // pivot block of the H^-1 sweep

// Everything the kernels read that does not change per step: model tables + the tree plan
// derived from them on the host.  The plan is bitmasks over links / dofs: every tree pass of the
// step kernel is a walk over one lane's own ancestor path or subtree (no level barriers), and
// each lane keeps its own masks in registers for the whole launch.
struct Consts {
  as_model_t model;
  as_sim_t sim;
  as_task_t task;
  as_actuator_t act;               // as_set_actuator (mode AS_ACT_TORQUE after as_create)
  as_quad_task_t quad;             // as_set_quad_task (BASELINE C5)
  int32_t nv;
  int32_t st_has_hind;             // the state carries contact_mask_hind (sensors 2, 3)
  int32_t max_path;                // longest root->link path, root excluded (links)
  int32_t max_sub;                 // largest subtree of a non-root link, itself excluded
  uint32_t root_kids;              // links whose parent is the root
  uint32_t lpath[kMaxLinks];       // links on the path root..link, both included
  uint32_t lsub[kMaxLinks];        // links in the subtree of link, itself included
  uint32_t ancmask[kMaxLinks];     // dofs on the path root..link (root dofs 0-5 always set)
  uint32_t dsub[kMaxDofs];         // links moved by dof j (subtree of its link; root dofs: all)
  uint32_t ddesc[kMaxDofs];        // dofs k whose link path contains dof j (bit k)
  // FK by pointer jumping (k_step fk): jump[i] byte r = the 2^r-th ancestor of link i, the root (0)
  // once the path is exhausted; fk_rounds = ceil(log2(max_path)) rounds cover every path
  uint32_t jump[kMaxLinks];
  int32_t fk_rounds;
  // collide pass B: the largest lane-group level per stone pair (allsteps_pair_group.h): 4, or what
  // ALLSTEPS_PAIR_GROUP set at as_create (1: one lane per pair, always)
  int32_t pair_group_cap;
  // everything lane-indexed that k_step reads once per launch, one row per lane (allsteps_lane_table.h);
  // rebuilt by fill_lane_table whenever the model, task or actuator fields above change
  LaneRow lane[kLaneRows];
};
static_assert(kLaneRows == 32 && kMaxLinks <= kLaneRows && kMaxDofs <= kLaneRows, "one table row per k_step lane");
inline void fill_lane_table(Consts& c) {
  build_lane_table(c.lane, c.model, c.task, c.act, c.nv, c.lpath, c.lsub, c.ancmask, c.dsub, c.jump);
}

// Every model field the kernels index with: a malformed model is rejected here instead of becoming
// an out-of-bounds LDS / register access (geoms: 32 LDS slots, foot id packed in 4 bits into the
// per-foot sensor masks; self pairs: 8-bit geom indices, 6 words per lane).  has_hind: the state carries
// contact_mask_hind, so foot ids 2 and 3 have a sensor mask.  False and the reason in `err` (the caller
// puts its own name in front).
inline bool check_model(const as_model_t& m, bool has_hind, std::string& err) {
  if (m.num_links < 1 || m.num_links > kMaxLinks) {
    err = "num_links out of range (1.." + std::to_string(kMaxLinks) + ")";
    return false;
  }
  if (m.num_hinges != m.num_links - 1 || m.num_hinges > AS_ACT_DIM) {
    err = "num_hinges must be num_links-1 <= 21";
    return false;
  }
  if (m.num_geoms < 0 || m.num_geoms > AS_MAX_GEOMS) {
    err = "num_geoms";
    return false;
  }
  if (m.num_priority_geoms < 0 || m.num_priority_geoms > m.num_geoms) {
    err = "num_priority_geoms outside [0, num_geoms]";
    return false;
  }
  const int max_foot = has_hind ? 3 : 1;
  for (int g = 0; g < m.num_geoms; ++g) {
    if (m.geom_link[g] < 0 || m.geom_link[g] >= m.num_links) {
      err = "geom_link[" + std::to_string(g) + "] outside [0, num_links)";
      return false;
    }
    if (m.geom_type[g] != 0 && m.geom_type[g] != 1) {
      err = "geom_type[" + std::to_string(g) + "] not 0 (sphere) / 1 (capsule)";
      return false;
    }
    if (m.geom_foot[g] < -1 || m.geom_foot[g] > max_foot) {
      err = "geom_foot[" + std::to_string(g) + "] outside [-1, " + std::to_string(max_foot) +
            "] (2, 3 need contact_mask_hind)";
      return false;
    }
  }
  if (m.num_self_pairs < 0 || m.num_self_pairs > AS_MAX_SELF_PAIRS) {
    err = "num_self_pairs outside [0, AS_MAX_SELF_PAIRS]";
    return false;
  }
  for (int i = 0; i < m.num_self_pairs; ++i) {
    const int w = m.self_pair[i], g1 = w & 0xff, g2 = w >> 8;
    if (w < 0 || g1 >= g2 || g2 >= m.num_geoms) {
      err = "self_pair[" + std::to_string(i) + "] is not g1 | g2 << 8 with g1 < g2 < num_geoms";
      return false;
    }
  }
  return true;
}

// parent[] is a tree in topological order: the root first, every other link after its parent.  What
// every walk up parent[] (plan_tree, sweep_skip_mask) needs to end at the root.  Requires check_model.
inline bool check_parents(const as_model_t& m, std::string& err) {
  for (int i = 0; i < m.num_links; ++i) {
    const int pa = m.parent[i];
    if (i == 0 ? pa != -1 : (pa < 0 || pa >= i)) {
      err = "parent not topological";
      return false;
    }
  }
  return true;
}

// The tree plan of c.model (c.nv = 6 + num_hinges set; requires check_model): lpath, lsub, dsub, ancmask,
// ddesc, jump, root_kids, max_path, max_sub, fk_rounds.  False and the reason in `err` for a parent[] that
// is no topologically ordered tree, a tree deeper than the FK's four jump rounds reach, or a cfg_dof_link
// outside the links.
inline bool plan_tree(Consts& h, std::string& err) {
  const as_model_t* model = &h.model;
  const int nl = model->num_links;
  h.max_path = h.max_sub = h.fk_rounds = 0;
  h.root_kids = 0u;
  for (int i = 0; i < kMaxLinks; ++i) h.lpath[i] = h.lsub[i] = h.ancmask[i] = h.jump[i] = 0u;
  for (int j = 0; j < kMaxDofs; ++j) h.dsub[j] = h.ddesc[j] = 0u;
  if (!check_parents(*model, err)) return false;
  for (int i = 0; i < nl; ++i) {
    int pa = model->parent[i];
    h.lpath[i] = (i == 0 ? 0u : h.lpath[pa]) | (1u << i);
    if (i > 0 && pa == 0) h.root_kids |= 1u << i;
  }
  for (int i = 0; i < nl; ++i)
    for (int l = 0; l < nl; ++l)
      if ((h.lpath[l] >> i) & 1u) h.lsub[i] |= 1u << l;
  for (int j = 0; j < h.nv; ++j) h.dsub[j] = j < 6 ? h.lsub[0] : h.lsub[j - 5];
  for (int i = 0; i < nl; ++i) {
    h.max_path = std::max(h.max_path, __builtin_popcount(h.lpath[i]) - 1);
    if (i > 0) h.max_sub = std::max(h.max_sub, __builtin_popcount(h.lsub[i]) - 1);
  }
  while ((1 << h.fk_rounds) < h.max_path) ++h.fk_rounds;
  if (h.fk_rounds > 4) {
    err = "tree deeper than 16 links";
    return false;
  }
  for (int i = 0; i < nl; ++i) {
    int a = i > 0 ? model->parent[i] : 0;
    for (int r = 0; r < 4; ++r) {  // a = the 2^r-th ancestor (0 past the root)
      h.jump[i] |= (uint32_t)a << (8 * r);
      for (int k = 0; k < (1 << r); ++k) a = a > 0 ? model->parent[a] : 0;
    }
  }
  for (int k = 0; k < model->num_hinges; ++k) {
    int li = model->cfg_dof_link[k];
    if (li < 1 || li >= model->num_links) {
      err = "cfg_dof_link";
      return false;
    }
  }
  for (int l = 0; l < model->num_links; ++l) {
    uint32_t mask = 0x3Fu;
    for (int i = l; i > 0; i = model->parent[i]) mask |= 1u << (6 + i - 1);
    h.ancmask[l] = mask;
  }
  for (int j = 0; j < h.nv; ++j)
    for (int k = 0; k < h.nv; ++k) {
      const int lk = k < 6 ? 0 : k - 5;
      if ((h.ancmask[lk] >> j) & 1u) h.ddesc[j] |= 1u << k;
    }
  return true;
}

// The H^-1 sweep's skipped column quads (step_dynamics.h sweep_inverse; bit r (NB - 1) + jb: round
// r, quad jb of the rotated row), compiled for the Allsteps walker (27 dofs) and the C5 quadruped (18):
// the quads in which the pivot rows are structurally zero for those trees.  as_create runs the
// structural sweep for the model it is given (sweep_skip_mask) and launches the skipping kernel only if
// every compiled bit is also set for that model.
constexpr uint64_t kSweepSkip27 = 207817167ull;  // 14 of the walker's 42 quad updates
constexpr uint64_t kSweepSkip18 = 3219ull;       // 6 of the quadruped's 20

// The structural sweep (host): which column quads of which rounds the pivot rows are exactly zero in,
// for this model's tree under the sweep's layout and round order (SweepLayout).  H_ij is nonzero only
// when the links of dofs i and j are on one root path (h_row writes +0 elsewhere); a round on block P
// leaves (i, j) zero unless it was nonzero or both a_iP and a_Pj have a nonzero entry, sets the pivot
// columns where a_iP has one and the pivot rows where a_Pj has one -- a zero stays +0 through every such
// update (its products all have a +0 factor and start from +0), which is what makes a skipped quad exact.
// Requires check_model and check_parents (the walks up parent[] end at the root).
inline uint64_t sweep_skip_mask(const as_model_t& m) {
  const int nl = m.num_links, nv = 6 + m.num_hinges;
  const int NP = (nv + kSweepB - 1) / kSweepB * kSweepB, NB = NP / kSweepB, NQ = NB - 1, PAD = AS_SWEEP_PAD(nv);
  if (NP > 32 || NQ * NB > 64 || nl < 1 || nl > kMaxLinks) return 0ull;
  auto padded = [&](int k) { return k < PAD ? k : k + (NP - nv); };
  auto link = [](int d) { return d < 6 ? 0 : d - 5; };
  auto on_path = [&](int a, int l) {  // a is l or one of its ancestors
    for (int x = l; x >= 0; x = x > 0 ? m.parent[x] : -1)
      if (x == a) return true;
    return false;
  };
  bool S[32][32] = {};
  for (int i = 0; i < nv; ++i)
    for (int j = 0; j < nv; ++j)
      S[padded(i)][padded(j)] = on_path(link(i), link(j)) || on_path(link(j), link(i));
  for (int q = 0; q < NP - nv; ++q) S[PAD + q][PAD + q] = true;
  uint64_t mask = 0ull;
  for (int r = 0; r < NB; ++r) {
    const int b = NB - 1 - r, p = kSweepB * b;
    bool colany[32] = {}, rowany[32] = {};
    for (int c = 0; c < kSweepB; ++c)
      for (int k = 0; k < NP; ++k) {
        colany[k] = colany[k] || S[p + c][k];
        rowany[k] = rowany[k] || S[k][p + c];
      }
    for (int jb = 0; jb < NQ; ++jb) {
      const int bb = ((b - 1 - jb) % NB + NB) % NB;
      bool any = false;
      for (int c = 0; c < kSweepB; ++c) any = any || colany[kSweepB * bb + c];
      if (!any) mask |= 1ull << (r * NQ + jb);
    }
    for (int i = 0; i < NP; ++i)
      for (int j = 0; j < NP; ++j) {
        const bool pi = i >= p && i < p + kSweepB, pj = j >= p && j < p + kSweepB;
        S[i][j] = pi && pj ? true : pj ? rowany[i] : pi ? colany[j] : (S[i][j] || (rowany[i] && colany[j]));
      }
  }
  return mask;
}

}  // namespace as
