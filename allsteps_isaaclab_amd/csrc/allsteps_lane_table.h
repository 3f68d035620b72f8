// allsteps_lane_table.h -- the per-lane constants table of the step kernel, and its host builder.
//
// k_step keeps one lane per link / dof / geom / hinge and reads that lane's model constants once per
// launch.  Read from the model tables they were a chain of dependent lookups (cfg_dof_link[lane] ->
// lower[link], right_idx / left_idx -> init_q[source]) spread over a dozen arrays; the host resolves
// every lookup once (as_create and the setters that change the constants) into one row per lane, so a
// lane's loads depend on nothing but its lane index: ten 16-B chunks, all issued together.
//
// Plain C++ with no HIP dependency: a host program can build and check the table (tests/).
#pragma once

#include <stdint.h>

#include "../../include/allsteps.h"

namespace as {

constexpr int kLaneRows = 32;  // lanes per env in k_step

// One row = ten 16-B chunks; the kernel loads all ten at launch start and chunks 8-9 (the reset constants)
// again ahead of the final FK, instead of holding them in registers across the substeps.
// "lane" below is the row index; every clamp is the one k_step applied when it read the model tables.
struct alignas(16) LaneRow {
  // chunk 0, 1: tree plan (k_step Topo) and the H-row mask of dof `lane`
  uint32_t lpath;    // lane < num_links ? Consts::lpath[lane] : 0
  uint32_t lsub;     // lane < num_links ? Consts::lsub[lane] : 0
  uint32_t dsub;     // lane < nv ? Consts::dsub[lane] : 0
  uint32_t jump;     // lane < num_links ? Consts::jump[lane] : 0
  float lo, hi;      // lower / upper[lane + 1 < num_links ? lane + 1 : 0]: limits of hinge `lane`
  float arm;         // 6 <= lane < nv ? armature[lane - 5] : 0
  uint32_t ancmask;  // Consts::ancmask[j < 6 ? 0 : j - 5], j = lane < nv ? lane : 0
  // chunk 2-5: joint constants of link i = (1 <= lane < num_links ? lane : 0) (k_step LinkC), then the
  // cfg-order joint `lane` (lane < num_hinges; zeros past it)
  float offset_quat[4];
  float axis[3];
  float anchor[3];
  float offset_pos[3];
  float gear;        // gear[lane]
  float default_q;   // actuator default_q[lane]
  uint32_t pad;
  // chunk 6-8: geom g = (lane < num_geoms ? lane : 0) (k_step GeomC)
  int32_t geom_link, geom_type, geom_foot;
  float geom_radius;
  float geom_p0[3];
  float geom_p1[3];
  // chunk 8, 9: reset constants of cfg-order joint `lane` (lane < num_hinges; zeros and link 1 past it)
  float init_q;      // init_q[lane]
  float init_qm;     // init_q[mirror source of lane] * sign
  float sign;        // -1 if lane is in neg_idx, else 1 (every lane)
  float rlo, rhi;    // lower / upper[cfg_dof_link[lane]]
  int32_t dof_link;  // cfg_dof_link[lane]
};
constexpr int kLaneChunks = 10;
static_assert(sizeof(LaneRow) == 16 * kLaneChunks, "ten 16-B chunks");

// The mirror source of joint `lane`: right_idx / left_idx applied in order, a later match winning over
// an earlier one (the sequential ifs of allsteps_env.py:505-530).
inline int lane_mirror_source(const as_task_t& T, int lane) {
  int src = lane;
  for (int t = 0; t < 9; ++t) {
    if (T.right_idx[t] == lane) src = T.left_idx[t];
    if (T.left_idx[t] == lane) src = T.right_idx[t];
  }
  return src;
}

// rows[kLaneRows] from the model, the task, the actuator and the tree plan (Consts::lpath .. jump; nv =
// 6 + num_hinges).  Requires what as_create checks: 1 <= num_links <= 24, num_hinges = num_links - 1 <=
// AS_ACT_DIM, 0 <= num_geoms <= AS_MAX_GEOMS, 1 <= cfg_dof_link[k] < num_links.
inline void build_lane_table(LaneRow* rows, const as_model_t& m, const as_task_t& T, const as_actuator_t& act, int nv,
                             const uint32_t* lpath, const uint32_t* lsub, const uint32_t* ancmask,
                             const uint32_t* dsub, const uint32_t* jump) {
  const int nl = m.num_links, nh = m.num_hinges;
  for (int lane = 0; lane < kLaneRows; ++lane) {
    LaneRow r{};
    const int hl = lane + 1 < nl ? lane + 1 : 0;
    const int j = lane < nv ? lane : 0;
    r.lpath = lane < nl ? lpath[lane] : 0u;
    r.lsub = lane < nl ? lsub[lane] : 0u;
    r.dsub = lane < nv ? dsub[lane] : 0u;
    r.jump = lane < nl ? jump[lane] : 0u;
    r.lo = m.lower[hl];
    r.hi = m.upper[hl];
    r.arm = lane >= 6 && lane < nv ? m.armature[lane - 5] : 0.f;
    r.ancmask = ancmask[j < 6 ? 0 : j - 5];
    const int i = lane >= 1 && lane < nl ? lane : 0;
    for (int k = 0; k < 4; ++k) r.offset_quat[k] = m.offset_quat[i][k];
    for (int k = 0; k < 3; ++k) {
      r.axis[k] = m.axis[i][k];
      r.anchor[k] = m.anchor[i][k];
      r.offset_pos[k] = m.offset_pos[i][k];
    }
    const int g = lane < m.num_geoms ? lane : 0;
    r.geom_link = m.geom_link[g];
    r.geom_type = m.geom_type[g];
    r.geom_foot = m.geom_foot[g];
    r.geom_radius = m.geom_radius[g];
    for (int k = 0; k < 3; ++k) {
      r.geom_p0[k] = m.geom_p0[g][k];
      r.geom_p1[k] = m.geom_p1[g][k];
    }
    r.dof_link = 1;
    r.sign = T.neg_idx[0] == lane || T.neg_idx[1] == lane ? -1.f : 1.f;
    if (lane < nh) {
      const int src = lane_mirror_source(T, lane);
      r.dof_link = m.cfg_dof_link[lane];
      r.gear = m.gear[lane];
      r.default_q = act.default_q[lane];
      r.init_q = T.init_q[lane] * 1.f;
      // a source outside the joints (a malformed mirror map) reads as 0 instead of past the table
      r.init_qm = (src >= 0 && src < AS_ACT_DIM ? T.init_q[src] : 0.f) * r.sign;
      r.rlo = m.lower[r.dof_link];
      r.rhi = m.upper[r.dof_link];
    }
    rows[lane] = r;
  }
}

}  // namespace as
