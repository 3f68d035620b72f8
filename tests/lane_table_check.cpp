// Stand-alone host check of csrc/allsteps_lane_table.h (built and run by tests/test_lane_table.py, plain
// and with -fsanitize=address,undefined).  Every source entry gets a distinct value; every field of each
// of the 32 rows is then compared with the entry k_step read from the model / task / actuator tables
// before the table existed (restated below lane by lane, clamps and the mirror select chain included).
#include <cstdio>
#include <cstring>

#include "../allsteps_isaaclab_amd/csrc/allsteps_lane_table.h"

static int g_bad = 0;
static float g_next = 1.0f;

// distinct, exactly representable values: 1.0, 1.5, 2.0, ...
static float fresh() { g_next += 0.5f; return g_next; }
static void fill(float* p, int n) { for (int i = 0; i < n; ++i) p[i] = fresh(); }

#define EXPECT(what, got, want)                                                                    \
  do {                                                                                             \
    if (std::memcmp(&(got), &(want), sizeof(got)) != 0) {                                          \
      if (g_bad++ < 20) std::printf("%s lane %d %s: got %g want %g\n", shape, lane, what, (double)(got), (double)(want)); \
    }                                                                                              \
  } while (0)

static void check(const char* shape, int nl, int ng) {
  const int nh = nl - 1, nv = 6 + nh;
  as_model_t m{};
  as_task_t T{};
  as_actuator_t act{};
  m.num_links = nl;
  m.num_hinges = nh;
  m.num_geoms = ng;
  fill(&m.offset_pos[0][0], AS_MAX_LINKS * 3);
  fill(&m.offset_quat[0][0], AS_MAX_LINKS * 4);
  fill(&m.axis[0][0], AS_MAX_LINKS * 3);
  fill(&m.anchor[0][0], AS_MAX_LINKS * 3);
  fill(m.armature, AS_MAX_LINKS);
  fill(m.lower, AS_MAX_LINKS);
  fill(m.upper, AS_MAX_LINKS);
  fill(m.gear, AS_MAX_LINKS);
  fill(m.geom_radius, AS_MAX_GEOMS);
  fill(&m.geom_p0[0][0], AS_MAX_GEOMS * 3);
  fill(&m.geom_p1[0][0], AS_MAX_GEOMS * 3);
  for (int g = 0; g < AS_MAX_GEOMS; ++g) {
    m.geom_link[g] = 1000 + g;
    m.geom_type[g] = 2000 + g;
    m.geom_foot[g] = 3000 + g;
  }
  for (int k = 0; k < AS_MAX_LINKS; ++k) m.cfg_dof_link[k] = 0;
  for (int k = 0; k < nh; ++k) m.cfg_dof_link[k] = 1 + (k * 5 + 3) % nh;  // a permutation of 1..nh (5 coprime to 21, 12)
  fill(T.init_q, AS_ACT_DIM);
  fill(act.default_q, AS_ACT_DIM);
  // the mirror map: joint 0 is matched at t = 0 (-> 8) and again at t = 8 (-> 10): the later match wins;
  // joint 9 is a left entry at t = 1 (-> 1) and a right entry at t = 7 (-> 11): again the later one
  const int right[9] = {0, 1, 2, 3, 4, 5, 6, 9, 0};
  const int left[9] = {8, 9, 7, 7, 7, 7, 7, 11, 10};
  for (int t = 0; t < 9; ++t) { T.right_idx[t] = right[t]; T.left_idx[t] = left[t]; }
  T.neg_idx[0] = 2;
  T.neg_idx[1] = 9;
  uint32_t lpath[32], lsub[32], ancmask[32], dsub[32], jump[32];
  for (int i = 0; i < 32; ++i) {
    lpath[i] = 0x10000u + i; lsub[i] = 0x20000u + i; ancmask[i] = 0x30000u + i; dsub[i] = 0x40000u + i;
    jump[i] = 0x50000u + i;
  }
  as::LaneRow rows[as::kLaneRows];
  as::build_lane_table(rows, m, T, act, nv, lpath, lsub, ancmask, dsub, jump);

  for (int lane = 0; lane < as::kLaneRows; ++lane) {
    const as::LaneRow& r = rows[lane];
    // tree plan (k_step load_topo)
    const int l = lane < nl ? lane : 0, j = lane < nv ? lane : 0, hl = lane + 1 < nl ? lane + 1 : 0;
    const uint32_t w_lpath = lane < nl ? lpath[l] : 0u, w_lsub = lane < nl ? lsub[l] : 0u;
    const uint32_t w_dsub = lane < nv ? dsub[j] : 0u, w_jump = lane < nl ? jump[l] : 0u;
    const float w_arm = lane >= 6 && lane < nv ? m.armature[lane - 5] : 0.f;
    EXPECT("lpath", r.lpath, w_lpath);
    EXPECT("lsub", r.lsub, w_lsub);
    EXPECT("dsub", r.dsub, w_dsub);
    EXPECT("jump", r.jump, w_jump);
    EXPECT("lo", r.lo, m.lower[hl]);
    EXPECT("hi", r.hi, m.upper[hl]);
    EXPECT("arm", r.arm, w_arm);
    // H-row mask (k_step load_geom)
    EXPECT("ancmask", r.ancmask, ancmask[j < 6 ? 0 : j - 5]);
    // joint constants (k_step load_link)
    const int i = lane >= 1 && lane < nl ? lane : 0;
    for (int k = 0; k < 4; ++k) EXPECT("offset_quat", r.offset_quat[k], m.offset_quat[i][k]);
    for (int k = 0; k < 3; ++k) {
      EXPECT("axis", r.axis[k], m.axis[i][k]);
      EXPECT("anchor", r.anchor[k], m.anchor[i][k]);
      EXPECT("offset_pos", r.offset_pos[k], m.offset_pos[i][k]);
    }
    // geom (k_step load_geom)
    const int g = lane < ng ? lane : 0;
    EXPECT("geom_link", r.geom_link, m.geom_link[g]);
    EXPECT("geom_type", r.geom_type, m.geom_type[g]);
    EXPECT("geom_foot", r.geom_foot, m.geom_foot[g]);
    EXPECT("geom_radius", r.geom_radius, m.geom_radius[g]);
    for (int k = 0; k < 3; ++k) {
      EXPECT("geom_p0", r.geom_p0[k], m.geom_p0[g][k]);
      EXPECT("geom_p1", r.geom_p1[k], m.geom_p1[g][k]);
    }
    // cfg-order joint `lane` and its reset constants (k_step's rs_* block: selects in sequence)
    int src = lane;
    for (int t = 0; t < 9; ++t) {
      src = right[t] == lane ? left[t] : src;
      src = left[t] == lane ? right[t] : src;
    }
    const float w_sign = lane == 2 || lane == 9 ? -1.f : 1.f;
    int w_li = 1;
    float w_gear = 0.f, w_dq = 0.f, w_q = 0.f, w_qm = 0.f, w_lo = 0.f, w_hi = 0.f;
    if (lane < nh) {
      w_li = m.cfg_dof_link[lane];
      w_gear = m.gear[lane];
      w_dq = act.default_q[lane];
      w_q = T.init_q[lane];
      w_qm = T.init_q[src] * w_sign;
      w_lo = m.lower[w_li];
      w_hi = m.upper[w_li];
    }
    EXPECT("dof_link", r.dof_link, w_li);
    EXPECT("gear", r.gear, w_gear);
    EXPECT("default_q", r.default_q, w_dq);
    EXPECT("init_q", r.init_q, w_q);
    EXPECT("init_qm", r.init_qm, w_qm);
    EXPECT("sign", r.sign, w_sign);
    EXPECT("rlo", r.rlo, w_lo);
    EXPECT("rhi", r.rhi, w_hi);
  }
  // the select chain above, spelled out for the two contested joints
  if (as::lane_mirror_source(T, 0) != 10 || as::lane_mirror_source(T, 9) != 11 || as::lane_mirror_source(T, 8) != 0) {
    std::printf("%s: mirror sources %d %d %d, want 10 11 0\n", shape, as::lane_mirror_source(T, 0),
                as::lane_mirror_source(T, 9), as::lane_mirror_source(T, 8));
    ++g_bad;
  }
}

int main() {
  check("walker", 22, 22);     // 22 links, 21 hinges, 22 geoms, 27 dofs
  check("quadruped", 13, 17);  // 13 links, 12 hinges, 18 dofs
  std::printf("lane table: %d mismatches\n", g_bad);
  return g_bad ? 1 : 0;
}
