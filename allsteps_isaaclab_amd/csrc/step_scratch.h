// step_scratch.h -- k_step's sizing constants and its LDS layout.
// Nothing here runs in a substep: DynScratch / ConScratch / PhaseScratch are the phase-local unions, Topo the
// per-lane tree plan, EnvS one env's state across the phases (every phase header says what it reads and
// writes there), Smem the workgroup's two envs.
#pragma once

#include <hip/hip_runtime.h>

#include "../../include/allsteps.h"
#include "allsteps_device.h"
#include "allsteps_kernels.h"

namespace as {

constexpr int G = 32;               // lanes per env
constexpr int EPB = 2;              // envs per 64-lane workgroup
constexpr int LMAX = kMaxLinks;     // links (walker: 22)
constexpr int NVMAX = 6 + LMAX - 1; // generalized velocities
constexpr int MAXC = AS_MAX_CONTACTS;
constexpr int MAXR = AS_MAX_ROWS;
constexpr int NST = AS_NUM_STONES;
constexpr int kBisectIters = 12;    // capsule minimum: slope-sign bisection, interval 2^-12 = 2.4e-4
constexpr int kPairsPerChunk = G;   // one lane per (stone, geom) pair in the exact test
static_assert(kPairsPerChunk - 1 + G <= 64, "pending pair list (PhaseScratch::col.pl)");
typedef float v4f __attribute__((ext_vector_type(4)));  // native 16-B vector (LDS b128 accesses)
typedef float v2f __attribute__((ext_vector_type(2)));  // register pair (packed FP32 math)

static_assert(NVMAX <= G, "one lane per generalized velocity");
static_assert(LMAX <= G, "one lane per link");
static_assert(MAXR <= G, "one row per lane in the row builders");
static_assert(MAXR <= 3 * MAXC, "a row index / 3 is a valid contact slot");

// ------------------------------------------------------------------------------------------------
// per-env LDS scratch.  Occupancy at 4096 envs is set by LDS: two envs per 64-lane workgroup must
// stay <= 20 KB so that 8 workgroups (2 waves/SIMD) fit a CU and 4096 envs run in one round.  The
// phase-local arrays therefore share one union: FK (Rl) -> dynamics (c, Ib, Ic, V, A, F) ->
// sweep (piv) -> constraint rows (Jm, Wm); each phase ends before the next one writes.
constexpr int kPrioRows = 9;          // constraint rows per issue-priority level (see substep; 4 / 6 / 9 / 12 / 15 timed)
constexpr int kRowGroup = 3;          // constraint rows per J / W / PGS group (a contact triplet)
constexpr int LDJ = 28;               // J / W row stride (>= NV = 27)
struct DynScratch {
  float c[LMAX][3];
  float Ib[LMAX][10];
  float Ic[LMAX][10];
  float Sq[LMAX][6];    // S_i qd_i, later the subtree force sums F_i
  union {
    float Rl[LMAX][12]; // FK: local joint transforms (R 9, p 3); dead before cr / f are written
    struct {
      float cr[LMAX][6];  // V_i x_m S_i qd_i
    } b;
    // subtree sums: body force (6) and spatial inertia (10) of every link, transposed and split by
    // link parity ([quantity][l & 1][l >> 1]: the MFMA's A operand runs, read as 16-B vectors),
    // written after the last read of cr
    alignas(16) float xt[16][2][LMAX / 2];
  };
};
struct alignas(16) ConScratch {
  float Jm[MAXR][LDJ];  // J rows (lane = dof column); W = H^-1 J^T stays in registers (lane = dof)
};
union alignas(16) PhaseScratch {
  DynScratch d;
  float obs[64];        // epilogue: observation row staging
  struct {
    // collide: geom segment endpoints, radius, packed type/foot/link; row stride 12 floats (16-B
    // aligned): geoms g and g + 8 land on different banks of the pair passes' gathered reads
    alignas(16) float g[32][12];
    alignas(16) float bs[32][4];  //  bounding sphere (segment midpoint, half length + radius)
    int pl[64];         //          pending (stone << 8 | geom) pairs (< 32 + G), then self pairs
    uint32_t need[NST]; //          per candidate stone: geoms past the bounding test
    alignas(16) float cc[NST][4];  //   per candidate stone: its center relative to the root
  } col;
  struct alignas(16) {
    // sweep: every lane's (rotated) row, rewritten each round, so the publishing stores need no
    // pivot-lane branch; rows are read by the next round's pivot indices.  Row stride 28 floats: the
    // 8-lane groups of a ds_write_b128 then cover 8 distinct 4-bank quads
    float rows[G][28];
  } sw;                 // aliases the dynamics scratch, dead by then
  ConScratch k;
  // contact flags: per contact lambda_n n (3) and its (foot, stone) key, written after the PGS
  alignas(16) float cf[MAXC][4];
};

// The constants block is read-only for the whole launch: address space 4 (constant) lets uniform
// loads become scalar loads and keeps lane-varying ones global (not flat) loads.
using CK = const __attribute__((address_space(4))) Consts;
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
typedef const __attribute__((address_space(4))) u32x4 ConstV4;  // a 16-B chunk of a LaneRow
typedef const uint32_t __attribute__((may_alias)) StateWord;     // a state word of any 4-B type

// Per-lane tree plan and joint constants, read once per launch and kept in registers
// (lane = link for the l* fields, lane = dof for the d* fields, lane = hinge for lo / hi).
struct Topo {
  uint32_t lpath;  // links on the path root..link(lane)
  uint32_t lsub;   // subtree of link(lane)
  uint32_t dsub;   // links moved by dof lane
  float lo, hi;    // limits of hinge lane (link lane + 1)
  float arm;       // armature of dof lane (0 on the root dofs)
  uint32_t jump;   // FK pointer jumping: byte r = the 2^r-th ancestor of link lane (Consts::jump)
};

__device__ Topo load_topo(const Consts& K, int lane) {
  const as_model_t& m = K.model;
  const int nl = m.num_links, nv = K.nv;
  Topo t;
  const int l = lane < nl ? lane : 0;
  const int j = lane < nv ? lane : 0;
  const int hl = lane + 1 < nl ? lane + 1 : 0;
  t.lpath = lane < nl ? K.lpath[l] : 0u;
  t.lsub = lane < nl ? K.lsub[l] : 0u;
  t.dsub = lane < nv ? K.dsub[j] : 0u;
  t.lo = m.lower[hl];
  t.hi = m.upper[hl];
  t.arm = lane >= 6 && lane < nv ? m.armature[lane - 5] : 0.f;
  t.jump = lane < nl ? K.jump[l] : 0u;
  return t;
}

struct EnvS {
  float R[LMAX][9];
  float p[LMAX][3];
  float c0[3];          // root COM (relative), kept past the dynamics phase for integration
  // motion subspace [w; v_O] per dof.  Rows of 12 floats (48 B, two 16-B stores / loads): 16 lanes at
  // that stride cover 16 distinct 16-B slots of the 64 read banks and 8 of the 32 write banks, where a
  // 32-B stride put dofs j and j + 4 (stores) or j + 8 (loads) on the same banks
  alignas(16) float S[NVMAX][12];
  float b[32];          // tau - C
  PhaseScratch x;
  // per row: 1/A_rr, target, bound parameter, in-group coupling.  The bound parameter is what the
  // PGS needs of the row's group: on row 1 of a group mu for a contact triplet (0 otherwise), on
  // row 2 the upper-bound offset, 0 for a contact triplet (+-mu ln) and +inf otherwise ([0, inf))
  alignas(16) float rmeta[MAXR][4];
  float cdir[MAXC][3][3];  // contact frame: normal, tangent 1, tangent 2
  int rlink[MAXR];      // contact rows: link | (link2 + 1) << 8 (link2 = -1: stone); limit rows: -1 - dof
  float rsign[MAXR];
  float cpt[MAXC][3], cn[MAXC][3], csep[MAXC];
  int clink[MAXC], clink2[MAXC], cstone[MAXC], cfoot[MAXC];  // clink2 / cstone: -1 unless self / stone
  float u[NVMAX];
  float qi[LMAX];       // hinge angles, link order (link i -> qi[i-1])
  float tau[LMAX];
  float qt[LMAX];       // AS_ACT_DC_MOTOR: joint position targets (link order)
  float act[AS_ACT_DIM];
  float stones[NST * 3];
  float root_pos[3], root_quat[4];
  int cand[NST];
  uint32_t mask[4];     // contact sensors 0..3 (2, 3: a quadruped's hind feet)
  int ndrop;            // contacts cut by the row budget over this launch's substeps (counters[kCntDropped])
  int nrows;            // constraint rows over this launch's substeps (the next launch's placement cost)
  // the task epilogue's per-env words (kPk*: its scalars, then the nine stored body positions a launch
  // without physics starts from), loaded with the rest of the state at launch start and parked here
  // across the substeps: registers cannot hold them, and read after the final FK they were eleven
  // exposed memory round trips
  uint32_t pk[20];
};
enum { kPkIdx = 0, kPkPrev, kPkNext, kPkCount, kPkSwing, kPkEpLen, kPkPot, kPkOldPot, kPkFc0, kPkFc1, kPkEpisode,
       kPkBody, kPkWords = kPkBody + 9 };

struct Smem {
  EnvS env[EPB];
  Topo topo[G];  // per-lane tree plan (shared by both envs; registers cannot hold it)
};

}  // namespace as
