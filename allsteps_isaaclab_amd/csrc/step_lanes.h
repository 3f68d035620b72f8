// step_lanes.h -- cross-lane primitives of the step kernels: DPP / readlane moves, half-wave sums, scans and
// minima, the diagnostic stamps (Stamp) and the bit-mask walks over a lane's path or subtree.
// Reads and writes no EnvS field of its own: path_sum reads the rows its caller hands it.
#pragma once

#include <hip/hip_runtime.h>

#include "step_scratch.h"

namespace as {

// ------------------------------------------------------------------------------------------------
// cross-lane helpers

template <int CTRL>
__device__ __forceinline__ float dpp(float v) {
  // bound_ctrl: the quad permutes and row mirrors used here never read outside the row, so the
  // "old" operand is dead and the move folds into the consuming v_add_f32_dpp.  (collide's flush_grp also
  // uses row shifts, which do read outside at a row's first lanes and get 0 there: it discards those lanes.)
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, true));
}

__device__ __forceinline__ float readlane_f(float v, int l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l)); }

// Sum over the 32 lanes of this env's half-wave: DPP butterfly inside each 16-lane row
// (quad_perm [1,0,3,2], [2,3,0,1], row_half_mirror, row_mirror), then v_permlane16_swap exchanges the
// two rows of each half so that every lane adds (row 0 + row 1) of its half -- no SGPR round trip.
// Every lane of a half gets the bit-identical value.
__device__ __forceinline__ float row_pair_sum(float v) {
  const auto p = __builtin_amdgcn_permlane16_swap(__float_as_int(v), __float_as_int(v), false, false);
  return __int_as_float(p[0]) + __int_as_float(p[1]);
}

__device__ __forceinline__ float half_sum(float v) {
  v += dpp<0xB1>(v);
  v += dpp<0x4E>(v);
  v += dpp<0x141>(v);
  v += dpp<0x140>(v);
  return row_pair_sum(v);
}

// Sums over the half-wave of N independent values (the W pass and the PGS), two at a time: the
// first v_permlane16_swap exchanges row 1 of value a with row 0 of value b, so one add leaves
// a_l + a_(l+16) in row 0 and b_l + b_(l+16) in row 1; the DPP butterfly then finishes both sums at
// once (A in every lane of row 0, B in row 1), and a second swap hands A and B to every lane of the
// half.  A pair costs 8 instructions instead of 14; an odd last value takes the swap with itself
// first (7).  The tree: the cross-row add, then a balanced tree over the 16 row lanes (oracle
// tree32); every lane gets the bit-identical value.
template <int N>
__device__ __forceinline__ void half_sum_n(float (&v)[N]) {
  constexpr int P = (N + 1) / 2;
  float c[P];
#pragma unroll
  for (int p = 0; p < P; ++p) {
    const int b = 2 * p + 1 < N ? 2 * p + 1 : 2 * p;
    const auto s = __builtin_amdgcn_permlane16_swap(__float_as_int(v[2 * p]), __float_as_int(v[b]), false, false);
    c[p] = __int_as_float(s[0]) + __int_as_float(s[1]);
  }
#pragma unroll
  for (int p = 0; p < P; ++p) c[p] += dpp<0xB1>(c[p]);
#pragma unroll
  for (int p = 0; p < P; ++p) c[p] += dpp<0x4E>(c[p]);
#pragma unroll
  for (int p = 0; p < P; ++p) c[p] += dpp<0x141>(c[p]);
#pragma unroll
  for (int p = 0; p < P; ++p) c[p] += dpp<0x140>(c[p]);
#pragma unroll
  for (int p = 0; p < P; ++p) {
    if (2 * p + 1 < N) {
      const auto s = __builtin_amdgcn_permlane16_swap(__float_as_int(c[p]), __float_as_int(c[p]), false, false);
      v[2 * p] = __int_as_float(s[0]);
      v[2 * p + 1] = __int_as_float(s[1]);
    } else {
      v[2 * p] = c[p];
    }
  }
}

// Exclusive prefix sum over this env's half-wave of a count c in [0, 3], and the half's total:
// two ballots (bit 0 and bit 1 of c) and popcounts, no cross-lane data movement.
__device__ __forceinline__ int half_scan3(int c, int& total) {
  const int sh = threadIdx.x & 32;
  const uint32_t m0 = (uint32_t)(__ballot((c & 1) != 0) >> sh);
  const uint32_t m1 = (uint32_t)(__ballot((c & 2) != 0) >> sh);
  const uint32_t lt = (1u << (threadIdx.x & 31)) - 1u;
  total = __popc(m0) + 2 * __popc(m1);
  return __popc(m0 & lt) + 2 * __popc(m1 & lt);
}

template <int CTRL>
__device__ __forceinline__ uint32_t dpp_u(uint32_t v) {
  return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xF, 0xF, true);
}

// OR over the half-wave of two values at once (the pairing of half_sum_n)
__device__ __forceinline__ void half_or2(uint32_t& x, uint32_t& y) {
  const auto s = __builtin_amdgcn_permlane16_swap((int)x, (int)y, false, false);
  uint32_t c = (uint32_t)s[0] | (uint32_t)s[1];
  c |= dpp_u<0xB1>(c);
  c |= dpp_u<0x4E>(c);
  c |= dpp_u<0x141>(c);
  c |= dpp_u<0x140>(c);
  const auto t = __builtin_amdgcn_permlane16_swap((int)c, (int)c, false, false);
  x = (uint32_t)t[0];
  y = (uint32_t)t[1];
}

// half_min of N values two at a time (the pairing of half_sum_n; min is exact, so any order gives
// the same value)
template <int N>
__device__ __forceinline__ void half_min_n(float (&v)[N]) {
  static_assert(N % 2 == 0, "pairs");
  constexpr int P = N / 2;
  float c[P];
#pragma unroll
  for (int p = 0; p < P; ++p) {
    const auto s = __builtin_amdgcn_permlane16_swap(__float_as_int(v[2 * p]), __float_as_int(v[2 * p + 1]), false, false);
    c[p] = fminf(__int_as_float(s[0]), __int_as_float(s[1]));
  }
#pragma unroll
  for (int p = 0; p < P; ++p) c[p] = fminf(c[p], dpp<0xB1>(c[p]));
#pragma unroll
  for (int p = 0; p < P; ++p) c[p] = fminf(c[p], dpp<0x4E>(c[p]));
#pragma unroll
  for (int p = 0; p < P; ++p) c[p] = fminf(c[p], dpp<0x141>(c[p]));
#pragma unroll
  for (int p = 0; p < P; ++p) c[p] = fminf(c[p], dpp<0x140>(c[p]));
#pragma unroll
  for (int p = 0; p < P; ++p) {
    const auto s = __builtin_amdgcn_permlane16_swap(__float_as_int(c[p]), __float_as_int(c[p]), false, false);
    v[2 * p] = __int_as_float(s[0]);
    v[2 * p + 1] = __int_as_float(s[1]);
  }
}

// diagnostic phase stamps, Stamp<kOn>.  k_step carries Stamp<false>: no members, empty methods, so the
// production kernel holds no stamp pointer, counter, branch, clock read or LDS for them.  Its twin
// k_step_diag carries Stamp<true> and is launched exactly when as_debug_stamps set a buffer (launch_step; p is
// never null there): each wave accumulates its s_memtime deltas per phase in LDS and adds them to the device
// counters once, at the end of the launch -- a global atomic per phase boundary would put a contended memory
// round trip into the next phase.
// With p[kWaveRecFlag] != 0 each wave also writes a record of its own (the last launch's waves:
// phase cycles, total, start / end time, HW_ID / XCC_ID, rows and contacts summed over substeps per
// env; collide's pass B: the stone pairs of each env, their sum over the substeps in bits 0-15 and the
// largest single flush's in bits 16-31 -- the substep's own count as long as that is at most
// kPairsPerChunk, one flush per substep -- and the wave's flushes per group level, 8 bits each: one lane
// per pair, then L = 2, 3, 4) at p + kWaveRecBase + block * kWaveRecWords, for tail analysis
// (scripts/stamps.py; the record's size and words are part of as_debug_stamps' contract, include/allsteps.h).
constexpr int kWaveRecFlag = 31, kWaveRecBase = 64, kWaveRecWords = 30;
static_assert(16 + kNumStamps <= kWaveRecFlag && kNumStamps + 14 <= kWaveRecWords, "stamp slots");
template <bool kOn>
struct Stamp;
template <>
struct Stamp<false> {
  __device__ __forceinline__ void start() {}
  __device__ __forceinline__ void count(int, int) {}
  __device__ __forceinline__ void pairs(int, int) {}
  __device__ __forceinline__ void mark(int) {}
  __device__ __forceinline__ void flush() {}
};
template <>
struct Stamp<true> {
  unsigned long long* p;
  unsigned long long* acc;  // LDS, kNumStamps
  unsigned long long t;
  unsigned long long t0 = 0ull, rt0 = 0ull;  // s_memtime / s_memrealtime (100 MHz) at the start
  unsigned rows = 0u, cons = 0u, prs = 0u, lvls = 0u;
  __device__ void start() {
    if (p) {
      if (threadIdx.x < kNumStamps) acc[threadIdx.x] = 0ull;
      t = t0 = __builtin_amdgcn_s_memtime();
      rt0 = __builtin_amdgcn_s_memrealtime();
      __syncthreads();  // here, not in k_step: an untimed launch has no fence ahead of its first loads
    }
  }
  __device__ void count(int nrow, int nc) {
    if (p) {
      rows += (unsigned)nrow;
      cons += (unsigned)nc;
    }
  }
  __device__ void pairs(int np, int level) {  // one pass-B flush: this env's pairs, the wave's level (0, 2, 3, 4)
    if (p) {
      const unsigned mx = prs >> 16 > (unsigned)np ? prs >> 16 : (unsigned)np;
      prs = ((prs + (unsigned)np) & 0xffffu) | (mx << 16);
      lvls += 1u << (8 * (level < 2 ? 0 : level - 1));
    }
  }
  __device__ void mark(int k) {
    if (p) {
      unsigned long long now = __builtin_amdgcn_s_memtime();
      if (threadIdx.x == 0) acc[k] += now - t;
      t = now;
    }
  }
  __device__ void flush() {
    if (p) {
      __syncthreads();
      unsigned long long tot = 0;
      for (int k = 0; k < kNumStamps; ++k) tot += acc[k];
      if (p[kWaveRecFlag]) {
        // per-wave records, plain stores only: the atomics of the aggregate mode would queue in
        // front of the late waves' own memory traffic and distort exactly the tail being measured
        unsigned long long* rec = p + kWaveRecBase + (size_t)blockIdx.x * kWaveRecWords;
        const unsigned long long now = __builtin_amdgcn_s_memtime();
        const unsigned hw = __builtin_amdgcn_s_getreg((31 << 11) | 4);    // HW_REG_HW_ID
        const unsigned xcc = __builtin_amdgcn_s_getreg((31 << 11) | 20);  // HW_REG_XCC_ID
        const int k = threadIdx.x;
        if (k < kNumStamps) rec[k] = acc[k];
        if (k == 0) {
          rec[kNumStamps] = tot; rec[kNumStamps + 1] = t0; rec[kNumStamps + 2] = now;
          rec[kNumStamps + 9] = rt0; rec[kNumStamps + 10] = __builtin_amdgcn_s_memrealtime();
          rec[kNumStamps + 3] = hw; rec[kNumStamps + 4] = xcc;
          rec[kNumStamps + 5] = rows; rec[kNumStamps + 7] = cons;
          rec[kNumStamps + 11] = prs; rec[kNumStamps + 13] = lvls;
        }
        if (k == 32) { rec[kNumStamps + 6] = rows; rec[kNumStamps + 8] = cons; rec[kNumStamps + 12] = prs; }
      } else {
        if (threadIdx.x < kNumStamps) {
          atomicAdd(p + threadIdx.x, acc[threadIdx.x]);
          atomicMax(p + 16 + threadIdx.x, acc[threadIdx.x]);  // slots 16..: per-phase maximum
        }
        if (threadIdx.x == 0) atomicMax(p + kNumStamps, tot);  // slot kNumStamps: the slowest wave's total
      }
    }
  }
};

// ------------------------------------------------------------------------------------------------
// Mask walks.  take_bit pops the lowest set bit (0 and !valid once the mask is empty); the walks run
// a wave-uniform number of iterations (the model's longest path / largest subtree) with several
// rows loaded per iteration, and add an invalid row as +0 (no-op), so the LDS loads of one
// iteration are independent of each other and of the running sum.
__device__ __forceinline__ int take_bit(uint32_t& m, bool& valid) {
  valid = m != 0u;
  const int l = valid ? __builtin_ctz(m) : 0;
  m &= m - 1u;
  return l;
}

// The dynamics walks read an invalid slot from row kZeroRow of their tables, which holds +0 (written
// in every substep by lane kZeroRow): adding it is the +0 a select would add, without the select.
// num_hinges <= AS_ACT_DIM keeps that row past every model's links.
constexpr int kZeroRow = LMAX - 1;
static_assert(AS_ACT_DIM + 1 <= kZeroRow, "zero row past the links");
__device__ __forceinline__ int take_bit_z(uint32_t& m) {
  const int l = m != 0u ? __builtin_ctz(m) : kZeroRow;
  m &= m - 1u;
  return l;
}

// acc += sum of rows[l] over the set bits l of `mask`, ascending, U rows per iteration.
template <int W, int U>
__device__ __forceinline__ void path_sum(uint32_t mask, int n_max, float (&acc)[W], const float (*rows)[W]) {
  for (int it = 0; it < n_max; it += U) {
    int l[U];
#pragma unroll
    for (int u = 0; u < U; ++u) l[u] = take_bit_z(mask);
    float x[U][W];
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int k = 0; k < W; ++k) x[u][k] = rows[l[u]][k];
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
      for (int k = 0; k < W; ++k) acc[k] += x[u][k];
  }
}

}  // namespace as
