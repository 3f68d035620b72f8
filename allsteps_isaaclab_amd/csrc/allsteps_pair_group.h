// allsteps_pair_group.h -- the capsule bisection of collide()'s pass B run by a group of lanes.
//
// The sequential search (oracle/physics.c collide(), kBisectIters = 12 rounds) halves [lo, hi] once per
// round on the sign of sd_box_slope at t = 0.5 (lo + hi).  lo and hi stay multiples of 2^-12 in [0, 1],
// so every t is exact.  A group of 2^L lanes owns one pair and runs L of those rounds at once: sub-lane
// k < 2^L - 1 evaluates the slope at lo + (k + 1) (hi - lo) / 2^L -- the 2^L - 1 points are exactly the
// midpoints the sequential loop can reach in its next L rounds, each formed without rounding, so each is
// the same float the loop would pass to sd_box_slope -- and every lane then walks the L decisions on the
// group's sign bits (bit k = sub-lane k's "slope > 0").  After 12 / L such rounds lo and hi are the
// sequential loop's, bit for bit, whatever the signs are: the walk follows the same decisions, it does
// not assume they are monotone.  The group keeps lo and the width d = hi - lo (a power of two): hi is
// lo + d, exact like every other value here, so products and sums may as well be fused.
//
// Plain C++ with no HIP dependency: tests/pair_group_check.cpp runs the group serially on the host.
#pragma once

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define AS_PG_FN __host__ __device__ __forceinline__
#else
#define AS_PG_FN inline
#endif

namespace as {

constexpr int kPairGroupIters = 12;  // the sequential rounds (kBisectIters); L must divide it

// 2^-L for the group levels L = 2, 3, 4 (L sequential rounds per group round, 4, 8 or 16 lanes per pair)
AS_PG_FN float pair_group_scale(int L) { return L == 4 ? 0.0625f : (L == 3 ? 0.125f : 0.25f); }

// Level for a wave whose larger pending-pair count is `npairs`, capped at `cap` (1: never group): the
// largest L with npairs <= 32 >> L, or 0 when even L = 2 does not hold them (one lane per pair).
AS_PG_FN int pair_group_level(int npairs, int cap) {
  const int L = npairs <= 2 ? 4 : (npairs <= 4 ? 3 : (npairs <= 8 ? 2 : 0));
  const int Lc = L < cap ? L : cap;
  return Lc >= 2 ? Lc : 0;
}

// The point sub-lane k of a 2^L-lane group evaluates: w = d 2^-L.  (k = 2^L - 1 gives hi: that lane's
// sign is not read.)
AS_PG_FN float pair_group_point(float lo, float w, int k) { return fmaf((float)(k + 1), w, lo); }

// One round of the one-lane loop on the group's signs.  The interval is [li, li + 2 half] in units of w, so
// only li is tracked: the sign at the midpoint li + half (bit li + half of b2 = bits << 1) keeps li ("up":
// hi <- t) or moves it there.
AS_PG_FN int pair_group_step(int li, uint32_t b2, int half) {
  const int mi = li + half;
  return ((b2 >> mi) & 1u) != 0u ? li : mi;
}
// L sequential rounds on the group's sign bits: lo <- the lower end of the interval the one-lane loop
// holds after L more rounds; its width is w.  Four steps written out, no loop and no branch (a loop over L
// costs a taken branch per decision on the GPU): past the L-th step half is 0 and li stays.
AS_PG_FN void pair_group_walk(float& lo, float w, int L, uint32_t bits) {
  const uint32_t b2 = bits << 1;
  const int n = 1 << L;
  int li = pair_group_step(0, b2, n >> 1);
  li = pair_group_step(li, b2, n >> 2);
  li = pair_group_step(li, b2, n >> 3);
  li = pair_group_step(li, b2, n >> 4);
  lo = fmaf((float)li, w, lo);
}

}  // namespace as
