// ray_caster_kernels.h -- k_ray_cast, the ray-caster height scanner of cfg.height_scanner (as_ray_cast).
// Semantics, formulas, tie rules and buffer layout: allsteps_ray_caster.h.  The kernel is not part of as_step: the
// env launches it when a sensor built from the cfg is read or updated, so the default step keeps its launches.
// Reads root_pos, root_quat and stones of the state and the local rays; writes hits, surface and pose only.  No
// host sync, no atomics, no LDS.
#pragma once

#include <hip/hip_runtime.h>

#include "allsteps_kernels.h"
#include "allsteps_ray_caster.h"

namespace as {

// A workgroup is kRayEnvs envs x kRayWaves ray slices: threadIdx.x is the env, so envs run along the lanes of a
// wave and every state read (root_pos, root_quat, the 60 stone rows) and every store (hits [3][R][n], surface
// [R][n], pose [7][n]) is one contiguous run.  A slice -- threadIdx.y of blockIdx.y, wave-uniform -- is
// `chunk` consecutive rays; the host sizes it so that the grid has about kRayTargetWaves waves (two on every SIMD
// of the chip at 4096 envs x 187 rays, where lane = env alone would be 64 waves), never below kRayMinChunk rays
// over which the thread's loads are shared.  A thread loads its env's pose and its 20 stone centres once into
// registers (the stone loop is fully unrolled: constant indices), forms the frame's quaternion once (the yaw
// quaternion's atan2 / sincos / normalise, or the root's own) and then walks its rays: a ray's local start and
// direction are wave-uniform loads, the per-ray work is quat_apply, three reciprocals and 20 branch-free slab
// tests (selects, fminf, fmaxf).  Tail lanes re-read env n - 1 and store nothing; a slice past the last ray
// leaves at once (no barrier in the kernel).  Slice 0 writes pose.  `rays` is P.rays once more, as a kernel
// argument of its own: const and __restrict__ there tell the compiler that no store of the kernel changes it,
// which is what lets the uniform loads be scalar ones.  152 VGPRs (the 60 stone coordinates and their slab
// bounds stay in registers across the rays), no scratch, no spills.
constexpr int kRayEnvs = 64;
constexpr int kRayWaves = 4;
constexpr int kRayMinChunk = 4;
constexpr int kRayTargetWaves = 2048;

__global__ __launch_bounds__(kRayEnvs * kRayWaves) void k_ray_cast(RayArgs P, const float* __restrict__ rays) {
  const int n = P.n, R = P.num_rays;
  const int64_t e64 = (int64_t)blockIdx.x * kRayEnvs + threadIdx.x;
  const bool valid = e64 < n;
  const int e = valid ? (int)e64 : n - 1;  // a tail lane re-reads the last env: in bounds, never stored
  // (threadIdx.y is one value per wave -- blockDim.x is the wave size -- which the compiler is told here)
  const int slice = __builtin_amdgcn_readfirstlane((int)(blockIdx.y * kRayWaves + threadIdx.y));
  const int r0 = slice * P.chunk;
  if (r0 >= R) return;
  const int r1 = min(R, r0 + P.chunk);

  float pos[3], q[4], st[3 * AS_NUM_STONES];
#pragma unroll
  for (int k = 0; k < 3; ++k) pos[k] = P.root_pos[(size_t)k * n + e];
#pragma unroll
  for (int k = 0; k < 4; ++k) q[k] = P.root_quat[(size_t)k * n + e];
#pragma unroll
  for (int k = 0; k < 3 * AS_NUM_STONES; ++k) st[k] = P.stones[(size_t)k * n + e];
  if (slice == 0 && valid && P.pose) {
#pragma unroll
    for (int k = 0; k < 3; ++k) P.pose[(size_t)k * n + e] = pos[k];
#pragma unroll
    for (int k = 0; k < 4; ++k) P.pose[(size_t)(3 + k) * n + e] = q[k];
  }
  const bool yaw_only = P.attach_yaw_only != 0;
  float qf[4];
  ray_frame(q, yaw_only, qf);
  const float half[3] = {P.half[0], P.half[1], P.half[2]};
  const bool ground = (P.surfaces & kRaySurfGround) != 0;
  const int ns = (P.surfaces & kRaySurfStones) ? P.num_steps : 0;

  for (int r = r0; r < r1; ++r) {
    const float start_l[3] = {rays[ray_local_index(0, r, R)], rays[ray_local_index(1, r, R)],
                              rays[ray_local_index(2, r, R)]};
    const float dir_l[3] = {rays[ray_local_index(3, r, R)], rays[ray_local_index(4, r, R)],
                            rays[ray_local_index(5, r, R)]};
    float o[3], d[3], inv[3], hit[3];
    ray_world(pos, qf, yaw_only, start_l, dir_l, o, d);
    ray_inverse(d, inv);
    RayBest b;
    ray_begin(b);
    // (the surface mask is uniform: the ground is a uniform branch, a stone past ns a uniform select)
    if (ground) ray_ground(b, o, d, inv, P.ground_z, P.max_distance);
#pragma unroll
    for (int s = 0; s < AS_NUM_STONES; ++s) {
      const float c[3] = {st[3 * s], st[3 * s + 1], st[3 * s + 2]};
      RayBest t = b;
      ray_stone(t, o, d, inv, c, half, P.max_distance, s);
      const bool on = s < ns;
      b.t = on ? t.t : b.t;
      b.surface = on ? t.surface : b.surface;
    }
    ray_hit_point(b, o, d, hit);
    if (valid) {
#pragma unroll
      for (int k = 0; k < 3; ++k) P.hits[ray_hit_index(k, r, e, n, R)] = hit[k];
      if (P.surface) P.surface[ray_surface_index(r, e, n)] = (int8_t)b.surface;
    }
  }
}

}  // namespace as
