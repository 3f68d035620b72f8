// allsteps_ray_caster.h -- the ray-caster height scanner over the ground and the stones (cfg.height_scanner).
//
// The reference's RayCaster (ray_caster.py:201-260) turns local rays into world rays from the pose of the body it
// is attached to and hands them to a warp mesh query; here the query is a closed-form test against the ground plane
// and the env's stones, axis-aligned boxes.  One ray of one env, every operation in float32 and rounded on its own
// (the library is built with -ffp-contract=off; no fmaf but inside as_atan2f / as_sincosf):
//
//   sensor frame   pos = root_pos[e], q = root_quat[e] (w, x, y, z)              ray_caster.py:225-240
//                  (no drift: drift_range other than (0, 0) is refused)
//   attach_yaw_only (ray_caster.py:243-247; math.py:567-579 quat_apply_yaw, :521-542 yaw_quat):
//     yaw  = as_atan2f(2 (qw qz + qx qy), 1 - 2 (qy qy + qz qz))                 math.py:537
//     s, c = as_sincosf(yaw / 2)                                                 math.py:539-540
//     nrm  = max(sqrtf(c c + s s), 1e-9)                                         math.py:92 normalize: the zeros
//     qf   = (c / nrm, 0, 0, s / nrm)                                            of x and y add nothing to the norm
//     start_w = quat_apply(qf, start_l) + pos;   dir_w = dir_l                   ray_caster.py:245-247
//   otherwise (ray_caster.py:248-252):
//     qf = q;  start_w = quat_apply(q, start_l) + pos;  dir_w = quat_apply(q, dir_l)
//   quat_apply(q, v) (math.py:545-564), a x b = (a1 b2 - a2 b1, a2 b0 - a0 b2, a0 b1 - a1 b0):
//     t = (xyz x v) * 2                                                          math.py:563
//     out = (v + w t) + xyz x t                                                  math.py:564
//   Directions are used as given, not normalised: distances are in units of |dir| (warp's mesh_query_ray).
//
//   One IEEE division per axis per ray: inv_k = 1 / dir_w[k], and every slab distance is a product with it,
//   ((c -+ h) - o) * inv_k -- NOT a division per plane.  This fixes the rounding: two roundings (reciprocal,
//   product) where a division has one.
//
//   ground (surface bit 0): the plane z = ground_z, hit when dir_w.z < 0 and t >= 0, t = (ground_z - o.z) inv_z
//   stones (surface bit 1): s in [0, num_steps), the closed box centre stones[3 s .. 3 s + 2] -+ stone_half.  Per
//     axis k: lo = c - h, hi = c + h;
//       dir_w[k] == 0:  near = -inf, far = +inf when lo <= o <= hi, else near = +inf, far = -inf (a miss)
//       otherwise:      t1 = (lo - o) inv, t2 = (hi - o) inv, near = fminf(t1, t2), far = fmaxf(t1, t2)
//     tn = max of the nears, tf = min of the fars; hit when tn <= tf and tf >= 0; t = tn when tn >= 0, else tf
//     (a ray that starts inside a box hits the far face, as a mesh without back-face culling answers).
//   result: the smallest t <= max_distance over the selected surfaces; a candidate replaces the best only when
//     its t is strictly smaller, and the order is ground, stone 0, stone 1, ...: on equal t the ground wins over
//     the stones, then the lowest stone index.  hit = start_w + t * dir_w (a product, then a sum); surface = the
//     stone index, -1 the ground, -2 a miss, whose hit is (+inf, +inf, +inf) (ops.py:70).
//
// Buffers, field-major / env-minor:
//   rays    [6][R]      local start xyz | dir xyz (after the cfg's offset: views._RayCaster)
//   hits    [3][R][n]
//   surface int8 [R][n] optional
//   pose    [7][n]      pos | quat as read, the reference's data.pos_w / quat_w stored at update time; optional
//
// Plain C++ with no HIP dependency: tests/ray_caster_check.cpp runs all of it on the host.
#pragma once

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/as_detmath.h"
#include "allsteps_contact_report.h"  // AS_CR_FN

namespace as {

enum { kRaySurfGround = 1, kRaySurfStones = 2, kRaySurfAll = 3 };
enum { kRayHitGround = -1, kRayMiss = -2 };
constexpr int kRayPoseRows = 7;

AS_CR_FN size_t ray_local_index(int k, int r, int R) { return (size_t)k * (size_t)R + (size_t)r; }
AS_CR_FN size_t ray_hit_index(int k, int r, int e, int n, int R) {
  return ((size_t)k * (size_t)R + (size_t)r) * (size_t)n + (size_t)e;
}
AS_CR_FN size_t ray_surface_index(int r, int e, int n) { return (size_t)r * (size_t)n + (size_t)e; }

// math.py:545-564 quat_apply, q = (w, x, y, z)
AS_CR_FN void ray_quat_apply(const float (&q)[4], const float (&v)[3], float (&o)[3]) {
  const float x = q[1], y = q[2], z = q[3], w = q[0];
  const float t0 = (y * v[2] - z * v[1]) * 2.f;
  const float t1 = (z * v[0] - x * v[2]) * 2.f;
  const float t2 = (x * v[1] - y * v[0]) * 2.f;
  o[0] = (v[0] + w * t0) + (y * t2 - z * t1);
  o[1] = (v[1] + w * t1) + (z * t0 - x * t2);
  o[2] = (v[2] + w * t2) + (x * t1 - y * t0);
}

// math.py:521-542 yaw_quat
AS_CR_FN void ray_yaw_quat(const float (&q)[4], float (&o)[4]) {
  const float qw = q[0], qx = q[1], qy = q[2], qz = q[3];
  const float yaw = as_atan2f(2.f * (qw * qz + qx * qy), 1.f - 2.f * (qy * qy + qz * qz));
  float s, c;
  as_sincosf(yaw / 2.f, &s, &c);
  const float nrm = fmaxf(sqrtf(c * c + s * s), 1e-9f);
  o[0] = c / nrm;
  o[1] = 0.f;
  o[2] = 0.f;
  o[3] = s / nrm;
}

// The quaternion the rays of an env are rotated by: formed once per env, not once per ray
AS_CR_FN void ray_frame(const float (&q)[4], bool attach_yaw_only, float (&qf)[4]) {
  if (attach_yaw_only) {
    ray_yaw_quat(q, qf);
  } else {
    for (int k = 0; k < 4; ++k) qf[k] = q[k];
  }
}

// ray_caster.py:243-252: a local ray in the world frame
AS_CR_FN void ray_world(const float (&pos)[3], const float (&qf)[4], bool attach_yaw_only, const float (&start_l)[3],
                        const float (&dir_l)[3], float (&o)[3], float (&d)[3]) {
  float s[3];
  ray_quat_apply(qf, start_l, s);
  for (int k = 0; k < 3; ++k) o[k] = s[k] + pos[k];
  if (attach_yaw_only) {
    for (int k = 0; k < 3; ++k) d[k] = dir_l[k];
  } else {
    ray_quat_apply(qf, dir_l, d);
  }
}

// One axis of the slab test: the ray's entry (near) and exit (far) distance of [c - h, c + h].  Selects only.
AS_CR_FN void ray_slab(float o, float d, float inv, float c, float h, float& near, float& far) {
  const float lo = c - h, hi = c + h;
  const float t1 = (lo - o) * inv, t2 = (hi - o) * inv;
  const bool par = d == 0.f;
  const bool in = o >= lo && o <= hi;
  near = par ? (in ? -INFINITY : INFINITY) : fminf(t1, t2);
  far = par ? (in ? INFINITY : -INFINITY) : fmaxf(t1, t2);
}

struct RayBest {
  float t;      // the smallest distance so far, +inf before any hit
  int surface;  // kRayMiss, kRayHitGround or the stone
};

AS_CR_FN void ray_begin(RayBest& b) {
  b.t = INFINITY;
  b.surface = kRayMiss;
}

// A candidate replaces the best only when strictly nearer (the tie rules follow from the order of the calls)
AS_CR_FN void ray_take(RayBest& b, bool hit, float t, float max_distance, int surface) {
  const bool better = hit && t <= max_distance && t < b.t;
  b.t = better ? t : b.t;
  b.surface = better ? surface : b.surface;
}

AS_CR_FN void ray_ground(RayBest& b, const float (&o)[3], const float (&d)[3], const float (&inv)[3], float ground_z,
                         float max_distance) {
  const float t = (ground_z - o[2]) * inv[2];
  ray_take(b, d[2] < 0.f && t >= 0.f, t, max_distance, kRayHitGround);
}

AS_CR_FN void ray_stone(RayBest& b, const float (&o)[3], const float (&d)[3], const float (&inv)[3],
                        const float (&c)[3], const float (&half)[3], float max_distance, int stone) {
  float n0, f0, n1, f1, n2, f2;
  ray_slab(o[0], d[0], inv[0], c[0], half[0], n0, f0);
  ray_slab(o[1], d[1], inv[1], c[1], half[1], n1, f1);
  ray_slab(o[2], d[2], inv[2], c[2], half[2], n2, f2);
  const float tn = fmaxf(fmaxf(n0, n1), n2), tf = fminf(fminf(f0, f1), f2);
  ray_take(b, tn <= tf && tf >= 0.f, tn >= 0.f ? tn : tf, max_distance, stone);
}

AS_CR_FN void ray_inverse(const float (&d)[3], float (&inv)[3]) {
  for (int k = 0; k < 3; ++k) inv[k] = 1.f / d[k];
}

AS_CR_FN void ray_hit_point(const RayBest& b, const float (&o)[3], const float (&d)[3], float (&hit)[3]) {
  for (int k = 0; k < 3; ++k) hit[k] = b.surface == kRayMiss ? INFINITY : o[k] + b.t * d[k];
}

// One ray of one env against everything: `stones` holds num_steps centres, xyz each
AS_CR_FN int ray_cast_one(const float (&pos)[3], const float (&qf)[4], bool attach_yaw_only, int surfaces,
                          const float (&start_l)[3], const float (&dir_l)[3], const float* stones, int num_steps,
                          const float (&half)[3], float ground_z, float max_distance, float (&hit)[3]) {
  float o[3], d[3], inv[3];
  ray_world(pos, qf, attach_yaw_only, start_l, dir_l, o, d);
  ray_inverse(d, inv);
  RayBest b;
  ray_begin(b);
  if (surfaces & kRaySurfGround) ray_ground(b, o, d, inv, ground_z, max_distance);
  if (surfaces & kRaySurfStones)
    for (int s = 0; s < num_steps; ++s) {
      const float c[3] = {stones[3 * s], stones[3 * s + 1], stones[3 * s + 2]};
      ray_stone(b, o, d, inv, c, half, max_distance, s);
    }
  ray_hit_point(b, o, d, hit);
  return b.surface;
}

}  // namespace as
