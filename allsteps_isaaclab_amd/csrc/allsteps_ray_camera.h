// allsteps_ray_camera.h -- the ray-cast depth camera over the ground and the stones (cfg.camera).
//
// The reference's RayCasterCamera (ray_caster_camera.py:257-318) rotates the pinhole pattern's local directions by
// the camera's world orientation, hands the rays to the warp mesh query and turns the hit distances back into the
// camera frame.  Here the query is the closed-form cast of allsteps_ray_caster.h (same formulas, same rounding
// order, same tie rules: ground, stone 0, stone 1, ...).  One pixel of one env, every operation in float32 and
// rounded on its own (the library is built with -ffp-contract=off; no fmaf here):
//
//   per env e (the camera is attached to the robot's root body, as the height scanner is):
//     view pose  p = root_pos[e], q = root_quat[e] (w, x, y, z)                    ray_caster_camera.py:394-413
//     pos_w   = p + quat_apply(q, off_pos[e])                                      :427
//     quat_w  = quat_mul(q, off_quat[e])                                           :428  off_quat is in the "world"
//               convention already and is used as given, NOT normalised, as in the reference
//     q_inv   = conj(quat_w) / max(sqrtf(((w w + x x) + y y) + z z), 1e-9f)        math.py:239-249 quat_inv ->
//               :82-92 normalize; torch fixes no order for the norm's sum, this one is the header's.  Four IEEE
//               divisions by the clamped norm.
//   per pixel r, local direction dir_l[r] (the pinhole pattern's ray starts are all zero):
//     o = pos_w                                                                    :269-270 (quat_apply(q, 0) = 0
//                                                                                  and 0 + pos_w = pos_w, exactly)
//     d = quat_apply(quat_w, dir_l[r])                                             :271
//     t, surface = the cast of allsteps_ray_caster.h over the selected surfaces with the distance cap
//                  kCamCastMax = 1e6f (:284) -- NOT cfg.max_distance; a miss has t = +inf
//     distance_to_camera = t, then the clip (:311-315)
//         max:  t > max ? max : t          zero:  t > max ? 0 : t          none: t
//     distance_to_image_plane = the x component of quat_apply(q_inv, (t d0, t d1, t d2))  (:293-298), then the clip
//         max:  x > max ? max : x, then NaN -> max       zero:  x > max ? 0 : x, then NaN -> 0       none: x
//       A miss is NOT special-cased: inf * d followed by the rotation is NaN in the reference and here (the cross
//       products subtract infinities; a zero component gives inf * 0).  Whatever NaN the arithmetic leaves is
//       stored as the canonical quiet NaN 0x7fc00000, so that host and device agree in its bits too.
//     normals = the outward unit normal of the face hit
//         ground:                             (0, 0, 1)
//         a stone entered from outside (t = tn): the first axis k (x, y, z) whose near distance equals tn;
//                                              -sign(d[k]) on that axis
//         a ray that starts inside (t = tf):   the first axis k whose far distance equals tf; +sign(d[k])
//         a miss:                              (+inf, +inf, +inf)   (ops.py:85)
//       (the axis chosen always has d[k] != 0: a parallel axis has near = -inf and far = +inf, which are the
//       entry / exit distance of a hit only when t is infinite, and that is a miss; sign(d) is then +-1)
//
// Buffers:
//   dirs    [3][R]      R = H W, row-major over the image: pixel (row v, column u) is ray v W + u
//   offset  [7][n]      off_pos | off_quat, env-minor (set_world_poses takes env_ids)
//   pose    [7][n]      pos_w | quat_w, the reference's data.pos_w / data.quat_w_world
//   plane   [n][R], camera [n][R], normals [n][R][3]     env-major and contiguous: the reference's (N, H, W, C)
//
// Plain C++ with no HIP dependency: tests/ray_camera_check.cpp runs all of it on the host.
#pragma once

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "allsteps_imu.h"         // imu_quat_mul
#include "allsteps_ray_caster.h"  // ray_quat_apply, ray_inverse, ray_ground, ray_stone, ray_slab, ray_take

namespace as {

enum { kCamClipNone = 0, kCamClipMax = 1, kCamClipZero = 2 };
constexpr float kCamCastMax = 1e6f;  // ray_caster_camera.py:284
constexpr int kCamPoseRows = 7;

AS_CR_FN size_t cam_dir_index(int k, int r, int R) { return (size_t)k * (size_t)R + (size_t)r; }
AS_CR_FN size_t cam_pixel_index(int e, int r, int R) { return (size_t)e * (size_t)R + (size_t)r; }
AS_CR_FN size_t cam_normal_index(int e, int r, int k, int R) {
  return ((size_t)e * (size_t)R + (size_t)r) * 3 + (size_t)k;
}

// The camera of one env: formed once per env, not once per pixel
struct CamFrame {
  float pos[3];    // pos_w
  float quat[4];   // quat_w ("world" convention)
  float q_inv[4];  // quat_inv(quat_w)
};

AS_CR_FN void cam_frame(const float (&root_pos)[3], const float (&root_quat)[4], const float (&off_pos)[3],
                        const float (&off_quat)[4], CamFrame& f) {
  float t[3];
  ray_quat_apply(root_quat, off_pos, t);
  for (int k = 0; k < 3; ++k) f.pos[k] = root_pos[k] + t[k];  // :427
  imu_quat_mul(root_quat, off_quat, f.quat);                  // :428
  const float w = f.quat[0], x = f.quat[1], y = f.quat[2], z = f.quat[3];
  const float nrm = fmaxf(sqrtf(((w * w + x * x) + y * y) + z * z), 1e-9f);
  f.q_inv[0] = w / nrm;
  f.q_inv[1] = -x / nrm;
  f.q_inv[2] = -y / nrm;
  f.q_inv[3] = -z / nrm;
}

// The cast of one world ray (o, d) over the selected surfaces; `stones` holds the env's centres, coordinate k of
// stone s at stones[(3 s + k) stride].  `inv` is left for cam_normal.
AS_CR_FN void cam_cast(const float (&o)[3], const float (&d)[3], int surfaces, const float* stones, size_t stride,
                       int num_steps, const float (&half)[3], float ground_z, float (&inv)[3], RayBest& b) {
  ray_inverse(d, inv);
  ray_begin(b);
  if (surfaces & kRaySurfGround) ray_ground(b, o, d, inv, ground_z, kCamCastMax);
  if (surfaces & kRaySurfStones)
    for (int s = 0; s < num_steps; ++s) {
      const float c[3] = {stones[(size_t)(3 * s) * stride], stones[(size_t)(3 * s + 1) * stride],
                          stones[(size_t)(3 * s + 2) * stride]};
      ray_stone(b, o, d, inv, c, half, kCamCastMax, s);
    }
}

// :311-315
AS_CR_FN float cam_clip_camera(float t, int clipping, float max_distance) {
  if (clipping == kCamClipMax) return t > max_distance ? max_distance : t;
  if (clipping == kCamClipZero) return t > max_distance ? 0.f : t;
  return t;
}

AS_CR_FN float cam_nan() { return __builtin_nanf(""); }  // the canonical quiet NaN, 0x7fc00000

// :293-305
AS_CR_FN float cam_plane(const float (&q_inv)[4], float t, const float (&d)[3], int clipping, float max_distance) {
  const float v[3] = {t * d[0], t * d[1], t * d[2]};
  float c[3];
  ray_quat_apply(q_inv, v, c);
  float x = c[0];
  x = x != x ? cam_nan() : x;  // one NaN for every target (an x86 host makes -NaN of inf - inf, the GPU +NaN)
  if (clipping == kCamClipMax) {
    x = x > max_distance ? max_distance : x;
    x = x != x ? max_distance : x;
  } else if (clipping == kCamClipZero) {
    x = x > max_distance ? 0.f : x;
    x = x != x ? 0.f : x;
  }
  return x;
}

// The outward normal of the face the best hit lies on; `c` is the centre of stone max(b.surface, 0)
AS_CR_FN void cam_normal(const RayBest& b, const float (&o)[3], const float (&d)[3], const float (&inv)[3],
                         const float (&c)[3], const float (&half)[3], float (&nrm)[3]) {
  float nr[3], fr[3];
  for (int k = 0; k < 3; ++k) ray_slab(o[k], d[k], inv[k], c[k], half[k], nr[k], fr[k]);
  const float tn = fmaxf(fmaxf(nr[0], nr[1]), nr[2]), tf = fminf(fminf(fr[0], fr[1]), fr[2]);
  const bool outside = tn >= 0.f;  // ray_stone: t = tn when tn >= 0, else tf
  const int axis = outside ? (nr[0] == tn ? 0 : nr[1] == tn ? 1 : 2) : (fr[0] == tf ? 0 : fr[1] == tf ? 1 : 2);
  const float da = axis == 0 ? d[0] : axis == 1 ? d[1] : d[2];
  const float s = (da > 0.f) == outside ? -1.f : 1.f;  // -sign(d) entering, +sign(d) leaving
  const bool stone = b.surface >= 0, miss = b.surface == kRayMiss;
  for (int k = 0; k < 3; ++k) {
    const float ground = k == 2 ? 1.f : 0.f;
    const float face = k == axis ? s : 0.f;
    nrm[k] = miss ? INFINITY : stone ? face : ground;
  }
}

struct CamPixel {
  float plane, camera, normal[3];
  float t;
  int surface;
  float d[3];  // the world direction handed to the cast
};

// One pixel of one env against everything, the header's one-call form
AS_CR_FN void cam_pixel_one(const CamFrame& f, const float (&dir_l)[3], int surfaces, int clipping,
                            float max_distance, const float* stones, size_t stride, int num_steps,
                            const float (&half)[3], float ground_z, CamPixel& px) {
  float inv[3];
  ray_quat_apply(f.quat, dir_l, px.d);  // :271
  RayBest b;
  cam_cast(f.pos, px.d, surfaces, stones, stride, num_steps, half, ground_z, inv, b);
  px.t = b.t;
  px.surface = b.surface;
  px.camera = cam_clip_camera(b.t, clipping, max_distance);
  px.plane = cam_plane(f.q_inv, b.t, px.d, clipping, max_distance);
  const int s = b.surface >= 0 ? b.surface : 0;
  const float c[3] = {stones[(size_t)(3 * s) * stride], stones[(size_t)(3 * s + 1) * stride],
                      stones[(size_t)(3 * s + 2) * stride]};
  cam_normal(b, f.pos, px.d, inv, c, half, px.normal);
}

}  // namespace as
