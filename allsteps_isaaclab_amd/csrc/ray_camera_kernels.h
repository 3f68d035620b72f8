// ray_camera_kernels.h -- k_ray_camera, the ray-cast depth camera of cfg.camera (as_ray_camera).
// Semantics, formulas, tie rules and buffer layout: allsteps_ray_camera.h.  The kernel is not part of as_step: the
// env launches it when a camera built from the cfg is read or updated, so the default step keeps its launches.
// Reads root_pos, root_quat and stones of the state, the local directions and the per-env offsets; writes pose and
// the requested images only.  No host sync, no atomics, no LDS, no barrier.
#pragma once

#include <hip/hip_runtime.h>

#include "allsteps_kernels.h"
#include "allsteps_ray_camera.h"

namespace as {

// A workgroup is one env x a tile of kCamTile consecutive pixels: the pixels run along the lanes, the env is
// uniform.  So the env's pose, its offset and its 60 stone coordinates are uniform loads (k_ray_cast keeps the
// stones per lane in VGPRs; here they cost none), the camera's frame -- quat_w, q_inv, pos_w -- is uniform
// arithmetic formed once per wave, the per-lane loads of dirs [3][R] are three contiguous runs and the stores into
// the env-major images plane / camera [n][R] one contiguous run each (normals [n][R][3]: three dwords a lane, 12
// bytes apart, the run still dense).  The per-pixel work is one quat_apply, three reciprocals, the ground and 20
// branch-free slab tests, then the camera-frame rotation of t d.  A normal needs the box hit, whose index differs
// from lane to lane: its three coordinates are re-read from the state by that index (an L1 / L2 hit).  The env's
// rows are passed once more as kernel arguments of their own: const and __restrict__ there tell the compiler that
// no store of the kernel changes them, which is what lets the uniform loads be scalar ones.  Tail lanes (pixel >=
// R) re-read pixel R - 1 and store nothing.  Lane 0 of tile 0 writes pose.  The grid is (tiles, envs up to
// kCamGridY, env groups): no dimension grows with n beyond kCamGridY.
constexpr int kCamTile = 256;
constexpr int kCamGridY = 32768;

__global__ __launch_bounds__(kCamTile) void k_ray_camera(CamArgs P, const float* __restrict__ root_pos,
                                                         const float* __restrict__ root_quat,
                                                         const float* __restrict__ stones,
                                                         const float* __restrict__ offset,
                                                         const float* __restrict__ dirs) {
  const int n = P.n, R = P.num_rays;
  const int64_t e64 = (int64_t)blockIdx.z * kCamGridY + blockIdx.y;
  if (e64 >= n) return;  // uniform
  const int e = (int)e64;
  const int r = (int)blockIdx.x * kCamTile + (int)threadIdx.x;
  const bool valid = r < R;
  const int rr = valid ? r : R - 1;  // a tail lane re-reads the last pixel: in bounds, never stored

  float rp[3], rq[4], op[3], oq[4];
#pragma unroll
  for (int k = 0; k < 3; ++k) rp[k] = root_pos[(size_t)k * n + e];
#pragma unroll
  for (int k = 0; k < 4; ++k) rq[k] = root_quat[(size_t)k * n + e];
#pragma unroll
  for (int k = 0; k < 3; ++k) op[k] = offset[(size_t)k * n + e];
#pragma unroll
  for (int k = 0; k < 4; ++k) oq[k] = offset[(size_t)(3 + k) * n + e];
  CamFrame f;
  cam_frame(rp, rq, op, oq, f);
  if (blockIdx.x == 0 && threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < 3; ++k) P.pose[(size_t)k * n + e] = f.pos[k];
#pragma unroll
    for (int k = 0; k < 4; ++k) P.pose[(size_t)(3 + k) * n + e] = f.quat[k];
  }

  const float dir_l[3] = {dirs[cam_dir_index(0, rr, R)], dirs[cam_dir_index(1, rr, R)],
                          dirs[cam_dir_index(2, rr, R)]};
  const float half[3] = {P.half[0], P.half[1], P.half[2]};
  const bool ground = (P.surfaces & kRaySurfGround) != 0;
  const int ns = (P.surfaces & kRaySurfStones) ? P.num_steps : 0;
  float d[3], inv[3];
  ray_quat_apply(f.quat, dir_l, d);
  ray_inverse(d, inv);
  RayBest b;
  ray_begin(b);
  // (the surface mask is uniform: the ground is a uniform branch, a stone past ns a uniform select)
  if (ground) ray_ground(b, f.pos, d, inv, P.ground_z, kCamCastMax);
#pragma unroll
  for (int s = 0; s < AS_NUM_STONES; ++s) {
    const float c[3] = {stones[(size_t)(3 * s) * n + e], stones[(size_t)(3 * s + 1) * n + e],
                        stones[(size_t)(3 * s + 2) * n + e]};
    RayBest t = b;
    ray_stone(t, f.pos, d, inv, c, half, kCamCastMax, s);
    const bool on = s < ns;
    b.t = on ? t.t : b.t;
    b.surface = on ? t.surface : b.surface;
  }
  if (!valid) return;
  if (P.plane) P.plane[cam_pixel_index(e, r, R)] = cam_plane(f.q_inv, b.t, d, P.clipping, P.max_distance);
  if (P.camera) P.camera[cam_pixel_index(e, r, R)] = cam_clip_camera(b.t, P.clipping, P.max_distance);
  if (P.normals) {
    const int s = b.surface >= 0 ? b.surface : 0;  // b.surface < AS_NUM_STONES: in bounds
    const float c[3] = {P.stones[(size_t)(3 * s) * n + e], P.stones[(size_t)(3 * s + 1) * n + e],
                        P.stones[(size_t)(3 * s + 2) * n + e]};
    float nrm[3];
    cam_normal(b, f.pos, d, inv, c, half, nrm);
#pragma unroll
    for (int k = 0; k < 3; ++k) P.normals[cam_normal_index(e, r, k, R)] = nrm[k];
  }
}

}  // namespace as
