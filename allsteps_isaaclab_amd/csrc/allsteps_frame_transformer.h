// allsteps_frame_transformer.h -- the FrameTransformer sensor over the robot's bodies and the stones
// (cfg.frame_transformer).
//
// The reference's FrameTransformer (frame_transformer.py:322-385) reads the link poses of a source body and of a
// set of target bodies from PhysX, moves each by a constant offset and expresses every target in the source frame.
// One frame of one env, every operation in float32 and rounded on its own (the library is built with
// -ffp-contract=off; no fmaf here), quaternions (w, x, y, z):
//
//   inputs    ps, qs     the source body's link pose          a robot body: as_body_state rows 0:7
//             pt, qt     the target body's link pose          a stone s: state.stones rows 3 s .. 3 s + 2, (1, 0, 0, 0)
//   constants the source offset (os, rs) and the frame's offset (ot, rt); both rot are used as given, NOT
//             normalised, as in the reference; the two switches apply_source / apply_target (formed on the host as
//             the reference forms them, is_identity_pose: the target one per sensor, true if ANY frame's offset is
//             not identity -- an identity offset is then applied too, and quat_mul by (1, 0, 0, 0) is not a no-op)
//
//     source          = apply_source ? combine(ps, qs, os, rs) : (ps, qs)        :341-350
//     target_w        = apply_target ? combine(pt, qt, ot, rt) : (pt, qt)        :358-367
//     target_source   = subtract(source, target_w)                               :371-376
//
//   quat_apply(q, v) (math.py:546-564):   t = (xyz x v) 2;  out = (v + w t) + (xyz x t)
//   quat_inv(q) (math.py:239-248):        conj(q) / max(sqrt(((w w + x x) + y y) + z z), 1e-9)
//                                         the reference's norm fixes no summation order; this one is the header's
//   combine(t01, q01, t12, q12) (:749-782):   q02 = quat_mul(q01, q12);  t02 = t01 + quat_apply(q01, t12)
//   subtract(t01, q01, t02, q02) (:786-816):  q10 = quat_inv(q01);  q12 = quat_mul(q10, q02)
//                                             t12 = quat_apply(q10, t02 - t01)
//   quat_mul and the cross product are allsteps_imu.h's, as they are.
//
// The sensor keeps nothing between updates: the buffers are a function of the state.  Buffers, field-major /
// env-minor (S sensors, F target frames over all of them):
//   source [kFrameSourceRows = 7][S][n]    pos 3 | quat 4
//   target [kFrameTargetRows = 14][F][n]   pos_w 3 | quat_w 4 | pos_source 3 | quat_source 4
// Before the first update they hold zeros, as the reference's (:315-320).
//
// Plain C++ with no HIP dependency: tests/frame_transformer_check.cpp runs all of it on the host.
#pragma once

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "allsteps_imu.h"  // AS_CR_FN, imu_quat_mul, imu_cross, imu_index

namespace as {

enum { kFrameSourcePos = 0, kFrameSourceQuat = 3, kFrameSourceRows = 7 };
enum { kFramePosW = 0, kFrameQuatW = 3, kFramePosSource = 7, kFrameQuatSource = 10, kFrameTargetRows = 14 };

// [row][slot][env]: slot is the sensor of the source buffer (count S), the frame of the target buffer (count F)
AS_CR_FN size_t frame_index(int row, int slot, int e, int n, int count) { return imu_index(row, slot, e, n, count); }

// math.py:546-564
AS_CR_FN void frame_quat_apply(const float (&q)[4], const float (&v)[3], float (&o)[3]) {
  const float w = q[0];
  const float xyz[3] = {q[1], q[2], q[3]};
  float t[3], u[3];
  imu_cross(xyz, v, t);
  for (int k = 0; k < 3; ++k) t[k] = t[k] * 2.0f;
  imu_cross(xyz, t, u);
  for (int k = 0; k < 3; ++k) o[k] = (v[k] + w * t[k]) + u[k];
}

// math.py:239-248 (normalize(quat_conjugate(q)), eps = 1e-9)
AS_CR_FN void frame_quat_inv(const float (&q)[4], float (&o)[4]) {
  const float s = sqrtf(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]);
  const float d = s > 1e-9f ? s : 1e-9f;
  o[0] = q[0] / d;
  o[1] = -q[1] / d;
  o[2] = -q[2] / d;
  o[3] = -q[3] / d;
}

// math.py:749-782
AS_CR_FN void frame_combine(const float (&t01)[3], const float (&q01)[4], const float (&t12)[3], const float (&q12)[4],
                            float (&t02)[3], float (&q02)[4]) {
  float r[3];
  imu_quat_mul(q01, q12, q02);
  frame_quat_apply(q01, t12, r);
  for (int k = 0; k < 3; ++k) t02[k] = t01[k] + r[k];
}

// math.py:786-816
AS_CR_FN void frame_subtract(const float (&t01)[3], const float (&q01)[4], const float (&t02)[3],
                             const float (&q02)[4], float (&t12)[3], float (&q12)[4]) {
  float q10[4];
  frame_quat_inv(q01, q10);
  imu_quat_mul(q10, q02, q12);
  const float d[3] = {t02[0] - t01[0], t02[1] - t01[1], t02[2] - t01[2]};
  frame_quat_apply(q10, d, t12);
}

// A constant offset: pos, then rot (w, x, y, z) as given
struct FrameOffset {
  float pos[3];
  float rot[4];
};

// The source frame of a sensor from its body's link pose: source[kFrameSourceRows] out.
AS_CR_FN void frame_source(const float (&ps)[3], const float (&qs)[4], bool apply, const FrameOffset& off,
                           float (&source)[kFrameSourceRows]) {
  float p[3] = {ps[0], ps[1], ps[2]}, q[4] = {qs[0], qs[1], qs[2], qs[3]};
  if (apply) frame_combine(ps, qs, off.pos, off.rot, p, q);
  for (int k = 0; k < 3; ++k) source[kFrameSourcePos + k] = p[k];
  for (int k = 0; k < 4; ++k) source[kFrameSourceQuat + k] = q[k];
}

// One target frame from its body's link pose and the sensor's source frame: target[kFrameTargetRows] out.
AS_CR_FN void frame_target(const float (&source)[kFrameSourceRows], const float (&pt)[3], const float (&qt)[4],
                           bool apply, const FrameOffset& off, float (&target)[kFrameTargetRows]) {
  const float sp[3] = {source[0], source[1], source[2]}, sq[4] = {source[3], source[4], source[5], source[6]};
  float p[3] = {pt[0], pt[1], pt[2]}, q[4] = {qt[0], qt[1], qt[2], qt[3]};
  if (apply) frame_combine(pt, qt, off.pos, off.rot, p, q);
  float pr[3], qr[4];
  frame_subtract(sp, sq, p, q, pr, qr);
  for (int k = 0; k < 3; ++k) {
    target[kFramePosW + k] = p[k];
    target[kFramePosSource + k] = pr[k];
  }
  for (int k = 0; k < 4; ++k) {
    target[kFrameQuatW + k] = q[k];
    target[kFrameQuatSource + k] = qr[k];
  }
}

}  // namespace as
