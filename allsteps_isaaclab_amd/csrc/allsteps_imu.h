// allsteps_imu.h -- the IMU sensor on any robot body (cfg.imu).
//
// The reference's Imu (imu.py:142-203) reads a rigid body's link pose and centre-of-mass velocities from PhysX and
// differences the velocities against the ones of its previous update.  One update of one sensor of one env, every
// operation in float32 and rounded on its own (the library is built with -ffp-contract=off; no fmaf here):
//
//   inputs    p, q (w, x, y, z)   the body's link pose                     as_body_state rows 0:7
//             v, w                the body's COM linear / angular velocity rows 13:16, 10:13 (PhysX get_velocities)
//   constants o = offset.pos, r = offset.rot (used as given, NOT normalised, as in the reference),
//             c = the body's COM in its frame (as_body_table_t.com), g = gravity_bias, dt
//   state     prev_v, prev_w      the world velocities the previous update of this env left
//
//     pos_w     = p + quat_rotate(q, o)                                     imu.py:157
//     quat_w    = quat_mul(q, r)                                            imu.py:158
//     lin_vel_w = v + cross(w, quat_rotate(q, o - c))                       imu.py:167-169
//     lin_acc_w = (lin_vel_w - prev_v) / dt + g                             imu.py:172  an IEEE division, then the sum
//     ang_acc_w = (w - prev_w) / dt                                         imu.py:173
//     lin_vel_b = quat_rotate_inverse(quat_w, lin_vel_w)                    imu.py:175
//     ang_vel_b = quat_rotate_inverse(quat_w, w)                            imu.py:176
//     lin_acc_b = quat_rotate_inverse(quat_w, lin_acc_w)                    imu.py:178
//     ang_acc_b = quat_rotate_inverse(quat_w, ang_acc_w)                    imu.py:179
//     prev_v, prev_w = lin_vel_w, w                                         imu.py:181-182
//
//   quat_mul(q1, q2) (math.py:489-497, that form and order):
//     ww = (z1 + x1) (x2 + y2);  yy = (w1 - y1) (w2 + z2);  zz = (w1 + y1) (w2 - z2);  xx = (ww + yy) + zz
//     qq = 0.5 (xx + (z1 - x1) (x2 - y2))
//     w = (qq - ww) + (z1 - y1) (y2 - z2);   x = (qq - xx) + (x1 + w1) (x2 + w2)
//     y = (qq - yy) + (w1 - x1) (y2 + z2);   z = (qq - zz) + (z1 + y1) (w2 - x2)
//   quat_rotate / quat_rotate_inverse(q, u) (math.py:583-625), a x b = (a1 b2 - a2 b1, a2 b0 - a0 b2, a0 b1 - a1 b0):
//     a = u (2 (qw qw) - 1)
//     b = ((xyz x u) qw) 2
//     c = (xyz ((x u0 + y u1) + z u2)) 2          the reference's bmm fixes no order for the dot product; this one
//     out = (a + b) + c    /    (a - b) + c       is the header's
//
// The first update of an env has prev = 0: the acceleration is v / dt + g, as in the reference.  Imu.reset(env_ids)
// (imu.py:92-103) zeroes the data rows of the reset envs and marks them outdated but does NOT clear prev_v / prev_w;
// the zeroed rows are never visible, because an outdated env is recomputed before its data is handed out.  So
// nothing here zeroes anything: a reset only flags the env, and the next update differences against the old prev.
//
// Lazy update (sensor_base.py:284-293): an env carries an outdated flag; an update recomputes exactly the flagged
// envs (or all of them) and clears their flags; an unflagged env keeps its data rows and its prev bit for bit.
//
// Buffers, field-major / env-minor (S sensors):
//   data     [kImuDataRows = 19][S][n]   pos_w 3 | quat_w 4 | lin_vel_b 3 | ang_vel_b 3 | lin_acc_b 3 | ang_acc_b 3
//   prev     [kImuPrevRows = 6][S][n]    prev_v 3 | prev_w 3
//   outdated uint8 [n]
//
// Plain C++ with no HIP dependency: tests/imu_check.cpp runs all of it on the host.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "allsteps_contact_report.h"  // AS_CR_FN

namespace as {

enum { kImuPos = 0, kImuQuat = 3, kImuLinVel = 7, kImuAngVel = 10, kImuLinAcc = 13, kImuAngAcc = 16, kImuDataRows = 19 };
enum { kImuPrevLin = 0, kImuPrevAng = 3, kImuPrevRows = 6 };

AS_CR_FN size_t imu_index(int row, int s, int e, int n, int S) {
  return ((size_t)row * (size_t)S + (size_t)s) * (size_t)n + (size_t)e;
}

// The constants of one sensor
struct ImuConst {
  float o[3];  // offset.pos
  float r[4];  // offset.rot (w, x, y, z), as given
  float c[3];  // the body's COM in its frame
  float g[3];  // gravity_bias
};

AS_CR_FN void imu_cross(const float (&a)[3], const float (&b)[3], float (&o)[3]) {
  o[0] = a[1] * b[2] - a[2] * b[1];
  o[1] = a[2] * b[0] - a[0] * b[2];
  o[2] = a[0] * b[1] - a[1] * b[0];
}

// math.py:489-497
AS_CR_FN void imu_quat_mul(const float (&q1)[4], const float (&q2)[4], float (&o)[4]) {
  const float w1 = q1[0], x1 = q1[1], y1 = q1[2], z1 = q1[3];
  const float w2 = q2[0], x2 = q2[1], y2 = q2[2], z2 = q2[3];
  const float ww = (z1 + x1) * (x2 + y2);
  const float yy = (w1 - y1) * (w2 + z2);
  const float zz = (w1 + y1) * (w2 - z2);
  const float xx = (ww + yy) + zz;
  const float qq = 0.5f * (xx + (z1 - x1) * (x2 - y2));
  o[0] = (qq - ww) + (z1 - y1) * (y2 - z2);
  o[1] = (qq - xx) + (x1 + w1) * (x2 + w2);
  o[2] = (qq - yy) + (w1 - x1) * (y2 + z2);
  o[3] = (qq - zz) + (z1 + y1) * (w2 - x2);
}

// math.py:583-602 (inverse = false) and :606-625 (inverse = true)
AS_CR_FN void imu_quat_rotate(const float (&q)[4], const float (&u)[3], bool inverse, float (&o)[3]) {
  const float qw = q[0];
  const float xyz[3] = {q[1], q[2], q[3]};
  const float s = 2.0f * (qw * qw) - 1.0f;
  float x[3];
  imu_cross(xyz, u, x);
  const float dot = (xyz[0] * u[0] + xyz[1] * u[1]) + xyz[2] * u[2];
  for (int k = 0; k < 3; ++k) {
    const float a = u[k] * s;
    const float b = (x[k] * qw) * 2.0f;
    const float c = (xyz[k] * dot) * 2.0f;
    o[k] = (inverse ? a - b : a + b) + c;
  }
}

// One update of one sensor of one outdated env: data[kImuDataRows] out, prev[kImuPrevRows] in and out.
AS_CR_FN void imu_update(const float (&p)[3], const float (&q)[4], const float (&v)[3], const float (&w)[3],
                         const ImuConst& K, float dt, float (&prev)[kImuPrevRows], float (&data)[kImuDataRows]) {
  float t[3], quat_w[4];
  imu_quat_rotate(q, K.o, false, t);
  for (int k = 0; k < 3; ++k) data[kImuPos + k] = p[k] + t[k];                     // :157
  imu_quat_mul(q, K.r, quat_w);                                                    // :158
  for (int k = 0; k < 4; ++k) data[kImuQuat + k] = quat_w[k];
  const float oc[3] = {K.o[0] - K.c[0], K.o[1] - K.c[1], K.o[2] - K.c[2]};
  float arm[3], x[3], lin_vel_w[3], lin_acc_w[3], ang_acc_w[3];
  imu_quat_rotate(q, oc, false, arm);
  imu_cross(w, arm, x);
  for (int k = 0; k < 3; ++k) lin_vel_w[k] = v[k] + x[k];                          // :167-169
  for (int k = 0; k < 3; ++k) {
    lin_acc_w[k] = (lin_vel_w[k] - prev[kImuPrevLin + k]) / dt + K.g[k];           // :172
    ang_acc_w[k] = (w[k] - prev[kImuPrevAng + k]) / dt;                            // :173
  }
  float b[3];
  imu_quat_rotate(quat_w, lin_vel_w, true, b);                                     // :175
  for (int k = 0; k < 3; ++k) data[kImuLinVel + k] = b[k];
  imu_quat_rotate(quat_w, w, true, b);                                             // :176
  for (int k = 0; k < 3; ++k) data[kImuAngVel + k] = b[k];
  imu_quat_rotate(quat_w, lin_acc_w, true, b);                                     // :178
  for (int k = 0; k < 3; ++k) data[kImuLinAcc + k] = b[k];
  imu_quat_rotate(quat_w, ang_acc_w, true, b);                                     // :179
  for (int k = 0; k < 3; ++k) data[kImuAngAcc + k] = b[k];
  for (int k = 0; k < 3; ++k) {                                                    // :181-182
    prev[kImuPrevLin + k] = lin_vel_w[k];
    prev[kImuPrevAng + k] = w[k];
  }
}

}  // namespace as
