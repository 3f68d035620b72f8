// allsteps_base_frame.h -- the base-frame expressions of the reference's articulation data (root_lin_vel_b,
// root_ang_vel_b, projected_gravity_b, heading_w), shared by the command terms (allsteps_commands.h) and the
// observation terms (allsteps_observations.h).
//
// Float32, every operation rounded on its own (the library is built with -ffp-contract=off) except where torch's
// own kernels are compiled with a contracted multiply-add: a cross product's a1 b2 - a2 b1 is
// fmaf(a1, b2, -(a2 b1)).  tests/golden/gen_commands.py established these forms against real torch bit for bit;
// fmaf is correctly rounded on the host and on the device alike.
//
// Plain C++ with no HIP dependency.
#pragma once

#include <math.h>

#include "allsteps_noise.h"

// the short loops over components are unrolled on the device, so that the values stay in registers
#if defined(__HIPCC__) || defined(__CUDACC__)
#define AS_BF_UNROLL _Pragma("unroll")
#else
#define AS_BF_UNROLL
#endif

namespace as {

// torch.cross / Tensor.cross: the kernel's a1 b2 - a2 b1 is compiled as one fused multiply-add over the rounded
// second product (established against torch by the fixture: the separately rounded form misses its bits)
AS_NZ_FN void base_cross(const float (&a)[3], const float (&b)[3], float (&o)[3]) {
  o[0] = fmaf(a[1], b[2], -(a[2] * b[1]));
  o[1] = fmaf(a[2], b[0], -(a[0] * b[2]));
  o[2] = fmaf(a[0], b[1], -(a[1] * b[0]));
}

// math.py:606-625 quat_rotate_inverse, the dot product (a bmm) in the order (x u0 + y u1) + z u2, each operation
// rounded
AS_NZ_FN void base_rotate_inverse(const float (&q)[4], const float (&u)[3], float (&o)[3]) {
  const float qw = q[0];
  const float xyz[3] = {q[1], q[2], q[3]};
  const float s = 2.0f * (qw * qw) - 1.0f;
  float x[3];
  base_cross(xyz, u, x);
  const float dot = (xyz[0] * u[0] + xyz[1] * u[1]) + xyz[2] * u[2];
  AS_BF_UNROLL
  for (int k = 0; k < 3; ++k) {
    const float a = u[k] * s;
    const float b = (x[k] * qw) * 2.0f;
    const float cc = (xyz[k] * dot) * 2.0f;
    o[k] = (a - b) + cc;
  }
}

// articulation_data.py heading_w's forward vector: quat_apply(q, (1, 0, 0)) (math.py:546-564)
AS_NZ_FN void base_forward(const float (&q)[4], float (&fwd)[3]) {
  const float xyz[3] = {q[1], q[2], q[3]};
  const float v[3] = {1.0f, 0.0f, 0.0f};
  float t[3], x[3];
  base_cross(xyz, v, t);
  AS_BF_UNROLL
  for (int k = 0; k < 3; ++k) t[k] = t[k] * 2.0f;
  base_cross(xyz, t, x);
  AS_BF_UNROLL
  for (int k = 0; k < 3; ++k) fwd[k] = (v[k] + q[0] * t[k]) + x[k];
}

}  // namespace as
