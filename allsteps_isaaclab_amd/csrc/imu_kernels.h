// imu_kernels.h -- k_imu, the IMU sensors of cfg.imu (as_imu).  Semantics, formulas and buffer layout:
// allsteps_imu.h.  Not part of as_step: the env launches it when a sensor's data is read while an env is outdated,
// or on update(force_recompute=True), so the default step keeps its launches.
//
// The launch shape is k_body_state's (two envs per one-wave workgroup): body_fk runs k_step's own fk<false> of the
// state as it stands and leaves the hinges' world axes in the dynamics scratch.  Lane s < num_sensors of an env
// then forms its body's as_body_state row (body_row, the function k_body_state stores from) in registers and runs
// imu_update on it.  An env that is not outdated (and `all` == 0) reads and writes neither prev nor data: its rows
// stay bit for bit.  The outdated flag is read by every lane before the first barrier and cleared by the env's
// lane 0 after its last use -- both in the env's own wave, so in program order.  The tail env of an odd n re-reads
// env n - 1 and stores nothing.  No atomics, no host sync; dt, the table and `all` are kernel arguments by value,
// so a captured launch replays what it was captured with.
#pragma once

#include <hip/hip_runtime.h>

#include "allsteps_imu.h"
#include "body_state_kernel.h"

namespace as {

__global__ __launch_bounds__(kStepThreads) void k_imu(ImuArgs P) {
  __shared__ Smem sm;
  const Consts& K = *(const Consts*)(CK*)P.consts;
  const int el = threadIdx.x >> 5, lane = threadIdx.x & 31;
  const int n = P.n;
  const int e_raw = blockIdx.x * EPB + el;
  const bool valid = e_raw < n;
  const int e = valid ? e_raw : n - 1;
  const bool outdated = P.all != 0 || P.outdated[e] != 0;
  float v0[3], w0[3];
  body_fk(K, P.st, sm, n, e, el, lane, v0, w0);
  const int S = P.imus.num_sensors;
  if (lane < S && valid && outdated) {
    const int s = lane;
    float row[AS_BODY_STATE_ROWS];
    body_row(K.model, sm, sm.env[el], v0, w0, P.imus.link[s], P.imus.body_offset_pos[s], P.imus.body_offset_quat[s],
             P.imus.com[s], row);
    ImuConst C;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      C.o[k] = P.imus.offset_pos[s][k];
      C.c[k] = P.imus.com[s][k];
      C.g[k] = P.imus.gravity_bias[s][k];
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) C.r[k] = P.imus.offset_rot[s][k];
    const float p[3] = {row[0], row[1], row[2]}, q[4] = {row[3], row[4], row[5], row[6]};
    const float w[3] = {row[10], row[11], row[12]}, v[3] = {row[13], row[14], row[15]};
    float prev[kImuPrevRows], data[kImuDataRows];
#pragma unroll
    for (int r = 0; r < kImuPrevRows; ++r) prev[r] = P.prev[imu_index(r, s, e, n, S)];
    imu_update(p, q, v, w, C, P.dt, prev, data);
#pragma unroll
    for (int r = 0; r < kImuDataRows; ++r) P.data[imu_index(r, s, e, n, S)] = data[r];
#pragma unroll
    for (int r = 0; r < kImuPrevRows; ++r) P.prev[imu_index(r, s, e, n, S)] = prev[r];
  }
  if (lane == 0 && valid && outdated) P.outdated[e] = 0;
}

}  // namespace as
