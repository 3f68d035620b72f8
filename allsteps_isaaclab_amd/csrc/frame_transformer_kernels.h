// frame_transformer_kernels.h -- k_frame_transformer, the FrameTransformer sensors of cfg.frame_transformer
// (as_frame_transformer).  Semantics, formulas and buffer layout: allsteps_frame_transformer.h.  Not part of
// as_step: the env launches it when a sensor's data is read after the scene changed, or on
// update(force_recompute=True), so the default step keeps its launches.
//
// The launch shape is k_imu's (two envs per one-wave workgroup): body_fk runs k_step's own fk<false> of the state
// as it stands.  Lane f < num_frames of an env then forms its frame: the link pose of its sensor's source body
// and of its own target body -- a robot body through body_row (rows 0:7 only: the velocity chain is dead code
// here), a stone through three loads -- then frame_source and frame_target.  The source pose is recomputed in
// every lane of the sensor rather than handed over through LDS: the same function of the same inputs, so the same
// bits, and no third barrier.  The first lane of a sensor (the table groups the frames by sensor) stores the
// sensor's source rows.  The tail env of an odd n re-reads env n - 1 and stores nothing.  No atomics, no host
// sync; the table is a kernel argument by value (2.4 KB of the 4 KB), so a captured launch replays what it was
// captured with.
#pragma once

#include <hip/hip_runtime.h>

#include "allsteps_frame_transformer.h"
#include "body_state_kernel.h"

namespace as {

// The link pose of a table entry: a robot body (link >= 0) or stone `stone` of the env
__device__ __forceinline__ void frame_link_pose(const as_model_t& m, const Smem& sm, const EnvS& s,
                                                const float (&v0)[3], const float (&w0)[3], const as_frame_body_t& b,
                                                const float* stones, int n, int e, float (&p)[3], float (&q)[4]) {
  if (b.link >= 0) {
    float row[AS_BODY_STATE_ROWS];
    const float no_com[3] = {0.f, 0.f, 0.f};
    body_row(m, sm, s, v0, w0, b.link, b.body_offset_pos, b.body_offset_quat, no_com, row);
#pragma unroll
    for (int k = 0; k < 3; ++k) p[k] = row[k];
#pragma unroll
    for (int k = 0; k < 4; ++k) q[k] = row[3 + k];
  } else {
#pragma unroll
    for (int k = 0; k < 3; ++k) p[k] = stones[(size_t)(3 * b.stone + k) * n + e];
    q[0] = 1.f; q[1] = 0.f; q[2] = 0.f; q[3] = 0.f;
  }
}

__device__ __forceinline__ void frame_offset_of(const as_frame_body_t& b, FrameOffset& o) {
#pragma unroll
  for (int k = 0; k < 3; ++k) o.pos[k] = b.offset_pos[k];
#pragma unroll
  for (int k = 0; k < 4; ++k) o.rot[k] = b.offset_rot[k];
}

__global__ __launch_bounds__(kStepThreads) void k_frame_transformer(FrameTransformerArgs P) {
  __shared__ Smem sm;
  const Consts& K = *(const Consts*)(CK*)P.consts;
  const int el = threadIdx.x >> 5, lane = threadIdx.x & 31;
  const int n = P.n;
  const int e_raw = blockIdx.x * EPB + el;
  const bool valid = e_raw < n;
  const int e = valid ? e_raw : n - 1;
  float v0[3], w0[3];
  body_fk(K, P.st, sm, n, e, el, lane, v0, w0);
  const as_frame_table_t& T = P.frames;
  const int F = T.num_frames, S = T.num_sensors;
  if (lane < F && valid) {
    const int f = lane;
    const int s = T.sensor[f];
    const bool first = f == 0 || T.sensor[f - 1] != s;
    float p[3], q[4], source[kFrameSourceRows], target[kFrameTargetRows];
    FrameOffset off;
    frame_link_pose(K.model, sm, sm.env[el], v0, w0, T.source[s], P.st.stones, n, e, p, q);
    frame_offset_of(T.source[s], off);
    frame_source(p, q, T.apply_source_offset[s] != 0, off, source);
    frame_link_pose(K.model, sm, sm.env[el], v0, w0, T.target[f], P.st.stones, n, e, p, q);
    frame_offset_of(T.target[f], off);
    frame_target(source, p, q, T.apply_target_offset[s] != 0, off, target);
    if (first) {
#pragma unroll
      for (int r = 0; r < kFrameSourceRows; ++r) P.source[frame_index(r, s, e, n, S)] = source[r];
    }
#pragma unroll
    for (int r = 0; r < kFrameTargetRows; ++r) P.target[frame_index(r, f, e, n, F)] = target[r];
  }
}

}  // namespace as
