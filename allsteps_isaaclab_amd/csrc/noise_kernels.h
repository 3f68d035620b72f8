// noise_kernels.h -- k_noise_actions / k_noise_post, the opt-in action and observation noise models
// (as_noise_actions / as_noise_post).  Formulas, draws and stream layout: allsteps_noise.h.  Neither kernel
// is part of as_step: the env launches them around it when its cfg names a model, so the default step keeps
// its launches.  No host sync, no atomics, no LDS.
#pragma once

#include <hip/hip_runtime.h>

#include "allsteps_kernels.h"
#include "allsteps_noise.h"

namespace as {

// One thread per (env, column quad), flat over the row-major buffer: thread g serves env g >> gshift, quad
// g & (G - 1), G = 1 << gshift = noise_group(cols) lanes per env.  Scalar 4-byte accesses (a 59-float row is
// 236 B: its quads are not 16-B aligned); neighbouring lanes touch neighbouring 16 B.  G divides the wave, so
// an env's lanes share a wave: the one load instruction that reads t[e] / bias[e] for all of them precedes,
// in the wave's program order, the store by which the group's first lane replaces them -- no double buffer
// (a replayed graph has fixed pointers) and no second launch.
constexpr int kNoiseThreads = 256;

// the quad's columns of one row through the model's term and bias; in == out: in place
__device__ __forceinline__ void noise_apply_quad(const as_noise_model_t& m, const float* in, float* out, size_t row,
                                                 int cols, int b, bool has_bias, float bias, const float* draws,
                                                 uint64_t seed, uint32_t env, uint32_t t, uint32_t tag) {
  const int c0 = 4 * b;
  if (c0 >= cols) return;
  float x[4] = {0.f, 0.f, 0.f, 0.f};
  if (noise_kind_random(m.kind)) {
    if (draws) {
#pragma unroll
      for (int k = 0; k < 4; ++k)
        if (c0 + k < cols) x[k] = draws[row + (size_t)(c0 + k)];
    } else {
      float u[4];
      noise_philox_block(seed, env, t, (uint32_t)b, tag, u);
      noise_block_draws(m.kind, u, x);
    }
  }
  float v[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int c = c0 + k;
    if (c < cols) {
      const float p1 = m.kind == AS_NOISE_CONSTANT ? 0.f : m.p1[c];
      v[k] = noise_term(m.kind, m.op, in[row + (size_t)c], x[k], m.p0[c], p1);
      if (has_bias) v[k] = noise_add_bias(v[k], bias);
    }
  }
#pragma unroll
  for (int k = 0; k < 4; ++k)
    if (c0 + k < cols) out[row + (size_t)(c0 + k)] = v[k];
}

__global__ __launch_bounds__(kNoiseThreads) void k_noise_actions(NoiseActArgs P) {
  const int64_t g = (int64_t)blockIdx.x * kNoiseThreads + threadIdx.x;
  const int64_t e = g >> P.gshift;
  if (e >= P.n) return;
  const int b = (int)(g & ((1 << P.gshift) - 1));
  const bool has_bias = P.m.bias_kind != AS_NOISE_NONE;
  const float bias = has_bias ? P.m.bias[e] : 0.f;
  noise_apply_quad(P.m, P.in, P.out, (size_t)e * (size_t)P.cols, P.cols, b, has_bias, bias, P.draws, P.seed,
                   (uint32_t)(P.env_offset + e), P.t[e], kNoiseActTag);
}

// bias[e] after this call: re-drawn from its own term for a reset env (the old bias is the term's data)
__device__ __forceinline__ float noise_next_bias(const as_noise_model_t& m, float old, bool reset, const float* draws,
                                                 int64_t e, uint64_t seed, uint32_t env, uint32_t t, uint32_t tag) {
  if (!reset) return old;
  const float x = !noise_kind_random(m.bias_kind) ? 0.f
                  : draws                         ? draws[e]
                                                  : noise_bias_draw(m.bias_kind, seed, env, t, tag);
  return noise_term(m.bias_kind, m.bias_op, old, x, m.bias_p0, m.bias_p1);
}

__global__ __launch_bounds__(kNoiseThreads) void k_noise_post(NoisePostArgs P) {
  const int64_t g = (int64_t)blockIdx.x * kNoiseThreads + threadIdx.x;
  const int64_t e = g >> P.gshift;
  if (e >= P.n) return;
  const int b = (int)(g & ((1 << P.gshift) - 1));
  const uint32_t t = P.t[e];
  const uint32_t env = (uint32_t)(P.env_offset + e);
  const bool reset = P.reset ? (P.reset[e] | (P.reset2 ? P.reset2[e] : (uint8_t)0)) != 0 : true;
  // every lane of the env forms the observation bias it adds (the same draw, the same bits); lane 0 stores it
  const bool obs_bias = P.obs.kind != AS_NOISE_NONE && P.obs.bias_kind != AS_NOISE_NONE;
  float ob = 0.f;
  if (obs_bias)
    ob = noise_next_bias(P.obs, P.obs.bias[e], reset, P.obs_bias_draws, e, P.seed, env, t, kNoiseObsBiasTag);
  if (P.data && P.obs.kind != AS_NOISE_NONE)
    noise_apply_quad(P.obs, P.data, P.data, (size_t)e * (size_t)P.cols, P.cols, b, obs_bias, ob, P.obs_draws, P.seed,
                     env, t, kNoiseObsTag);
  if (b != 0) return;
  if (obs_bias && reset) P.obs.bias[e] = ob;
  if (P.act.kind != AS_NOISE_NONE && P.act.bias_kind != AS_NOISE_NONE && reset)
    P.act.bias[e] = noise_next_bias(P.act, P.act.bias[e], true, P.act_bias_draws, e, P.seed, env, t, kNoiseActBiasTag);
  P.t[e] = t + 1u;
}

}  // namespace as
