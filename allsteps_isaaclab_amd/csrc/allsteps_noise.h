// allsteps_noise.h -- the action / observation noise models: formulas, draws and stream layout.
//
// The reference's DirectRLEnv.step perturbs the action with cfg.action_noise_model before the physics and
// the policy observation with cfg.observation_noise_model after it (direct_rl_env.py:322-323, 379-380), and
// re-draws the models' per-env bias for the envs it resets (:578-581).  The models are those of
// isaaclab/utils/noise/noise_model.py: a term (constant / uniform / gaussian noise, operation add / scale /
// abs) and, for NoiseModelWithAdditiveBias, one bias per env drawn from a second term on reset.
//
// Formulas (float32, every operation rounded on its own -- the library is built with -ffp-contract=off --
// so they give torch's bits from the same draws; d the data, u a uniform draw, z a normal draw):
//              add                    scale                   abs
//   constant   d + b                  d * b                   0 + b
//   uniform    (d + u w) + lo         d * (u w + lo)          u w + lo           w = hi - lo, formed once
//   gaussian   (d + mean) + std z     d * (mean + std z)      mean + std z
// and model(d) = term(d) + bias[e] with a bias model.  A bias re-draw is bias[e] = bias_term(bias[e]): the
// old bias is the data, so `add` is a random walk and `abs` a fresh draw.
//
// Draws: Philox4x32-10 keyed by the env's seed, counter (env_id_offset + e, t[e], b, tag) -- the reset
// stream's layout (allsteps_device.h philox_block) with the per-env step counter t[e] in the slot that stream
// uses for the episode.  Block b covers columns 4b .. 4b + 3 of env e's row; a bias draw is block 0, word 0.
// Uniform draws are the block's four uniforms as they are; normal draws are Box-Muller pairs of them.
// k_noise_post (noise_kernels.h) advances t[e] by one per env step.
//
// Plain C++ with no HIP dependency: tests/noise_check.cpp runs all of it on the host.
#pragma once

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/allsteps.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define AS_NZ_FN __host__ __device__ __forceinline__
#else
#define AS_NZ_FN inline
#endif

namespace as {

// Philox tags of the four noise streams, in the style of kResetTag
constexpr uint32_t kNoiseActTag = 0x4e416374u;      // "NAct": action term
constexpr uint32_t kNoiseObsTag = 0x4e4f6273u;      // "NObs": observation term
constexpr uint32_t kNoiseActBiasTag = 0x4e416269u;  // "NAbi": action bias
constexpr uint32_t kNoiseObsBiasTag = 0x4e4f6269u;  // "NObi": observation bias

constexpr int kNoiseMaxCols = 256;  // a row's column quads fit one 64-lane wave

// philox_block of allsteps_device.h in plain C++ (integer arithmetic and an exact conversion: the same
// bits on the host, on the device and in the oracle's or_philox_block)
AS_NZ_FN void noise_philox_block(uint64_t seed, uint32_t env, uint32_t t, uint32_t b, uint32_t tag, float* out4) {
  uint32_t c0 = env, c1 = t, c2 = b, c3 = tag;
  uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c0 = n0; c1 = (uint32_t)p1; c2 = n2; c3 = (uint32_t)p0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  out4[0] = (float)(c0 >> 8) * (1.0f / 16777216.0f);
  out4[1] = (float)(c1 >> 8) * (1.0f / 16777216.0f);
  out4[2] = (float)(c2 >> 8) * (1.0f / 16777216.0f);
  out4[3] = (float)(c3 >> 8) * (1.0f / 16777216.0f);
}

// Box-Muller: (r cos a, r sin a) with r = sqrt(-2 ln(1 - u0)), a = 2 pi u1.  u0 in [0, 1) has 24 bits, so
// 1 - u0 is exact and lies in (0, 1]: no log of 0, r <= sqrt(48 ln 2).
AS_NZ_FN void noise_box_muller(float u0, float u1, float* z0, float* z1) {
  const float r = sqrtf(-2.0f * logf(1.0f - u0));
  const float a = 6.283185307179586f * u1;
  *z0 = r * cosf(a);
  *z1 = r * sinf(a);
}

AS_NZ_FN bool noise_kind_random(int kind) { return kind == AS_NOISE_UNIFORM || kind == AS_NOISE_GAUSSIAN; }

// one Philox block's four uniforms -> the four draws a term of `kind` consumes
AS_NZ_FN void noise_block_draws(int kind, const float* u4, float* x4) {
  if (kind == AS_NOISE_GAUSSIAN) {
    noise_box_muller(u4[0], u4[1], &x4[0], &x4[1]);
    noise_box_muller(u4[2], u4[3], &x4[2], &x4[3]);
  } else {
    x4[0] = u4[0]; x4[1] = u4[1]; x4[2] = u4[2]; x4[3] = u4[3];
  }
}

// the draw of a per-env bias: block 0, word 0
AS_NZ_FN float noise_bias_draw(int kind, uint64_t seed, uint32_t env, uint32_t t, uint32_t tag) {
  if (!noise_kind_random(kind)) return 0.f;
  float u4[4], z0, z1;
  noise_philox_block(seed, env, t, 0u, tag, u4);
  if (kind == AS_NOISE_UNIFORM) return u4[0];
  noise_box_muller(u4[0], u4[1], &z0, &z1);
  return z0;
}

// The nine term formulas.  x: the draw (unused by the constant term); p0 / p1: bias / - (constant),
// lo / w = hi - lo (uniform), mean / std (gaussian).
AS_NZ_FN float noise_term(int kind, int op, float d, float x, float p0, float p1) {
  if (kind == AS_NOISE_CONSTANT) {
    if (op == AS_NOISE_ADD) return d + p0;
    if (op == AS_NOISE_SCALE) return d * p0;
    return 0.0f + p0;
  }
  if (kind == AS_NOISE_UNIFORM) {
    const float uw = x * p1;
    if (op == AS_NOISE_ADD) return (d + uw) + p0;
    if (op == AS_NOISE_SCALE) return d * (uw + p0);
    return uw + p0;
  }
  const float sz = p1 * x;
  if (op == AS_NOISE_ADD) return (d + p0) + sz;
  if (op == AS_NOISE_SCALE) return d * (p0 + sz);
  return p0 + sz;
}

// NoiseModelWithAdditiveBias.apply: one more add
AS_NZ_FN float noise_add_bias(float v, float bias) { return v + bias; }

// Work mapping of the kernels: the column quads of an env's row sit on a group of G lanes of one wave, G the
// next power of two >= ceil(cols / 4) (16 for 59 columns, 8 for 21; 1 for a launch without columns), so
// that every lane of an env loads t[e] / bias[e] before the group's first lane stores them.
AS_NZ_FN int noise_group(int cols) {
  const int quads = (cols + 3) / 4;
  int g = 1;
  while (g < quads) g <<= 1;
  return g;
}

}  // namespace as
