// allsteps_observations.h -- the observation manager's term groups (cfg.observations): the term values, the
// post-processing, the history rule, the draw layout and the Philox stream.
//
// The reference's ObservationManager.compute_group (managers/observation_manager.py:260-335) evaluates a group's
// terms in cfg order; per term: the term function (envs/mdp/observations.py), noise, clip, scale, then an optional
// history (utils/buffers/circular_buffer.py), and concatenates the results along the last dimension.  Float32, every
// operation rounded on its own (the library is built with -ffp-contract=off), so the same inputs and draws give
// torch's bits.
//
// A group's columns before the history ("pre-history columns", d0 of them) are the terms side by side.  Column c of
// term T (j = c - T.col) has one entry in the column table: the source row, two constants a and b, the noise
// parameters p0 / p1 and the scale.  The value, by T.kind (x = source[row][e]):
//   AS_OBS_GATHER           x - a                      joint_pos / joint_vel (a = 0), joint_pos_rel / joint_vel_rel (a
//                                                      the default), root_*_w, base_pos_z, generated_commands, imu_*
//                                                      (x - 0 is x bit for bit, -0 and NaN included)
//   AS_OBS_LIMIT_NORM       (2 (x - a)) / b            math.py scale_transform: a = (lo + hi) 0.5, b = hi - lo, formed
//                                                      by the host in float32 as torch forms them
//   AS_OBS_QUAT_UNIQUE      w < 0 ? -x : x             math.py quat_unique (w = -0 keeps the sign, as torch.where)
//   AS_OBS_ROTATE_INVERSE   quat_rotate_inverse(root_quat, u)[j]   allsteps_base_frame.h; u the source's three rows,
//                                                      or (0, 0, -1) for projected_gravity
//   AS_OBS_HEIGHT_SCAN      (pose_z - hit_z) - a       observations.py:173, a the offset; a miss (+inf) gives -inf
//   AS_OBS_LAST_ACTION      actions[e][row]            0 for an env the step reset (action_manager.reset); clamped to
//                                                      [-1, 1] where the env's `actions` clamps
// then   noise_term(kind, op, v, draw, p0, p1)         allsteps_noise.h, the nine formulas
//        clip: y = v < lo ? lo : v;  y > hi ? hi : y   torch's clip_: a NaN passes, a zero keeps its sign
//        v * scale                                     scale = 1 where the term has none (exact)
// History of H slots per term, oldest first, newest last, kept in the output row itself: a launch moves slot s + 1
// to slot s (each old value once) and writes the new value into slot H - 1; an env at push count 0 (never pushed
// since its reset) fills all H slots with the new value, as CircularBuffer.append does.  The push count is per env;
// a reset sets it to 0 and clears the row (CircularBuffer.reset).
//
// Draws: Philox4x32-10 keyed by the env's seed, counter (env_id_offset + e, t[e], block, tag) -- the layout of the
// noise, event and command streams with a per-env, per-group counter t[e] of the observation manager's own, advanced
// once per launch of k_observations.  The tag is "ObsM".  Group g owns blocks 64 g .. 64 g + 63; block 64 g + c / 4
// covers the pre-history columns 4 (c / 4) .. + 3.  Uniform draws are the block's four uniforms as they are; normal
// draws are Box-Muller pairs of them (noise_block_draws).  The global env id is in the counter, so shards equal the
// unsharded run.
//
// Plain C++ with no HIP dependency: tests/observations_check.cpp runs all of it on the host.
#pragma once

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/allsteps.h"
#include "allsteps_base_frame.h"
#include "allsteps_noise.h"

namespace as {

constexpr uint32_t kObsTag = 0x4f62734du;  // "ObsM"
constexpr int kObsBlocksPerGroup = AS_MAX_OBS_COLS / 4;
constexpr int kObsMaxCount = 1 << 30;  // the push count saturates here (only 0 / not 0 matters)

// rows of the column table: cols [AS_OBS_COL_ROWS][AS_MAX_OBS_COLS] 32-bit words
enum { kObsColSrcRow = 0, kObsColA = 1, kObsColB = 2, kObsColP0 = 3, kObsColP1 = 4, kObsColScale = 5 };

// the output map's word: pre-history column | last slot << 8 | term width << 9
AS_NZ_FN int32_t obs_omap_pack(int col, bool last, int width) { return col | ((last ? 1 : 0) << 8) | (width << 9); }
AS_NZ_FN int obs_omap_col(int32_t m) { return m & 255; }
AS_NZ_FN bool obs_omap_last(int32_t m) { return ((m >> 8) & 1) != 0; }
AS_NZ_FN int obs_omap_width(int32_t m) { return m >> 9; }

// torch's clip_ (clamp with two scalars): min(max(x, lo), hi) by comparisons that a NaN fails, so it passes, and
// that keep the sign of a zero that equals a bound
AS_NZ_FN float obs_clip(float x, float lo, float hi) {
  const float y = x < lo ? lo : x;
  return y > hi ? hi : y;
}

// The value of column j of term T for one env.  load(source, row): the env's element of a source row (the
// actions: column `row` of the env's action row); a source that is not there reads as 0.
template <typename Load>
AS_NZ_FN float obs_term_value(const as_observation_term_t& T, int j, int row, float a, float b, bool reset,
                              Load&& load) {
  switch (T.kind) {
    case AS_OBS_LIMIT_NORM:
      return (2.0f * (load(T.source, row) - a)) / b;
    case AS_OBS_QUAT_UNIQUE: {
      const float x = load(T.source, row);
      return load(T.source, row - j) < 0.0f ? -x : x;
    }
    case AS_OBS_ROTATE_INVERSE: {
      float q[4], u[3] = {0.0f, 0.0f, -1.0f}, o[3];
      AS_BF_UNROLL
      for (int k = 0; k < 4; ++k) q[k] = load(AS_OBS_SRC_ROOT_QUAT, k);
      if (T.source != AS_OBS_SRC_GRAVITY) {
        AS_BF_UNROLL
        for (int k = 0; k < 3; ++k) u[k] = load(T.source, row - j + k);
      }
      base_rotate_inverse(q, u, o);
      return j == 0 ? o[0] : (j == 1 ? o[1] : o[2]);
    }
    case AS_OBS_HEIGHT_SCAN:
      return (load(AS_OBS_SRC_RAY_POSE, 2) - load(T.source, row)) - a;
    case AS_OBS_LAST_ACTION: {
      if (reset) return 0.0f;
      const float x = load(T.source, row);
      return (T.flags & 1) ? obs_clip(x, -1.0f, 1.0f) : x;
    }
    default:
      return load(T.source, row) - a;
  }
}

// noise -> clip -> scale (observation_manager.py:313-318); x the column's draw (unused without random noise)
AS_NZ_FN float obs_post(const as_observation_term_t& T, float v, float x, float p0, float p1, float scale) {
  if (T.noise_kind != AS_NOISE_NONE) v = noise_term(T.noise_kind, T.noise_op, v, x, p0, p1);
  if (T.clip) v = obs_clip(v, T.clip_lo, T.clip_hi);
  return v * scale;
}

// the draw of pre-history column c of group g: word c % 4 of block 64 g + c / 4, as the term's noise takes it
AS_NZ_FN float obs_draw(int noise_kind, uint64_t seed, uint32_t env, uint32_t t, int group, int c) {
  if (!noise_kind_random(noise_kind)) return 0.0f;
  float u4[4], x4[4];
  noise_philox_block(seed, env, t, (uint32_t)(group * kObsBlocksPerGroup + (c >> 2)), kObsTag, u4);
  const int w = c & 3;
  if (noise_kind == AS_NOISE_GAUSSIAN) {
    // one Box-Muller pair: words (0, 1) or (2, 3)
    const bool hi = w >= 2;
    noise_box_muller(hi ? u4[2] : u4[0], hi ? u4[3] : u4[1], &x4[0], &x4[1]);
    return (w & 1) ? x4[1] : x4[0];
  }
  return w == 0 ? u4[0] : (w == 1 ? u4[1] : (w == 2 ? u4[2] : u4[3]));
}

// the history rule: output column oc takes the new value (the last slot, or an env never pushed since its reset),
// otherwise the old value one slot on, `width` columns to the right
AS_NZ_FN bool obs_takes_new(int32_t omap_word, int count) { return obs_omap_last(omap_word) || count == 0; }

// One env's launch of one group on host arrays -- what k_observations does per env, in the same pieces.
// cols: the column table; omap [out_cols]; row: the env's output row (in place); draws: d0 draws or null (Philox).
// Returns the new push count.
template <typename Load>
inline int obs_group_env_step(const as_observation_term_t* terms, int num_terms, const uint32_t* cols,
                              const int32_t* omap, int d0, int out_cols, int group, bool reset, int count,
                              float* row, const float* draws, uint64_t seed, uint32_t env, uint32_t t,
                              float* fresh /* [d0] scratch */, Load&& load) {
  auto colf = [&](int r, int c) {
    union { uint32_t u; float f; } w;
    w.u = cols[(size_t)r * AS_MAX_OBS_COLS + c];
    return w.f;
  };
  if (reset) count = 0;
  for (int k = 0; k < num_terms; ++k) {
    const as_observation_term_t& T = terms[k];
    for (int j = 0; j < T.width; ++j) {
      const int c = T.col + j;
      const float v = obs_term_value(T, j, (int32_t)cols[(size_t)kObsColSrcRow * AS_MAX_OBS_COLS + c],
                                     colf(kObsColA, c), colf(kObsColB, c), reset, load);
      const float x = noise_kind_random(T.noise_kind)
                          ? (draws ? draws[c] : obs_draw(T.noise_kind, seed, env, t, group, c))
                          : 0.0f;
      fresh[c] = obs_post(T, v, x, colf(kObsColP0, c), colf(kObsColP1, c), colf(kObsColScale, c));
    }
  }
  (void)d0;
  // ascending columns: column oc reads oc + width, which is still the old value
  for (int oc = 0; oc < out_cols; ++oc) {
    const int32_t m = omap[oc];
    row[oc] = obs_takes_new(m, count) ? fresh[obs_omap_col(m)] : row[oc + obs_omap_width(m)];
  }
  return count < kObsMaxCount ? count + 1 : count;
}

}  // namespace as
