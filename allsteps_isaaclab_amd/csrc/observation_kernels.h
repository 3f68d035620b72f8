// observation_kernels.h -- k_observations / k_observations_reset, the opt-in observation manager of
// cfg.observations (as_observations_step / as_observations_reset).  Semantics, formulas, history rule, draw layout
// and stream: allsteps_observations.h.  Neither kernel is part of as_step: the env launches k_observations last in
// its step, once per group, when its cfg names observations, so the default step keeps its launches.  No host sync,
// no atomics, no scratch.
#pragma once

#include <hip/hip_runtime.h>

#include "allsteps_kernels.h"
#include "allsteps_observations.h"

namespace as {

// The state is field-major ([rows][n], envs contiguous) and the output row-major ([n][out_cols], columns
// contiguous), so a block turns a tile: it takes kObsTile consecutive envs -- 16, so that 4096 envs make 256 blocks,
// one for every compute unit, and a block's serial walk over its (column, env) items is half as long as with 32
// (measured: DESIGN.md §3 "Observation manager").
//   Phase A, lanes along the envs: for each term in cfg order, every (column, env) item loads its source rows -- a
//   wave reads four runs of 16 consecutive envs (64 bytes each) -- and computes value, noise, clip and scale into
//   the LDS tile [column][env] (pitch kObsTile + 1, odd: the transposed reads of phase B spread over the banks).
//   The actions, the one row-major source, are walked along their columns instead.
//   Phase B, lanes along the output columns: wave w takes the tile's rows w, w + 4, ...; each lane holds the
//   columns lane, lane + 64, ... of the row in registers -- the new value from the tile, or, for a history slot
//   that is not the last, the old value one slot on from the output row itself (a contiguous run, shifted by the
//   term's width) -- and after a barrier stores them: whole rows, coalesced.  Every old value moves once.  The
//   barrier separates a row's loads from its stores: within a row they overlap, between rows they do not.
// The term descriptors, the column table and the output map are read from device memory, so a descriptor rewritten
// by set_term_cfg takes effect in a graph that is already captured.
constexpr int kObsThreads = 256;
constexpr int kObsTile = 16;
constexpr int kObsPitch = kObsTile + 1;
constexpr int kObsWaves = kObsThreads / 64;
constexpr int kObsChunks = AS_MAX_OBS_OUT_COLS / 64;  // register columns per lane in phase B
static_assert(AS_MAX_OBS_OUT_COLS % 64 == 0 && kObsTile % kObsWaves == 0 && AS_MAX_OBS_COLS <= 256, "tile shape");

__global__ __launch_bounds__(kObsThreads) void k_observations(ObservationsArgs P) {
  __shared__ float tile[AS_MAX_OBS_COLS * kObsPitch];
  __shared__ int s_count[kObsTile];
  __shared__ uint32_t s_t[kObsTile];
  __shared__ uint8_t s_reset[kObsTile];
  const int tid = threadIdx.x;
  const int64_t e0 = (int64_t)blockIdx.x * kObsTile;
  const size_t n = (size_t)P.n;
  if (tid < kObsTile) {
    const int64_t e = e0 + tid;
    bool reset = false;
    int count = 0;
    uint32_t t = 0u;
    if (e < P.n) {
      reset = (P.reset && P.reset[e]) || (P.reset2 && P.reset2[e]);
      count = reset ? 0 : P.count[e];
      t = P.t[e];
    }
    s_reset[tid] = reset ? 1 : 0;
    s_count[tid] = count;
    s_t[tid] = t;
  }
  __syncthreads();

  const uint32_t* colw = reinterpret_cast<const uint32_t*>(P.cols);
  for (int k = 0; k < P.num_terms; ++k) {
    const as_observation_term_t T = P.terms[k];
    const bool row_major = T.kind == AS_OBS_LAST_ACTION;
    const int items = T.width * kObsTile;
    for (int item = tid; item < items; item += kObsThreads) {
      int el, j;
      if (row_major) {
        el = item / T.width;
        j = item - el * T.width;
      } else {
        j = item / kObsTile;
        el = item - j * kObsTile;
      }
      const int64_t e = e0 + el;
      const int c = T.col + j;
      if (e >= P.n || c < 0 || c >= P.d0) continue;  // (d0 <= AS_MAX_OBS_COLS: tile, table and draws hold c)
      auto load = [&](int source, int row) __attribute__((always_inline)) -> float {
        const float* p = P.src.ptr[source];
        if (!p || row < 0 || row >= P.src.rows[source]) return 0.0f;
        return source == AS_OBS_SRC_ACTIONS ? p[(size_t)e * (size_t)P.src.rows[source] + (size_t)row]
                                            : p[(size_t)row * n + (size_t)e];
      };
      const float v = obs_term_value(T, j, (int32_t)colw[kObsColSrcRow * AS_MAX_OBS_COLS + c],
                                     P.cols[kObsColA * AS_MAX_OBS_COLS + c], P.cols[kObsColB * AS_MAX_OBS_COLS + c],
                                     s_reset[el] != 0, load);
      float x = 0.0f;
      if (noise_kind_random(T.noise_kind))
        x = P.draws ? P.draws[(size_t)c * n + (size_t)e]
                    : obs_draw(T.noise_kind, P.seed, (uint32_t)(P.env_offset + e), s_t[el], P.group, c);
      tile[c * kObsPitch + el] = obs_post(T, v, x, P.cols[kObsColP0 * AS_MAX_OBS_COLS + c],
                                          P.cols[kObsColP1 * AS_MAX_OBS_COLS + c],
                                          P.cols[kObsColScale * AS_MAX_OBS_COLS + c]);
    }
  }
  __syncthreads();

  const int lane = tid & 63, wave = tid >> 6;
  for (int r = 0; r < kObsTile / kObsWaves; ++r) {
    const int el = r * kObsWaves + wave;
    const int64_t e = e0 + el;
    const bool valid = e < P.n;
    float* row = P.out + (size_t)(valid ? e : 0) * (size_t)P.out_cols;
    const int count = s_count[el];
    float v[kObsChunks];
#pragma unroll
    for (int k = 0; k < kObsChunks; ++k) {
      const int oc = lane + 64 * k;
      v[k] = 0.0f;
      if (valid && oc < P.out_cols) {
        const int32_t m = P.omap[oc];
        const int src = oc + obs_omap_width(m);
        v[k] = (obs_takes_new(m, count) || src >= P.out_cols) ? tile[obs_omap_col(m) * kObsPitch + el] : row[src];
      }
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kObsChunks; ++k) {
      const int oc = lane + 64 * k;
      if (valid && oc < P.out_cols) row[oc] = v[k];
    }
  }
  if (tid < kObsTile && e0 + tid < P.n) {
    const int count = s_count[tid];
    P.count[e0 + tid] = count < kObsMaxCount ? count + 1 : count;
    P.t[e0 + tid] = s_t[tid] + 1u;
  }
}

// ObservationManager.reset(env_ids): wave w clears the rows w, w + 4, ... of the tile's masked envs
__global__ __launch_bounds__(kObsThreads) void k_observations_reset(ObservationsArgs P) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for (int r = 0; r < kObsTile / kObsWaves; ++r) {
    const int64_t e = (int64_t)blockIdx.x * kObsTile + r * kObsWaves + wave;
    if (e >= P.n || (P.reset && !P.reset[e])) continue;
    float* row = P.out + (size_t)e * (size_t)P.out_cols;
    for (int oc = lane; oc < P.out_cols; oc += 64) row[oc] = 0.0f;
    if (lane == 0) P.count[e] = 0;
  }
}

}  // namespace as
