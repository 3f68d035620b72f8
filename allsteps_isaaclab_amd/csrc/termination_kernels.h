// termination_kernels.h -- k_terminations_step, the opt-in termination manager of cfg.terminations
// (as_terminations_step).  Semantics, formulas and the float32 operations: allsteps_terminations.h.  The kernel is not
// part of as_step: the env launches it directly after the step (and after as_contact_forces where a term reads the net
// forces) when its cfg names terminations, so the default step keeps its launches.  No host sync, no atomics, no
// scratch.
#pragma once

#include <hip/hip_runtime.h>

#include "allsteps_kernels.h"
#include "allsteps_terminations.h"

namespace as {

// Every source is field-major ([rows][n], envs contiguous), so lanes run along the envs and every load is one
// contiguous run of 64 envs.  A block takes kTermEnvs = 64 consecutive envs with kTermWaves = 4 waves (measured against
// 1, 2, 8 and 16: DESIGN.md §3 "Termination manager"); wave w takes the terms w, w + kTermWaves, ... one at a time, so
// the descriptor, the kind switch and the term's row of the index table are the same in every lane of a wave (the wave
// index goes through readfirstlane, which lets the compiler keep them in scalar registers and load them with scalar
// loads): no divergence across kinds.  The lane that made a term's flag stores it to term_dones[k][env] and leaves it
// in LDS [term][env]; after one barrier every wave forms its env's cfg-order ORs from LDS (at most 16 byte reads):
// wave 0 stores time_outs, terminated, dones and reset_request, and wave w copies the flags of its own terms to
// last_episode_dones for an env that is done -- by the manager or by the step's own flags.  The term descriptors and
// the index table are read from device memory, so a descriptor rewritten by set_term_cfg takes effect in a graph that
// is already captured.
// (AS_TERM_WAVES: the waves per block of a variant build, for measurements; DESIGN.md §3 "Termination manager")
#ifndef AS_TERM_WAVES
#define AS_TERM_WAVES 4
#endif
constexpr int kTermEnvs = 64;
constexpr int kTermWaves = AS_TERM_WAVES;
constexpr int kTermThreads = 64 * kTermWaves;

__global__ __launch_bounds__(kTermThreads) void k_terminations_step(TerminationsArgs P) {
  __shared__ uint8_t s_flag[AS_MAX_TERMINATION_TERMS * kTermEnvs];
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int64_t e = (int64_t)blockIdx.x * kTermEnvs + lane;
  const bool valid = e < P.n;
  const size_t n = (size_t)P.n, i = (size_t)(valid ? e : 0);
  const int T = P.num_terms < AS_MAX_TERMINATION_TERMS ? P.num_terms : AS_MAX_TERMINATION_TERMS;
  const TerminationEnv E{&P.src, n, i};
  const uint32_t* tab = reinterpret_cast<const uint32_t*>(P.table);
  for (int k = wave; k < T; k += kTermWaves) {
    const as_termination_term_t term = P.terms[k];
    uint8_t flag = 0;
    if (valid) {
      flag = termination_term_flag(term, reinterpret_cast<const int32_t*>(tab + term_table_at(kTermTabId, k, 0)),
                                   P.table + term_table_at(kTermTabA, k, 0), P.table + term_table_at(kTermTabB, k, 0),
                                   E)
                 ? 1
                 : 0;
      P.term_dones[(size_t)k * n + i] = flag;
    }
    s_flag[k * kTermEnvs + lane] = flag;
  }
  __syncthreads();
  if (!valid) return;
  bool to, te;
  terminations_union(P.terms, T, s_flag + lane, kTermEnvs, &to, &te);
  const bool stepped = E.step_terminated() || E.step_truncated();
  if (wave == 0) {
    P.time_outs[i] = to ? 1 : 0;
    P.terminated[i] = te ? 1 : 0;
    P.dones[i] = (to || te) ? 1 : 0;
    if (P.reset_request) P.reset_request[i] = ((to || te) && !stepped) ? 1 : 0;
  }
  if (P.last_episode_dones && (to || te || stepped))
    for (int k = wave; k < T; k += kTermWaves) P.last_episode_dones[(size_t)k * n + i] = s_flag[k * kTermEnvs + lane];
}

}  // namespace as
