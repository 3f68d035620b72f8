// contact_forces_kernel.h -- k_contact_forces, the dense contact-force views (as_contact_forces), off the hot
// path.  Reads the contact report (allsteps_contact_report.h); writes only its two outputs, every entry of
// them (zero-filled).
#pragma once

#include <hip/hip_runtime.h>

#include "allsteps_contact_report.h"
#include "allsteps_kernels.h"

namespace as {

// One thread per (env, substep slot), envs along the lanes: every read and write is env-minor, so a wave's
// accesses are contiguous.  The thread gathers its env's records once (at most kRepMaxC, four words each)
// and forms every output entry as its own ascending sum over them (report_pair_sum / report_body_sum): no
// atomics, no order that depends on the launch.
constexpr int kForcesThreads = 64;

__global__ __launch_bounds__(kForcesThreads) void k_contact_forces(ForcesArgs P) {
  const int n = P.n;
  const int e = blockIdx.x * kForcesThreads + threadIdx.x;
  const int slot = blockIdx.y;
  if (e >= n || slot >= P.depth) return;
  ReportEnv r;
  report_load_env(P.count, P.records, slot, e, n, r);
  for (int f = 0; f < kRepFeet; ++f)
    for (int st = 0; st < AS_NUM_STONES; ++st) {
      float v[3];
      report_pair_sum(r, f, st, v);
#pragma unroll
      for (int k = 0; k < 3; ++k) P.matrix[report_matrix_index(slot, f, st, k, e, n)] = v[k];
    }
  const int nb = P.num_bodies;
  for (int b = 0; b < nb; ++b) {
    float v[3];
    report_body_sum(r, P.link[b], v);
#pragma unroll
    for (int k = 0; k < 3; ++k) P.net[report_net_index(slot, b, k, e, n, nb)] = v[k];
  }
}

}  // namespace as
