// step_report.h -- k_step's stores into the opt-in contact report (allsteps_contact_report.h).
// Reads x.cf (the impulse products and pair keys the PGS left for the flags), cpt, csep, clink, clink2, cstone,
// cfoot and u; writes global memory only.  Both calls sit in k_step's substep loop behind the wave-uniform
// test of StepArgs::rep, outside substep(): after a substep's last barrier every register of the solve
// is dead, x.cf and the contact list are still as the PGS left them (the next substep's FK is the first to
// write the phase union again), and no vector global load is needed -- the ids come from LDS, the dof map
// of the velocities from uniform (scalar) loads.
#pragma once

#include <hip/hip_runtime.h>

#include "allsteps_contact_report.h"
#include "allsteps_kernels.h"
#include "step_scratch.h"

namespace as {

// The joint velocities at the start of the launch's last substep, cfg dof order (lane = cfg dof).
__device__ __forceinline__ void report_store_qd(const ReportDesc* rp, int n, CK* Kc0, const EnvS& s, int lane0, int e0,
                                                bool valid) {
  // opaque copies, as in substep(): nothing derived from them (addresses, lane masks, the descriptor's words) is
  // hoisted out of the substep loop and held in registers across the substeps -- hoisted, they cost k_step<27>
  // 9 VGPRs and 28 SGPR spills
  int lane = lane0, e = e0;
  typedef const __attribute__((address_space(4))) ReportDesc* DescP;
  DescP dp = (DescP)rp;
  CK* Kc = Kc0;
  asm volatile("" : "+v"(lane), "+v"(e), "+s"(dp), "+s"(Kc));
  const int nh = Kc->model.num_hinges;
  int li = 1;
#pragma unroll 1
  for (int k = 0; k < nh; ++k) {
    const int lk = Kc->model.cfg_dof_link[k];  // uniform index: a scalar load
    li = lane == k ? lk : li;
  }
  if (valid && lane < nh) dp->qd_prev[(size_t)lane * (size_t)n + (size_t)e] = s.u[6 + li - 1];
}

// One substep's kept contacts into substep slot `slot` (nothing for slot >= depth): lane c < MAXC writes
// record c -- zeros past the env's count -- and lane 0 the count.  A kept contact is one whose x.cf key is not
// the "no contact" key -1 (step_solve.h: lanes >= nce).
__device__ __forceinline__ void report_store(const ReportDesc* rp, int n, EnvS& s, int lane0, int e0, bool valid,
                                             int slot) {
  int lane = lane0, e = e0;  // opaque copies (see report_store_qd)
  typedef const __attribute__((address_space(4))) ReportDesc* DescP;
  DescP dp = (DescP)rp;
  asm volatile("" : "+v"(lane), "+v"(e), "+s"(dp));
  const __attribute__((address_space(4))) ReportDesc& D = *dp;
  if (slot >= D.depth) return;  // uniform
  const int el = (int)(threadIdx.x >> 5) + (lane & 0);  // (tied to the opaque lane: formed here, not ahead of the loop)
  const int c = lane < MAXC ? lane : 0;
  const v4f cf = *reinterpret_cast<const v4f*>(s.x.cf[c]);
  const bool kept = lane < MAXC && __float_as_int(cf.w) != -1;
  const uint64_t bl = __ballot(kept);
  const int cnt = __popcll(bl >> (32 * el) & 0xffffffffull);
  if (valid && lane < MAXC) {
    const uint32_t w[kRepWords] = {
        __float_as_uint(cf.x), __float_as_uint(cf.y), __float_as_uint(cf.z), __float_as_uint(s.cpt[c][0]),
        __float_as_uint(s.cpt[c][1]), __float_as_uint(s.cpt[c][2]), __float_as_uint(s.csep[c]),
        report_pack_ids(s.clink[c], s.clink2[c], s.cstone[c], s.cfoot[c])};
    // one lane pointer stepped by the word stride, opaque between the stores, so that the eight addresses are
    // formed one after the other (scalar registers are the scarce ones here: tests/kernel_budget.json)
    uint32_t* p = D.records + report_record_index(slot, 0, c, e, n);
    static_assert(kRepIx == 0, "first word");
    const size_t stride = report_record_index(0, 1, 0, 0, n);
#pragma unroll
    for (int k = 0; k < kRepWords; ++k) {
      *p = kept ? w[k] : 0u;
      p += stride;
      asm volatile("" : "+v"(p));
    }
  }
  if (valid && lane == 0) D.count[report_count_index(slot, e, n)] = cnt;
  __syncthreads();  // the reads above, before the next substep's FK rewrites the phase union
}

}  // namespace as
