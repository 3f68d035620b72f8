// contact_timer_kernels.h -- k_contact_timers, the air / contact timers of cfg.contact_air_time
// (as_contact_timers).  Semantics, formulas and buffer layout: allsteps_contact_timers.h.  The kernel is not part
// of as_step: the env launches it after as_step when its cfg asks for the timers, so the default step keeps its
// launches.  Reads the contact report (allsteps_contact_report.h); writes the timers and the timestamp only.  No
// host sync, no atomics, no LDS.
#pragma once

#include <hip/hip_runtime.h>

#include "allsteps_contact_timers.h"
#include "allsteps_kernels.h"

namespace as {

// A workgroup is kTimerEnvs envs x kTimerGroup body lanes: threadIdx.x is the env, so envs run along the lanes
// of a wave, and threadIdx.y -- one wave each -- the body lane.  The report, the timers [4][bodies][n], the
// timestamp [n] and the reset masks [n] are all env-minor, so a wave's access to a row is one contiguous run.
// Wave j serves the bodies j, j + kTimerGroup, ...: the sensor feet are two or four bodies, one per wave, and a
// longer table loops in the wave.  A body's link is wave-uniform (a scalar) and its four timers are registers:
// nothing is indexed dynamically; the timers are read once, carried across the `updates` sensor updates (slot
// updates - 1, the oldest substep, down to slot 0) and written once.  A thread gathers its env's records of a
// slot once per body (report_load_env; the body waves of an env re-read the same lines, L2 hits) and forms the
// body's net impulse from them (report_body_sum, the sum net_forces_w shows): ten records of selects and adds,
// three IEEE divisions and a square root per update, which is why the bodies go side by side on the workgroup's
// four SIMDs and not one after the other in a thread (measured at 4096 envs: 10.9 us a launch in sequence).
// The timestamp: every wave replays the sequence ts += dt from the value it read, wave 0 alone writes it, and the
// barrier between the reads and that write keeps the env's other waves -- all in this workgroup -- from seeing
// the new value: one writer, no hazard between workgroups or launches.
constexpr int kTimerEnvs = 64;
constexpr int kTimerGroup = 4;

__global__ __launch_bounds__(kTimerEnvs * kTimerGroup) void k_contact_timers(TimersArgs P) {
  const int64_t e64 = (int64_t)blockIdx.x * kTimerEnvs + threadIdx.x;
  const bool valid = e64 < P.n;  // (no early return: every thread meets the barrier)
  const int n = P.n, nb = P.num_bodies;
  const int e = valid ? (int)e64 : n - 1;  // a tail lane re-reads the last env: in bounds, never stored
  const float ts0 = P.timestamp[e];
  // the envs reset after the updates: reset | reset2; no mask: every env of a reset-only launch, none otherwise
  bool rst = P.updates == 0;
  if (P.reset) rst = (P.reset[e] | (P.reset2 ? P.reset2[e] : (uint8_t)0)) != 0;
  asm volatile("" ::"v"(ts0));  // the timestamp is in its register -- the load has returned -- ahead of the barrier
  __syncthreads();
  float ts = ts0;
  for (int b = (int)threadIdx.y; b < nb; b += kTimerGroup) {
    const int link = P.link[b];
    ContactTimers t;
    t.current_air = P.timers[timers_index(kTimerCurrentAir, b, e, n, nb)];
    t.last_air = P.timers[timers_index(kTimerLastAir, b, e, n, nb)];
    t.current_contact = P.timers[timers_index(kTimerCurrentContact, b, e, n, nb)];
    t.last_contact = P.timers[timers_index(kTimerLastContact, b, e, n, nb)];
    ts = ts0;
    for (int slot = P.updates - 1; slot >= 0; --slot) {
      // (on an opaque copy of n: the 41 row offsets of a slot are formed where they are used, in scalar
      // registers that are free again after the load, not hoisted out of the loops and held -- spilled)
      int ns = n;
      asm volatile("" : "+s"(ns));
      ReportEnv r;
      report_load_env(P.count, P.records, slot, e, ns, r);
      const float elapsed = timers_tick(&ts, P.dt);
      float imp[3];
      report_body_sum(r, link, imp);
      timers_update_impulse(t, imp, P.dt, P.force_threshold, elapsed);
    }
    if (rst) timers_reset(t);
    if (valid) {
      P.timers[timers_index(kTimerCurrentAir, b, e, n, nb)] = t.current_air;
      P.timers[timers_index(kTimerLastAir, b, e, n, nb)] = t.last_air;
      P.timers[timers_index(kTimerCurrentContact, b, e, n, nb)] = t.current_contact;
      P.timers[timers_index(kTimerLastContact, b, e, n, nb)] = t.last_contact;
    }
  }
  // wave 0 always has body 0, so its ts is the sequence's end
  if (threadIdx.y == 0 && valid) P.timestamp[e] = rst ? 0.f : ts;
}

}  // namespace as
