// allsteps_contact_timers.h -- the air / contact timers of the foot contact sensors (cfg.contact_air_time).
//
// The reference's ContactSensor with track_air_time = True keeps four timers per body (contact_sensor.py:351-379)
// and a float32 timestamp per env (SensorBase.update, sensor_base.py:199).  One sensor update of one (env, body),
// every operation in float32 and rounded on its own (the library is built with -ffp-contract=off):
//     ts_new  = ts + dt                     SensorBase.update: a float32 tensor += the physics step
//     elapsed = ts_new - ts                 contact_sensor.py:355: the DIFFERENCE of the two timestamps, not dt --
//                                           it drifts by ulps as ts grows, and the timers sum it
//     f_k     = imp_k / dt                  k = x y z: get_net_contact_forces(dt), the body's net contact impulse
//                                           (report_body_sum, allsteps_contact_report.h) over float32(sim.dt)
//     contact = sqrtf((fx fx + fy fy) + fz fz) > force_threshold            (:357)
//     first_contact  = current_air > 0     && contact                      (:358)
//     first_detached = current_contact > 0 && !contact                     (:359)
//     last_air        = first_contact  ? current_air + elapsed     : last_air          (:361-365)
//     current_air     = !contact       ? current_air + elapsed     : 0                 (:367-369)
//     last_contact    = first_detached ? current_contact + elapsed : last_contact      (:371-375)
//     current_contact = contact        ? current_contact + elapsed : 0                 (:377-379)
// in this order: each line reads what the lines above it left.  reset(env) zeroes the four timers of every body
// and the timestamp (contact_sensor.py:156-161, sensor_base.py:192-193).
//
// The reference's sensors update once per physics step (update_period = 0 with history_length = 4:
// allsteps_env_cfg.py:119-130, sensor_base.py:204), so an env step is `decimation` updates, oldest substep first
// -- report slot depth - 1 down to slot 0 -- and the reset of the envs the step reset comes after them
// (direct_rl_env.py:347, then :361 / :569).
//
// Buffers, field-major / env-minor like the report:
//   timers    [kTimerRows][num_bodies][n]   rows current_air, last_air, current_contact, last_contact
//   timestamp [n]
//
// Plain C++ with no HIP dependency: tests/contact_timers_check.cpp runs all of it on the host.
#pragma once

#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "allsteps_contact_report.h"

namespace as {

enum { kTimerCurrentAir = 0, kTimerLastAir, kTimerCurrentContact, kTimerLastContact, kTimerRows };

AS_CR_FN size_t timers_index(int row, int body, int e, int n, int num_bodies) {
  return ((size_t)row * (size_t)num_bodies + (size_t)body) * (size_t)n + (size_t)e;
}

// The four timers of one (env, body), held by value.
struct ContactTimers {
  float current_air, last_air, current_contact, last_contact;
};

// SensorBase.update on the env's timestamp: returns the elapsed time the timers add
AS_CR_FN float timers_tick(float* ts, float dt) {
  const float t0 = *ts;
  const float t1 = t0 + dt;
  *ts = t1;
  return t1 - t0;
}

// get_net_contact_forces(dt): the net impulse over the physics step, an IEEE division per component
AS_CR_FN void timers_force(const float (&imp)[3], float dt, float (&f)[3]) {
  for (int k = 0; k < 3; ++k) f[k] = imp[k] / dt;
}

// |f| > force_threshold
AS_CR_FN bool timers_in_contact(const float (&f)[3], float force_threshold) {
  return sqrtf((f[0] * f[0] + f[1] * f[1]) + f[2] * f[2]) > force_threshold;
}

// The four lines of the update, in the reference's order, on a contact state already decided
AS_CR_FN void timers_update(ContactTimers& t, bool contact, float elapsed) {
  const bool first_contact = t.current_air > 0.f && contact;
  const bool first_detached = t.current_contact > 0.f && !contact;
  t.last_air = first_contact ? t.current_air + elapsed : t.last_air;
  t.current_air = !contact ? t.current_air + elapsed : 0.f;
  t.last_contact = first_detached ? t.current_contact + elapsed : t.last_contact;
  t.current_contact = contact ? t.current_contact + elapsed : 0.f;
}

// One sensor update of one body from its net impulse of the physics step
AS_CR_FN void timers_update_impulse(ContactTimers& t, const float (&imp)[3], float dt, float force_threshold,
                                    float elapsed) {
  float f[3];
  timers_force(imp, dt, f);
  timers_update(t, timers_in_contact(f, force_threshold), elapsed);
}

AS_CR_FN void timers_reset(ContactTimers& t) { t.current_air = t.last_air = t.current_contact = t.last_contact = 0.f; }

}  // namespace as
