// allsteps_contact_report.h -- layout of the opt-in contact report and the per-env reductions over it.
//
// With a report set (as_set_contact_report) k_step stores, for each of the last `depth` substeps of a launch
// with physics, the contacts the solver kept: per env a count and AS_MAX_CONTACTS records of kRepWords
// 32-bit words (step_report.h); k_contact_forces (contact_forces_kernel.h) sums them into the dense force
// matrix and per-body net impulses.  Everything is field-major / env-minor and indexed by env id:
//   count   [depth][n]                                  int32, kept contacts of the substep
//   records [depth][kRepWords][AS_MAX_CONTACTS][n]      words kRepIx.. below; slots >= count hold zeros
//   qd_prev [AS_ACT_DIM][n]                             joint velocity (cfg dof order) at the start of the
//                                                       launch's last substep
// substep slot 0 is the launch's last substep, slot k the k-th before it.
//   force matrix out [depth][AS_REPORT_FEET][AS_NUM_STONES][3][n]   impulse (N s) of the stone on the foot
//   net out          [depth][num_bodies][3][n]                      net contact impulse on each body
//
// Plain C++ with no HIP dependency: tests/contact_report_check.cpp runs the reductions on the host.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "../../include/allsteps.h"

#if defined(__HIPCC__) || defined(__CUDACC__)
#define AS_CR_FN __host__ __device__ __forceinline__
#else
#define AS_CR_FN inline
#endif

namespace as {

constexpr int kRepMaxC = AS_MAX_CONTACTS;
constexpr int kRepWords = AS_REPORT_WORDS;
constexpr int kRepFeet = AS_REPORT_FEET;
// record words: lambda_n n (the floats the contact flags sum: EnvS::x.cf), contact point, separation, ids
enum { kRepIx = 0, kRepIy, kRepIz, kRepPx, kRepPy, kRepPz, kRepSep, kRepIds };
static_assert(kRepIds + 1 == kRepWords, "record words");

// ids word: link | (link2 + 1) << 8 | (stone + 1) << 16 | (foot + 1) << 24  (link2 / stone / foot: -1 = none;
// links < AS_MAX_LINKS, stones < AS_NUM_STONES, feet < kRepFeet: a byte each)
AS_CR_FN uint32_t report_pack_ids(int link, int link2, int stone, int foot) {
  return (uint32_t)(link & 0xff) | (uint32_t)((link2 + 1) & 0xff) << 8 | (uint32_t)((stone + 1) & 0xff) << 16 |
         (uint32_t)((foot + 1) & 0xff) << 24;
}
AS_CR_FN void report_unpack_ids(uint32_t w, int& link, int& link2, int& stone, int& foot) {
  link = (int)(w & 0xffu);
  link2 = (int)(w >> 8 & 0xffu) - 1;
  stone = (int)(w >> 16 & 0xffu) - 1;
  foot = (int)(w >> 24) - 1;
}
// the (foot, stone) half of an ids word: what a force-matrix entry matches
AS_CR_FN uint32_t report_pair_key(int foot, int stone) { return report_pack_ids(0, -1, stone, foot) & 0xffff0000u; }

AS_CR_FN size_t report_count_index(int slot, int e, int n) { return (size_t)slot * (size_t)n + (size_t)e; }
AS_CR_FN size_t report_record_index(int slot, int word, int c, int e, int n) {
  return (((size_t)slot * kRepWords + (size_t)word) * kRepMaxC + (size_t)c) * (size_t)n + (size_t)e;
}
AS_CR_FN size_t report_count_words(int depth, int n) { return (size_t)depth * (size_t)n; }
AS_CR_FN size_t report_record_words(int depth, int n) { return (size_t)depth * kRepWords * kRepMaxC * (size_t)n; }
AS_CR_FN size_t report_matrix_index(int slot, int foot, int stone, int k, int e, int n) {
  return ((((size_t)slot * kRepFeet + (size_t)foot) * AS_NUM_STONES + (size_t)stone) * 3 + (size_t)k) * (size_t)n +
         (size_t)e;
}
AS_CR_FN size_t report_net_index(int slot, int body, int k, int e, int n, int num_bodies) {
  return (((size_t)slot * (size_t)num_bodies + (size_t)body) * 3 + (size_t)k) * (size_t)n + (size_t)e;
}

AS_CR_FN float report_word_float(uint32_t w) {
  union { uint32_t u; float f; } c;
  c.u = w;
  return c.f;
}

// One env's records of one substep slot, held by value (k_contact_forces: registers): the three impulse
// words and the ids word of every slot; slots >= count are not read.
struct ReportEnv {
  int count;
  float imp[kRepMaxC][3];
  uint32_t ids[kRepMaxC];
};

// Gather an env's slot from the report buffers (count clamped to [0, kRepMaxC]: a buffer the caller never
// had written cannot index past the records).
AS_CR_FN void report_load_env(const int32_t* count, const uint32_t* records, int slot, int e, int n, ReportEnv& r) {
  const int c0 = count[report_count_index(slot, e, n)];
  r.count = c0 < 0 ? 0 : (c0 > kRepMaxC ? kRepMaxC : c0);
  for (int c = 0; c < kRepMaxC; ++c) {
    for (int k = 0; k < 3; ++k) r.imp[c][k] = report_word_float(records[report_record_index(slot, kRepIx + k, c, e, n)]);
    r.ids[c] = records[report_record_index(slot, kRepIds, c, e, n)];
  }
}

// Force-matrix entry (foot, stone): the records with that pair, ascending, from +0 with plain adds -- the
// sum contact_flag (step_solve.h) tests against the sensor threshold.
AS_CR_FN void report_pair_sum(const ReportEnv& r, int foot, int stone, float (&f)[3]) {
  const uint32_t key = report_pair_key(foot, stone);
  f[0] = f[1] = f[2] = 0.f;
  for (int c = 0; c < kRepMaxC; ++c) {
    const bool same = c < r.count && (r.ids[c] & 0xffff0000u) == key;
    for (int k = 0; k < 3; ++k) f[k] += same ? r.imp[c][k] : 0.f;
  }
}

// Net contact impulse on the body carried by `link`: + a record's impulse where it is the record's link,
// - where it is the record's second link (a self-contact pushes its two links apart), ascending.
AS_CR_FN void report_body_sum(const ReportEnv& r, int link, float (&f)[3]) {
  f[0] = f[1] = f[2] = 0.f;
  for (int c = 0; c < kRepMaxC; ++c) {
    const bool live = c < r.count;
    const bool on1 = live && (int)(r.ids[c] & 0xffu) == link;
    const bool on2 = live && (int)(r.ids[c] >> 8 & 0xffu) - 1 == link;
    for (int k = 0; k < 3; ++k) {
      f[k] += on1 ? r.imp[c][k] : 0.f;
      f[k] -= on2 ? r.imp[c][k] : 0.f;
    }
  }
}

}  // namespace as
