// commands_check.cpp -- stand-alone host check of csrc/allsteps_commands.h (tests/test_commands_host.py builds and
// runs it, plain and under -fsanitize=address,undefined).
//
//   commands_check <cases.bin> [<dump.bin>]
//
// cases.bin (written by the test from tests/golden/commands.npz, native endianness, 4-byte words):
//   int32 nphilox, then per query: uint32 seed_lo, seed_hi, env, t, b, tag; float expect[4]
//     (the oracle's or_philox_block for the two command tags) -- noise_philox_block must give the same bits;
//   int32 ncases, then per case
//     int32 n, terms, steps, has_init;  float dt
//     float rows[terms][21] (as_command_term_t)
//     the state the case starts from: float vel[terms][3][n], heading[terms][n]; int32 flags[terms][5][n];
//       float time_left[terms][n]; int32 counter[terms][n]; float metrics[terms][2][n]
//     float init_draws[terms][11][n] -- has_init: a reset of every env from the zero state must give that state
//     per step: float root_quat[4][n], root_lin[3][n], root_ang[3][n]; int32 reset[n];
//               float draws[2][terms][11][n]; then the reference's state after the step in the layout above,
//               float last_metrics[terms][2][n] and int32 resampled[2][terms][n]
// The program replays a case the way k_commands_step does (terms in order, one env at a time) with the header's
// functions.  Everything that is not downstream of atan2 must equal the reference bit for bit: timers, counters,
// masks, heading targets, the sampled commands, the standing and zero masks' zeroing, error_vel_xy, the snapshot
// rows, which envs resample in which phase, and the normal term entirely.  Downstream of atan2 -- the yaw command
// of a heading env that is not standing, and error_vel_yaw of a term with heading_command -- the largest
// differences are measured and printed; the test bounds them.  A heading error of the reference within 1e-5 rad of
// the wrap's ends +-pi is an edge: there the two atan2 may fall on different sides, and the value is compared only
// when it is bit-equal (the fixture's exact +-pi cases are).
// dump.bin, when named, receives the header's own state after every step (the layout above, without resampled):
// what the GPU tests compare the kernels with, bit for bit.
// Then the stream layout: which block and word each draw of a term is.
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../allsteps_isaaclab_amd/csrc/allsteps_commands.h"

namespace {

struct Reader {
  FILE* f;
  bool ok = true;
  template <typename T>
  T one() {
    T v{};
    if (fread(&v, sizeof(T), 1, f) != 1) ok = false;
    return v;
  }
  template <typename T>
  std::vector<T> many(size_t n) {
    std::vector<T> v(n);
    if (n && fread(v.data(), sizeof(T), n, f) != n) ok = false;
    return v;
  }
};

uint32_t bits(float x) {
  uint32_t u;
  std::memcpy(&u, &x, sizeof u);
  return u;
}

int check_philox(Reader& r) {
  const int32_t nq = r.one<int32_t>();
  int bad = 0;
  for (int q = 0; q < nq && r.ok; ++q) {
    const std::vector<uint32_t> w = r.many<uint32_t>(6);
    const std::vector<float> expect = r.many<float>(4);
    if (!r.ok) break;
    float got[4];
    as::noise_philox_block((uint64_t)w[0] | (uint64_t)w[1] << 32, w[2], w[3], w[4], w[5], got);
    for (int j = 0; j < 4; ++j) bad += bits(got[j]) != bits(expect[j]);
  }
  printf("philox: %d queries, %d mismatches\n", (int)nq, bad);
  return bad;
}

// the state of a case in the kernel's layouts
struct State {
  std::vector<float> vel, heading, time_left, metrics, last;
  std::vector<int32_t> flags, counter;
  void read(Reader& r, size_t K, size_t N, bool with_last) {
    vel = r.many<float>(K * 3 * N);
    heading = r.many<float>(K * N);
    flags = r.many<int32_t>(K * as::kCommandFlagRows * N);
    time_left = r.many<float>(K * N);
    counter = r.many<int32_t>(K * N);
    metrics = r.many<float>(K * as::kCommandMetricRows * N);
    if (with_last) last = r.many<float>(K * as::kCommandMetricRows * N);
  }
  void zero(size_t K, size_t N) {
    vel.assign(K * 3 * N, 0.f);
    heading.assign(K * N, 0.f);
    flags.assign(K * as::kCommandFlagRows * N, 0);
    time_left.assign(K * N, 0.f);
    counter.assign(K * N, 0);
    metrics.assign(K * as::kCommandMetricRows * N, 0.f);
    last.assign(K * as::kCommandMetricRows * N, 0.f);
  }
  void load(size_t k, size_t e, size_t N, as::CommandState& s) const {
    for (size_t a = 0; a < 3; ++a) s.vel[a] = vel[(k * 3 + a) * N + e];
    s.heading_target = heading[k * N + e];
    for (size_t a = 0; a < as::kCommandFlagRows; ++a) s.flag[a] = flags[(k * as::kCommandFlagRows + a) * N + e] != 0;
    s.time_left = time_left[k * N + e];
    s.counter = counter[k * N + e];
    for (size_t a = 0; a < as::kCommandMetricRows; ++a) s.metrics[a] = metrics[(k * as::kCommandMetricRows + a) * N + e];
  }
  void store(size_t k, size_t e, size_t N, const as::CommandState& s, const float* last2, bool was_reset) {
    for (size_t a = 0; a < 3; ++a) vel[(k * 3 + a) * N + e] = s.vel[a];
    heading[k * N + e] = s.heading_target;
    for (size_t a = 0; a < as::kCommandFlagRows; ++a) flags[(k * as::kCommandFlagRows + a) * N + e] = s.flag[a];
    time_left[k * N + e] = s.time_left;
    counter[k * N + e] = s.counter;
    for (size_t a = 0; a < as::kCommandMetricRows; ++a) {
      metrics[(k * as::kCommandMetricRows + a) * N + e] = s.metrics[a];
      if (was_reset) last[(k * as::kCommandMetricRows + a) * N + e] = last2[a];
    }
  }
  void dump(FILE* f) const {
    fwrite(vel.data(), 4, vel.size(), f);
    fwrite(heading.data(), 4, heading.size(), f);
    fwrite(flags.data(), 4, flags.size(), f);
    fwrite(time_left.data(), 4, time_left.size(), f);
    fwrite(counter.data(), 4, counter.size(), f);
    fwrite(metrics.data(), 4, metrics.size(), f);
    fwrite(last.data(), 4, last.size(), f);
  }
};

struct Measure {
  double yaw = 0, yaw_per_stiffness = 0, err_yaw = 0;
  long compared = 0, edges = 0;
};

// exact comparison of two states but for what is downstream of atan2, which is measured
int compare(const State& got, const State& want, const std::vector<as_command_term_t>& desc, size_t K, size_t N,
            bool with_last, Measure& m, long& checked) {
  int bad = 0;
  for (size_t k = 0; k < K; ++k) {
    const bool heading_term = desc[k].kind == AS_COMMAND_UNIFORM && desc[k].heading;
    for (size_t e = 0; e < N; ++e) {
      const auto flag = [&](const State& s, int a) { return s.flags[(k * as::kCommandFlagRows + a) * N + e] != 0; };
      for (size_t a = 0; a < as::kCommandFlagRows; ++a, ++checked) bad += flag(got, (int)a) != flag(want, (int)a);
      bad += bits(got.heading[k * N + e]) != bits(want.heading[k * N + e]);
      bad += bits(got.time_left[k * N + e]) != bits(want.time_left[k * N + e]);
      bad += got.counter[k * N + e] != want.counter[k * N + e];
      checked += 3;
      for (size_t a = 0; a < 3; ++a, ++checked) {
        const float g = got.vel[(k * 3 + a) * N + e], w = want.vel[(k * 3 + a) * N + e];
        const bool soft = a == 2 && heading_term && flag(want, as::kCmdHeading) && !flag(want, as::kCmdStanding);
        if (!soft || bits(g) == bits(w)) {
          bad += bits(g) != bits(w);
          continue;
        }
        const double st = std::fabs((double)desc[k].stiffness);
        if (st > 0 && std::fabs(std::fabs((double)w) / st - (double)as::kCommandPi) < 1e-5) {
          ++m.edges;
          continue;
        }
        const double d = std::fabs((double)g - (double)w);
        m.yaw = std::fmax(m.yaw, d);
        if (st > 0) m.yaw_per_stiffness = std::fmax(m.yaw_per_stiffness, d / st);
        ++m.compared;
      }
      for (size_t a = 0; a < as::kCommandMetricRows; ++a, ++checked) {
        const size_t i = (k * as::kCommandMetricRows + a) * N + e;
        for (int which = 0; which < (with_last ? 2 : 1); ++which) {
          const float g = which ? got.last[i] : got.metrics[i], w = which ? want.last[i] : want.metrics[i];
          if (a == as::kCmdErrYaw && heading_term && bits(g) != bits(w)) {
            if (std::isfinite(g) && std::isfinite(w)) m.err_yaw = std::fmax(m.err_yaw, std::fabs((double)g - (double)w));
            else ++bad;
          } else {
            bad += bits(g) != bits(w);
          }
        }
      }
    }
  }
  return bad;
}

int check_cases(Reader& r, FILE* dump) {
  static_assert(sizeof(as_command_term_t) == 21 * sizeof(float), "as_command_term_t is 21 packed words");
  const int32_t ncases = r.one<int32_t>();
  int bad = 0;
  long checked = 0, resamples = 0, doubles = 0;
  Measure m;
  for (int c = 0; c < ncases && r.ok; ++c) {
    const std::vector<int32_t> h = r.many<int32_t>(4);
    if (!r.ok) break;
    const int n = h[0], terms = h[1], steps = h[2], has_init = h[3];
    if (n < 1 || n > 4096 || terms < 1 || terms > AS_MAX_COMMAND_TERMS || steps < 1 || steps > 1000) {
      printf("case %d: bad header\n", c);
      return 1;
    }
    const float dt = r.one<float>();
    const size_t N = (size_t)n, K = (size_t)terms, D = as::kCommandDraws;
    const std::vector<float> rows = r.many<float>(K * 21);
    std::vector<as_command_term_t> desc(K);
    if (!r.ok) break;
    std::memcpy(desc.data(), rows.data(), K * sizeof(as_command_term_t));
    State st0;
    st0.read(r, K, N, false);
    st0.last.assign(K * as::kCommandMetricRows * N, 0.f);
    const std::vector<float> init = r.many<float>(K * D * N);
    if (!r.ok) break;
    int case_bad = 0;
    const float q0[4] = {1.f, 0.f, 0.f, 0.f}, v0[3] = {0.f, 0.f, 0.f};
    if (has_init) {  // the reset-only entry from the zero state
      State z;
      z.zero(K, N);
      for (size_t e = 0; e < N; ++e)
        for (size_t k = 0; k < K; ++k) {
          as::CommandState s;
          z.load(k, e, N, s);
          float last[as::kCommandMetricRows];
          as::command_term_step(desc[k], s, last, true, false, dt, q0, v0, v0,
                                [&](uint32_t, float (&d)[as::kCommandDraws]) {
                                  for (size_t a = 0; a < D; ++a) d[a] = init[(k * D + a) * N + e];
                                });
          z.store(k, e, N, s, last, true);
        }
      case_bad += compare(z, st0, desc, K, N, false, m, checked);
    }
    State st = st0;
    for (int s = 0; s < steps && r.ok; ++s) {
      const std::vector<float> quat = r.many<float>(4 * N), lin = r.many<float>(3 * N), ang = r.many<float>(3 * N);
      const std::vector<int32_t> reset = r.many<int32_t>(N);
      const std::vector<float> draws = r.many<float>(2 * K * D * N);
      State want;
      want.read(r, K, N, true);
      const std::vector<int32_t> resampled = r.many<int32_t>(2 * K * N);
      if (!r.ok) break;
      for (size_t e = 0; e < N; ++e) {
        const float q[4] = {quat[e], quat[N + e], quat[2 * N + e], quat[3 * N + e]};
        const float l[3] = {lin[e], lin[N + e], lin[2 * N + e]}, a3[3] = {ang[e], ang[N + e], ang[2 * N + e]};
        for (size_t k = 0; k < K; ++k) {
          as::CommandState cs;
          st.load(k, e, N, cs);
          float last[as::kCommandMetricRows];
          const int got = as::command_term_step(
              desc[k], cs, last, reset[e] != 0, true, dt, q, l, a3, [&](uint32_t tag, float (&d)[as::kCommandDraws]) {
                const size_t phase = tag == as::kCommandComputeTag ? 1 : 0;
                for (size_t a = 0; a < D; ++a) d[a] = draws[((phase * K + k) * D + a) * N + e];
              });
          st.store(k, e, N, cs, last, reset[e] != 0);
          const int expect = (resampled[k * N + e] ? 1 : 0) | (resampled[(K + k) * N + e] ? 2 : 0);
          case_bad += got != expect;
          resamples += (got & 1) + (got >> 1);
          doubles += got == 3;
          ++checked;
        }
      }
      case_bad += compare(st, want, desc, K, N, true, m, checked);
      if (dump) st.dump(dump);
      // what is downstream of atan2 follows the reference from here on, so that a difference is measured once and
      // not carried along: the yaw commands and error_vel_yaw are taken over where they differ within the measure
      for (size_t k = 0; k < K; ++k)
        if (desc[k].kind == AS_COMMAND_UNIFORM && desc[k].heading && !dump)
          for (size_t e = 0; e < N; ++e) {
            st.vel[(k * 3 + 2) * N + e] = want.vel[(k * 3 + 2) * N + e];
            st.metrics[(k * 2 + 1) * N + e] = want.metrics[(k * 2 + 1) * N + e];
            st.last[(k * 2 + 1) * N + e] = want.last[(k * 2 + 1) * N + e];
          }
    }
    if (case_bad) printf("case %d (n %d terms %d steps %d): %d mismatches\n", c, n, terms, steps, case_bad);
    bad += case_bad;
  }
  printf("commands fixture: %d cases, %ld values, %ld resamples, %ld double resamples, %d mismatches\n", (int)ncases,
         checked, resamples, doubles, bad);
  printf("heading: %ld yaw commands differ, max |diff| %.9g rad/s, per unit stiffness %.9g rad; error_vel_yaw max "
         "|diff| %.9g; %ld at the wrap's edge\n", m.compared, m.yaw, m.yaw_per_stiffness, m.err_yaw, m.edges);
  return bad;
}

// block and word of the draws: term k owns blocks 3k .. 3k + 2 of the phase's tag
int check_layout() {
  int bad = 0;
  const uint64_t seed = 0xfedcba9876543210ull;
  for (int term = 0; term < AS_MAX_COMMAND_TERMS; ++term)
    for (uint32_t tag : {as::kCommandResetTag, as::kCommandComputeTag}) {
      float u[12], d[as::kCommandDraws];
      for (int b = 0; b < 3; ++b) as::noise_philox_block(seed, 77u, 9u, (uint32_t)(3 * term + b), tag, u + 4 * b);
      as_command_term_t c{};
      c.kind = AS_COMMAND_UNIFORM;
      as::command_draws(c, seed, 77u, 9u, term, tag, d);
      for (int a = 0; a < 7; ++a) bad += bits(d[a]) != bits(u[a]);
      c.kind = AS_COMMAND_NORMAL;
      as::command_draws(c, seed, 77u, 9u, term, tag, d);
      float z[4];
      as::noise_box_muller(u[1], u[2], &z[0], &z[1]);
      as::noise_box_muller(u[3], u[4], &z[2], &z[3]);
      bad += bits(d[0]) != bits(u[0]);
      for (int a = 0; a < 3; ++a) bad += bits(d[1 + a]) != bits(z[a]);
      for (int a = 0; a < 7; ++a) bad += bits(d[4 + a]) != bits(u[5 + a]);
    }
  bad += as::kCommandResetTag != 0x436d5273u || as::kCommandComputeTag != 0x436d4370u;
  // wrap_to_pi's ends and torch's %: pi and odd multiples go to +-pi by sign
  bad += bits(as::command_wrap_to_pi(as::kCommandPi)) != bits(as::kCommandPi);
  bad += bits(as::command_wrap_to_pi(-as::kCommandPi)) != bits(-as::kCommandPi);
  bad += bits(as::command_wrap_to_pi(0.f)) != bits(0.f);
  bad += as::command_wrap_to_pi(-4.f) <= 0.f;
  // the sample is one fused multiply-add
  bad += bits(as::command_sample(0.3f, 0.26f, 0.11f)) != bits(fmaf(0.3f, 0.26f, 0.11f));
  printf("stream layout, wrap and sample: %d mismatches\n", bad);
  return bad;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2 && argc != 3) {
    fprintf(stderr, "usage: %s cases.bin [dump.bin]\n", argv[0]);
    return 2;
  }
  FILE* f = fopen(argv[1], "rb");
  if (!f) {
    perror(argv[1]);
    return 2;
  }
  FILE* dump = nullptr;
  if (argc == 3 && !(dump = fopen(argv[2], "wb"))) {
    perror(argv[2]);
    fclose(f);
    return 2;
  }
  Reader r{f};
  int bad = check_philox(r);
  bad += check_cases(r, dump);
  const bool at_end = r.ok && fgetc(f) == EOF;
  fclose(f);
  if (dump) fclose(dump);
  if (!at_end) {
    printf("cases.bin: truncated or trailing bytes\n");
    return 1;
  }
  bad += check_layout();
  return bad ? 1 : 0;
}
