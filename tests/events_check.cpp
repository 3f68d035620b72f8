// events_check.cpp -- stand-alone host check of csrc/allsteps_events.h (tests/test_events_host.py builds and
// runs it, plain and under -fsanitize=address,undefined).
//
//   events_check <cases.bin>
//
// cases.bin (written by the test from tests/golden/events.npz, native endianness, 4-byte words):
//   int32 nphilox, then per query: uint32 seed_lo, seed_hi, env, t, b, tag; float expect[4]
//     (the oracle's or_philox_block for the two event tags) -- noise_philox_block must give the same bits;
//   int32 ncases, then per case
//     int32 n, terms, steps, has_init;  float dt
//     float rows[terms][14] (as_event_term_t), vel0[6][n], time_left0[terms][n]
//     has_init: float init_draws[terms][n] -- time_left0 must be event_sample of them (the initial timers)
//     per step: float iv_draws[terms][n], push_draws[terms][6][n], time_left_expect[terms][n];
//               int32 fired_expect[terms][n]; float vel_expect[6][n]
//   -- the reference's outputs from the same draws.  The program replays a case the way k_events_interval does
//   (terms in order on the env's velocity) with the header's functions and demands every value bit for bit.
// Then the stream layout: which block and word an interval draw and the six push draws are.
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../allsteps_isaaclab_amd/csrc/allsteps_events.h"

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

int check_cases(Reader& r) {
  static_assert(sizeof(as_event_term_t) == 14 * sizeof(float), "as_event_term_t is 14 packed floats");
  const int32_t ncases = r.one<int32_t>();
  int bad = 0;
  long checked = 0, firings = 0;
  for (int c = 0; c < ncases && r.ok; ++c) {
    const std::vector<int32_t> h = r.many<int32_t>(4);
    if (!r.ok) break;
    const int n = h[0], terms = h[1], steps = h[2], has_init = h[3];
    if (n < 1 || n > 4096 || terms < 1 || terms > AS_MAX_EVENT_TERMS || steps < 1 || steps > 1000) {
      printf("case %d: bad header\n", c);
      return 1;
    }
    const float dt = r.one<float>();
    const size_t N = (size_t)n, K = (size_t)terms;
    const std::vector<float> rows = r.many<float>(K * 14);
    std::vector<float> vel = r.many<float>(6 * N);
    std::vector<float> tl = r.many<float>(K * N);
    if (!r.ok) break;
    std::vector<as_event_term_t> desc(K);
    std::memcpy(desc.data(), rows.data(), K * sizeof(as_event_term_t));
    int case_bad = 0;
    if (has_init) {
      const std::vector<float> u0 = r.many<float>(K * N);
      if (!r.ok) break;
      for (size_t k = 0; k < K; ++k)
        for (size_t e = 0; e < N; ++e) {
          case_bad += bits(as::event_sample(u0[k * N + e], desc[k].interval_w, desc[k].interval_lo)) != bits(tl[k * N + e]);
          ++checked;
        }
    }
    for (int s = 0; s < steps && r.ok; ++s) {
      const std::vector<float> iv = r.many<float>(K * N), push = r.many<float>(K * 6 * N);
      const std::vector<float> tl_expect = r.many<float>(K * N);
      const std::vector<int32_t> fired_expect = r.many<int32_t>(K * N);
      const std::vector<float> vel_expect = r.many<float>(6 * N);
      if (!r.ok) break;
      for (size_t e = 0; e < N; ++e) {
        float v[6];
        for (size_t a = 0; a < 6; ++a) v[a] = vel[a * N + e];
        for (size_t k = 0; k < K; ++k) {
          float u6[6];
          for (size_t a = 0; a < 6; ++a) u6[a] = push[(k * 6 + a) * N + e];
          const bool fire = as::event_term_step(desc[k], dt, &tl[k * N + e], v, iv[k * N + e], u6);
          case_bad += (int)fire != fired_expect[k * N + e];
          case_bad += bits(tl[k * N + e]) != bits(tl_expect[k * N + e]);
          firings += fire;
          checked += 2;
        }
        for (size_t a = 0; a < 6; ++a) {
          vel[a * N + e] = v[a];
          case_bad += bits(v[a]) != bits(vel_expect[a * N + e]);
          ++checked;
        }
      }
    }
    if (case_bad) printf("case %d (n %d terms %d steps %d): %d mismatches\n", c, n, terms, steps, case_bad);
    bad += case_bad;
  }
  printf("events fixture: %d cases, %ld values, %ld firings, %d mismatches\n", (int)ncases, checked, firings, bad);
  return bad;
}

// block and word of the draws: interval = block term, word 0; push = blocks 2 term, 2 term + 1, words
// x y z roll | pitch yaw
int check_layout() {
  int bad = 0;
  const uint64_t seed = 0xfedcba9876543210ull;
  for (int term = 0; term < AS_MAX_EVENT_TERMS; ++term) {
    float a[4], b[4], u6[6];
    as::noise_philox_block(seed, 77u, 9u, (uint32_t)term, as::kEventIntervalTag, a);
    bad += bits(as::event_interval_draw(seed, 77u, 9u, term)) != bits(a[0]);
    as::noise_philox_block(seed, 77u, 9u, (uint32_t)(2 * term), as::kEventPushTag, a);
    as::noise_philox_block(seed, 77u, 9u, (uint32_t)(2 * term + 1), as::kEventPushTag, b);
    as::event_push_draws(seed, 77u, 9u, term, u6);
    const float want[6] = {a[0], a[1], a[2], a[3], b[0], b[1]};
    for (int k = 0; k < 6; ++k) bad += bits(u6[k]) != bits(want[k]);
  }
  bad += as::kEventIntervalTag != 0x45764976u || as::kEventPushTag != 0x45765075u;
  // the fire test: strictly below float32(1e-6)
  float tl = 1e-6f;
  bad += as::event_tick(&tl, 0.f);
  tl = std::nextafterf(1e-6f, 0.f);
  bad += !as::event_tick(&tl, 0.f);
  printf("stream layout and fire test: %d mismatches\n", bad);
  return bad;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: %s cases.bin\n", argv[0]);
    return 2;
  }
  FILE* f = fopen(argv[1], "rb");
  if (!f) {
    perror(argv[1]);
    return 2;
  }
  Reader r{f};
  int bad = check_philox(r);
  bad += check_cases(r);
  const bool at_end = r.ok && fgetc(f) == EOF;
  fclose(f);
  if (!at_end) {
    printf("cases.bin: truncated or trailing bytes\n");
    return 1;
  }
  bad += check_layout();
  return bad ? 1 : 0;
}
