// noise_check.cpp -- stand-alone host check of csrc/allsteps_noise.h (tests/test_noise_host.py builds and
// runs it, plain and under -fsanitize=address,undefined).
//
//   noise_check <cases.bin>
//
// cases.bin (written by the test from tests/golden/noise.npz, native endianness, 4-byte words):
//   int32 nphilox, then per query: uint32 seed_lo, seed_hi, env, t, b, tag; float expect[4]
//     (the oracle's or_philox_block) -- noise_philox_block must give the same bits;
//   int32 ncases, then per case
//     int32 n, cols, kind, op, bias_kind, bias_op, steps;  float bias_p0, bias_p1
//     float p0[cols], p1[cols], x[n * cols], draws[n * cols]
//     per step: int32 mask[n]; float bias_draw[n], bias_expect[n], out_expect[n * cols]
//   -- the reference's outputs from the same draws.  The program replays a case the way k_noise_post does
//   (bias re-draw of the masked envs from the old bias, then term + bias) with the header's formulas and
//   demands every output bit for bit.
// Then the host Box-Muller against a float64 one over Philox uniforms and the edge draws (bound 1e-5), and
// the lane-group sizes of the kernels' work mapping.
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../allsteps_isaaclab_amd/csrc/allsteps_noise.h"

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
  const int32_t ncases = r.one<int32_t>();
  int bad = 0;
  long checked = 0;
  for (int c = 0; c < ncases && r.ok; ++c) {
    const std::vector<int32_t> h = r.many<int32_t>(7);
    if (!r.ok) break;
    const int n = h[0], cols = h[1], kind = h[2], op = h[3], bkind = h[4], bop = h[5], steps = h[6];
    if (n < 1 || cols < 1 || cols > as::kNoiseMaxCols || steps < 1 || steps > 2) {
      printf("case %d: bad header\n", c);
      return 1;
    }
    const float bp0 = r.one<float>(), bp1 = r.one<float>();
    const size_t nc = (size_t)n * (size_t)cols;
    const std::vector<float> p0 = r.many<float>(cols), p1 = r.many<float>(cols);
    const std::vector<float> x = r.many<float>(nc), draws = r.many<float>(nc);
    std::vector<float> bias((size_t)n, 0.f);
    int case_bad = 0;
    for (int s = 0; s < steps && r.ok; ++s) {
      const std::vector<int32_t> mask = r.many<int32_t>(n);
      const std::vector<float> bdraw = r.many<float>(n), bias_expect = r.many<float>(n);
      const std::vector<float> out_expect = r.many<float>(nc);
      if (!r.ok) break;
      for (int e = 0; e < n; ++e) {
        if (bkind != AS_NOISE_NONE) {
          if (mask[e]) bias[e] = as::noise_term(bkind, bop, bias[e], bdraw[e], bp0, bp1);
          case_bad += bits(bias[e]) != bits(bias_expect[e]);
          ++checked;
        }
        for (int k = 0; k < cols; ++k) {
          const size_t i = (size_t)e * (size_t)cols + (size_t)k;
          float v = as::noise_term(kind, op, x[i], draws[i], p0[k], p1[k]);
          if (bkind != AS_NOISE_NONE) v = as::noise_add_bias(v, bias[e]);
          case_bad += bits(v) != bits(out_expect[i]);
          ++checked;
        }
      }
    }
    if (case_bad) printf("case %d (kind %d op %d cols %d bias %d/%d): %d mismatches\n", c, kind, op, cols, bkind, bop, case_bad);
    bad += case_bad;
  }
  printf("noise fixture: %d cases, %ld values, %d mismatches\n", (int)ncases, checked, bad);
  return bad;
}

// the host Box-Muller against float64 from the same uniforms: Philox draws and the edges of [0, 1)
int check_box_muller() {
  const double two_pi = 6.283185307179586476925286766559;
  const float edge[] = {0.f, 1.0f / 16777216.0f, 0.25f, 0.5f, 0.75f, 1.0f - 1.0f / 16777216.0f};
  double worst = 0.0, s1 = 0.0, s2 = 0.0;
  long count = 0;
  auto one = [&](float u0, float u1) {
    float z0, z1;
    as::noise_box_muller(u0, u1, &z0, &z1);
    const double rr = std::sqrt(-2.0 * std::log(1.0 - (double)u0));
    const double e0 = std::fabs((double)z0 - rr * std::cos(two_pi * (double)u1));
    const double e1 = std::fabs((double)z1 - rr * std::sin(two_pi * (double)u1));
    worst = std::fmax(worst, std::fmax(e0, e1));
    return z0 + z1;
  };
  for (float a : edge)
    for (float b : edge) (void)one(a, b);
  for (uint32_t e = 0; e < 4096; ++e) {
    float u[4], x[4];
    as::noise_philox_block(0x1234567890abcdefull, e, 7u, e & 15u, as::kNoiseObsTag, u);
    (void)one(u[0], u[1]);
    (void)one(u[2], u[3]);
    as::noise_block_draws(AS_NOISE_GAUSSIAN, u, x);
    for (int j = 0; j < 4; ++j) {
      s1 += x[j];
      s2 += (double)x[j] * x[j];
      ++count;
    }
  }
  const double mean = s1 / (double)count, var = s2 / (double)count - mean * mean;
  printf("box-muller: max abs error %.3e (bound 1e-05), %ld draws mean %.4f var %.4f\n", worst, count, mean, var);
  // 16384 draws: |mean| < 5 / sqrt(N) = 0.039, |var - 1| < 5 sqrt(2 / N) = 0.055
  return !(worst <= 1e-5) || !(std::fabs(mean) < 0.039) || !(std::fabs(var - 1.0) < 0.055);
}

int check_groups() {
  const int cols[] = {1, 4, 5, 12, 21, 59, 64, 65, 256, 0};
  const int want[] = {1, 1, 2, 4, 8, 16, 16, 32, 64, 1};
  int bad = 0;
  for (int i = 0; i < 10; ++i) bad += as::noise_group(cols[i]) != want[i];
  // the bias draw is block 0, word 0 of its stream
  float u[4];
  as::noise_philox_block(42u, 5u, 9u, 0u, as::kNoiseObsBiasTag, u);
  bad += bits(as::noise_bias_draw(AS_NOISE_UNIFORM, 42u, 5u, 9u, as::kNoiseObsBiasTag)) != bits(u[0]);
  float z0, z1;
  as::noise_box_muller(u[0], u[1], &z0, &z1);
  bad += bits(as::noise_bias_draw(AS_NOISE_GAUSSIAN, 42u, 5u, 9u, as::kNoiseObsBiasTag)) != bits(z0);
  bad += as::noise_bias_draw(AS_NOISE_CONSTANT, 42u, 5u, 9u, as::kNoiseObsBiasTag) != 0.f;
  printf("groups and bias draw: %d mismatches\n", bad);
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
  bad += check_box_muller();
  bad += check_groups();
  return bad ? 1 : 0;
}
