// observations_check.cpp -- stand-alone host check of csrc/allsteps_observations.h (tests/test_observations_host.py
// builds and runs it, plain and under -fsanitize=address,undefined).
//
//   observations_check <cases.bin> [<dump.bin>]
//   observations_check --draws <request.bin> <draws.bin>
//
// --draws: request.bin holds uint32 seed_lo, seed_hi, env0, group, d0, noise kind, n, then uint32 t[n]; draws.bin
// receives float obs_draw[d0][n] -- the header's own draws (uniforms, or its Box-Muller normals through the host's
// libm), what the GPU tests compare the kernel's Philox path with.
//
// cases.bin (written by the test from tests/golden/observations.npz and the groups parsed by envs/observations.py,
// native endianness, 4-byte words):
//   int32 nphilox, then per query: uint32 seed_lo, seed_hi, env, t, b, tag; float expect[4]
//     (the oracle's or_philox_block for the observation tag) -- noise_philox_block must give the same bits;
//   int32 ncases, then per case
//     int32 n, terms, d0, out_cols, steps, group
//     words terms[terms][12] (as_observation_term_t), cols[AS_OBS_COL_ROWS][AS_MAX_OBS_COLS], int32 omap[out_cols]
//     int32 rows[AS_OBS_NUM_SOURCES]
//     per step: for every source but the gravity constant float data[rows][n] (the actions [n][rows]);
//               float draws[d0][n]; int32 reset[n]; float expect[n][out_cols]
// The program replays a case the way k_observations does -- one env at a time, the header's functions, the history
// kept in the output row -- from a zero row and push count 0, and compares every output word of every step with the
// reference's bit for bit (two NaNs are equal).  dump.bin, when named, receives the header's own out [n][out_cols]
// after every step.  Then the stream layout: which block and word each column's draw is.
#include <cinttypes>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../allsteps_isaaclab_amd/csrc/allsteps_observations.h"

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

bool same(float a, float b) { return bits(a) == bits(b) || (std::isnan(a) && std::isnan(b)); }

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

int check_layout() {
  int bad = 0;
  const uint64_t seed = 0x1234567887654321ull;
  for (int g = 0; g < AS_MAX_OBS_GROUPS; ++g)
    for (int c = 0; c < AS_MAX_OBS_COLS; c += 7) {
      float u4[4], z4[4];
      as::noise_philox_block(seed, 5u + c, 9u, (uint32_t)(g * 64 + c / 4), as::kObsTag, u4);
      as::noise_block_draws(AS_NOISE_GAUSSIAN, u4, z4);
      bad += bits(as::obs_draw(AS_NOISE_UNIFORM, seed, 5u + c, 9u, g, c)) != bits(u4[c % 4]);
      bad += bits(as::obs_draw(AS_NOISE_GAUSSIAN, seed, 5u + c, 9u, g, c)) != bits(z4[c % 4]);
      bad += as::obs_draw(AS_NOISE_CONSTANT, seed, 5u + c, 9u, g, c) != 0.0f;
    }
  // the clip's edge cases: a NaN passes, a zero keeps its sign, lo > hi gives hi
  bad += !std::isnan(as::obs_clip(NAN, -1.f, 1.f));
  bad += bits(as::obs_clip(-0.0f, 0.0f, 1.0f)) != bits(-0.0f);
  bad += as::obs_clip(INFINITY, -1.f, 1.f) != 1.f || as::obs_clip(-INFINITY, -1.f, 1.f) != -1.f;
  bad += as::obs_clip(0.5f, 2.f, 1.f) != 1.f;
  // the output map's word
  const int32_t m = as::obs_omap_pack(255, true, 256);
  bad += as::obs_omap_col(m) != 255 || !as::obs_omap_last(m) || as::obs_omap_width(m) != 256;
  printf("stream layout, clip and map: %d mismatches\n", bad);
  return bad;
}

int dump_draws(const char* request, const char* path) {
  FILE* f = fopen(request, "rb");
  if (!f) {
    perror(request);
    return 2;
  }
  Reader r{f};
  const std::vector<uint32_t> h = r.many<uint32_t>(7);
  const std::vector<uint32_t> t = r.ok ? r.many<uint32_t>(h[6]) : std::vector<uint32_t>();
  fclose(f);
  if (!r.ok || h[3] >= AS_MAX_OBS_GROUPS || h[4] < 1 || h[4] > AS_MAX_OBS_COLS) {
    fprintf(stderr, "%s: bad request\n", request);
    return 2;
  }
  const uint64_t seed = (uint64_t)h[0] | (uint64_t)h[1] << 32;
  std::vector<float> out((size_t)h[4] * h[6]);
  for (uint32_t c = 0; c < h[4]; ++c)
    for (uint32_t e = 0; e < h[6]; ++e)
      out[(size_t)c * h[6] + e] = as::obs_draw((int)h[5], seed, h[2] + e, t[e], (int)h[3], (int)c);
  FILE* o = fopen(path, "wb");
  if (!o) {
    perror(path);
    return 2;
  }
  fwrite(out.data(), 4, out.size(), o);
  fclose(o);
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc == 4 && !strcmp(argv[1], "--draws")) return dump_draws(argv[2], argv[3]);
  if (argc < 2) {
    fprintf(stderr, "usage: %s <cases.bin> [<dump.bin>]\n", argv[0]);
    return 2;
  }
  FILE* f = fopen(argv[1], "rb");
  if (!f) {
    perror(argv[1]);
    return 2;
  }
  FILE* dump = argc > 2 ? fopen(argv[2], "wb") : nullptr;
  Reader r{f};
  int bad = check_philox(r);
  const int32_t ncases = r.one<int32_t>();
  long total = 0, mismatches = 0, history_moves = 0, fills = 0, nans = 0, infs = 0;
  for (int ci = 0; ci < ncases && r.ok; ++ci) {
    const int32_t n = r.one<int32_t>(), nt = r.one<int32_t>(), d0 = r.one<int32_t>(), oc = r.one<int32_t>(),
                  steps = r.one<int32_t>(), group = r.one<int32_t>();
    if (!r.ok || n < 1 || nt < 1 || nt > AS_MAX_OBS_TERMS || d0 < 1 || d0 > AS_MAX_OBS_COLS || oc < d0 ||
        oc > AS_MAX_OBS_OUT_COLS) {
      fprintf(stderr, "case %d: bad header\n", ci);
      return 2;
    }
    static_assert(sizeof(as_observation_term_t) == 12 * 4, "as_observation_term_t is 12 words");
    std::vector<as_observation_term_t> terms = r.many<as_observation_term_t>((size_t)nt);
    const std::vector<uint32_t> cols = r.many<uint32_t>((size_t)AS_OBS_COL_ROWS * AS_MAX_OBS_COLS);
    const std::vector<int32_t> omap = r.many<int32_t>((size_t)oc);
    const std::vector<int32_t> rows = r.many<int32_t>(AS_OBS_NUM_SOURCES);
    std::vector<float> out((size_t)n * oc, 0.0f), fresh((size_t)d0);
    std::vector<int> count((size_t)n, 0);
    long case_bad = 0;
    for (int s = 0; s < steps && r.ok; ++s) {
      std::vector<std::vector<float>> src(AS_OBS_NUM_SOURCES);
      for (int k = 0; k < AS_OBS_SRC_GRAVITY; ++k) src[k] = r.many<float>((size_t)rows[k] * n);
      const std::vector<float> draws = r.many<float>((size_t)d0 * n);
      const std::vector<int32_t> reset = r.many<int32_t>((size_t)n);
      const std::vector<float> expect = r.many<float>((size_t)n * oc);
      if (!r.ok) break;
      std::vector<float> d((size_t)d0);
      for (int e = 0; e < n; ++e) {
        auto load = [&](int source, int row) -> float {
          if (source < 0 || source >= AS_OBS_SRC_GRAVITY || row < 0 || row >= rows[source]) return 0.0f;
          return source == AS_OBS_SRC_ACTIONS ? src[source][(size_t)e * rows[source] + row]
                                              : src[source][(size_t)row * n + e];
        };
        for (int c = 0; c < d0; ++c) d[c] = draws[(size_t)c * n + e];
        const bool rs = reset[e] != 0;
        if (rs || count[e] == 0) ++fills;
        count[e] = as::obs_group_env_step(terms.data(), nt, cols.data(), omap.data(), d0, oc, group, rs, count[e],
                                          &out[(size_t)e * oc], d.data(), 0, (uint32_t)e, (uint32_t)s, fresh.data(),
                                          load);
        for (int c = 0; c < oc; ++c) {
          const float got = out[(size_t)e * oc + c], want = expect[(size_t)e * oc + c];
          ++total;
          nans += std::isnan(want);
          infs += std::isinf(want);
          history_moves += !as::obs_omap_last(omap[c]);
          if (!same(got, want)) {
            if (++case_bad <= 5)
              fprintf(stderr, "case %d step %d env %d column %d: got %.9g (%08" PRIx32 ") want %.9g (%08" PRIx32 ")\n",
                      ci, s, e, c, got, bits(got), want, bits(want));
          }
        }
      }
      if (dump) fwrite(out.data(), 4, out.size(), dump);
    }
    mismatches += case_bad;
  }
  if (!r.ok) {
    fprintf(stderr, "cases.bin: short read\n");
    return 2;
  }
  printf("observations fixture: %d cases, %ld values (%ld history slots, %ld first pushes, %ld NaN, %ld inf), "
         "%ld mismatches\n", (int)ncases, total, history_moves, fills, nans, infs, mismatches);
  bad += (int)(mismatches != 0);
  bad += check_layout();
  if (dump) fclose(dump);
  fclose(f);
  return bad ? 1 : 0;
}
