// terminations_check.cpp -- a stand-alone program around csrc/allsteps_terminations.h
// (tests/test_terminations_host.py builds it once plain and once with -fsanitize=address,undefined and runs it
// directly).
//
//   terminations_check cases.bin dump.bin
//   terminations_check acos x.bin y.bin        term_acosf of every float32 of x.bin
//
// cases.bin (little endian, written by the test from tests/golden/terminations.npz and the tables
// envs/terminations.py makes): int32 cases; per case: int32 n, terms, steps, joint_rows, depth, bodies, command_terms,
// step_flags; float32 sim_dt; per step: the descriptor rows [terms][8], the index table [3][16][32], root_pos [3][n],
// root_quat [4][n], q, qd [joint_rows][n], time_left [command_terms][n], command_counter [command_terms][n] int32, net
// [depth][bodies][3][n], ep_len [n] int32, and with step_flags step_terminated, step_truncated [n] uint8.
// dump.bin: per case and step term_dones [terms][n], time_outs, terminated, dones [n], last_episode_dones [terms][n],
// reset_request [n] (uint8, after the step), then the angle of bad_orientation [n] float32.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../allsteps_isaaclab_amd/csrc/allsteps_terminations.h"

static_assert(sizeof(as_termination_term_t) == 8 * sizeof(uint32_t), "as_termination_term_t is 8 words");

template <typename T>
static std::vector<T> take(FILE* f, size_t count) {
  std::vector<T> v(count);
  if (count && fread(v.data(), sizeof(T), count, f) != count) {
    fprintf(stderr, "input file is truncated\n");
    exit(2);
  }
  return v;
}

template <typename T>
static void put(FILE* f, const std::vector<T>& v) {
  fwrite(v.data(), sizeof(T), v.size(), f);
}

static int acos_mode(const char* in_path, const char* out_path) {
  FILE* in = fopen(in_path, "rb");
  FILE* out = fopen(out_path, "wb");
  if (!in || !out) return 2;
  fseek(in, 0, SEEK_END);
  const size_t count = (size_t)ftell(in) / sizeof(float);
  fseek(in, 0, SEEK_SET);
  std::vector<float> x = take<float>(in, count), y(count);
  for (size_t i = 0; i < count; ++i) y[i] = as::term_acosf(x[i]);
  put(out, y);
  fclose(in);
  fclose(out);
  printf("acos: %zu values\n", count);
  return 0;
}

int main(int argc, char** argv) {
  if (argc == 4 && !strcmp(argv[1], "acos")) return acos_mode(argv[2], argv[3]);
  if (argc != 3) {
    fprintf(stderr, "usage: terminations_check cases.bin dump.bin | terminations_check acos x.bin y.bin\n");
    return 2;
  }
  FILE* in = fopen(argv[1], "rb");
  FILE* out = fopen(argv[2], "wb");
  if (!in || !out) return 2;
  const int cases = take<int32_t>(in, 1)[0];
  long items = 0, set = 0, done_envs = 0;
  for (int c = 0; c < cases; ++c) {
    const std::vector<int32_t> h = take<int32_t>(in, 8);
    const float sim_dt = take<float>(in, 1)[0];
    const size_t n = (size_t)h[0], T = (size_t)h[1];
    const int steps = h[2];
    std::vector<uint8_t> flags(T * n), time_outs(n), terminated(n), dones(n), last(T * n), request(n);
    std::vector<float> angle(n);
    for (int s = 0; s < steps; ++s) {
      const auto desc = take<as_termination_term_t>(in, T);
      const auto table =
          take<uint32_t>(in, (size_t)AS_TERMINATION_TABLE_ROWS * AS_MAX_TERMINATION_TERMS * AS_MAX_TERMINATION_IDS);
      const auto root_pos = take<float>(in, 3 * n), root_quat = take<float>(in, 4 * n);
      const auto q = take<float>(in, (size_t)h[3] * n), qd = take<float>(in, (size_t)h[3] * n);
      const auto time_left = take<float>(in, (size_t)h[6] * n);
      const auto counter = take<int32_t>(in, (size_t)h[6] * n);
      const auto net = take<float>(in, (size_t)h[4] * h[5] * 3 * n);
      const auto ep_len = take<int32_t>(in, n);
      const auto step_term = take<uint8_t>(in, h[7] ? n : 0), step_trunc = take<uint8_t>(in, h[7] ? n : 0);
      as_termination_sources_t S{};
      S.root_pos = root_pos.data();
      S.root_quat = root_quat.data();
      S.q = q.data();
      S.qd = qd.data();
      S.time_left = time_left.data();
      S.command_counter = counter.data();
      S.net = net.data();
      S.ep_len = ep_len.data();
      S.step_terminated = h[7] ? step_term.data() : nullptr;
      S.step_truncated = h[7] ? step_trunc.data() : nullptr;
      S.joint_rows = h[3];
      S.depth = h[4];
      S.bodies = h[5];
      S.command_terms = h[6];
      S.sim_dt = sim_dt;
      for (size_t e = 0; e < n; ++e) {
        as::terminations_env_step(desc.data(), (int)T, table.data(), S, n, e, flags.data(), time_outs.data(),
                                  terminated.data(), dones.data(), last.data(), request.data());
        angle[e] = as::term_orientation_angle(as::TerminationEnv{&S, n, e});
        for (size_t k = 0; k < T; ++k) set += flags[k * n + e];
        items += (long)T;
        done_envs += dones[e];
      }
      put(out, flags);
      put(out, time_outs);
      put(out, terminated);
      put(out, dones);
      put(out, last);
      put(out, request);
      put(out, angle);
    }
  }
  fclose(in);
  fclose(out);
  printf("terminations fixture: %d cases, %ld (term, env) items, %ld set, %ld done envs\n", cases, items, set,
         done_envs);
  return 0;
}
