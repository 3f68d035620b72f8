// actions_check.cpp -- a stand-alone program around csrc/allsteps_actions.h
// (tests/test_actions_host.py builds it once plain and once with -fsanitize=address,undefined and runs it directly).
//
//   actions_check cases.bin dump.bin
//
// cases.bin (little endian, written by the test from tests/golden/actions.npz and the column table envs/actions.py
// makes): int32 cases; per case: int32 n, cols, joints, steps; the column rows [cols][12]; per step: the raw action
// [n][cols], the joint positions [joints][n], int32 reset (0: none, 1: the mask's envs, 2: every env, a null mask) and
// the mask [n] uint8.
// dump.bin: per case and step action, prev_action, processed, prev_applied [n][cols] and cmd [n][joints] after the
// process step, then action, prev_action, prev_applied after the reset (float32).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../allsteps_isaaclab_amd/csrc/allsteps_actions.h"

static_assert(sizeof(as_action_column_t) == 12 * sizeof(uint32_t), "as_action_column_t is 12 words");

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

int main(int argc, char** argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: actions_check cases.bin dump.bin\n");
    return 2;
  }
  FILE* in = fopen(argv[1], "rb");
  FILE* out = fopen(argv[2], "wb");
  if (!in || !out) return 2;
  const int cases = take<int32_t>(in, 1)[0];
  long items = 0, resets = 0;
  for (int c = 0; c < cases; ++c) {
    const std::vector<int32_t> h = take<int32_t>(in, 4);
    const size_t n = (size_t)h[0], D = (size_t)h[1], J = (size_t)h[2];
    const int steps = h[3];
    const auto cols = take<as_action_column_t>(in, D);
    std::vector<float> action(n * D, 0.0f), prev_action(n * D, 0.0f), processed(n * D, 0.0f),
        prev_applied(n * D, 0.0f), cmd(n * J, 0.0f);
    for (int s = 0; s < steps; ++s) {
      const auto raw = take<float>(in, n * D), q = take<float>(in, J * n);
      const int reset = take<int32_t>(in, 1)[0];
      const auto mask = take<uint8_t>(in, n);
      for (size_t e = 0; e < n; ++e)
        for (size_t k = 0; k < D; ++k) {
          as::actions_process_one(cols[k], e * D + k, e, (int32_t)J, raw.data(), action.data(), prev_action.data(),
                                  processed.data(), prev_applied.data(), cmd.data());
          ++items;
        }
      put(out, action);
      put(out, prev_action);
      put(out, processed);
      put(out, prev_applied);
      put(out, cmd);
      for (size_t e = 0; e < n && reset; ++e) {
        if (reset == 1 && !mask[e]) continue;
        for (size_t k = 0; k < D; ++k)
          as::actions_reset_one(cols[k], e * D + k, e, n, (int32_t)J, q.data(), action.data(), prev_action.data(),
                                prev_applied.data());
        ++resets;
      }
      put(out, action);
      put(out, prev_action);
      put(out, prev_applied);
    }
  }
  fclose(in);
  fclose(out);
  printf("actions fixture: %d cases, %ld (env, column) items, %ld env resets\n", cases, items, resets);
  return 0;
}
