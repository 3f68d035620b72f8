// rewards_check.cpp -- a stand-alone program around csrc/allsteps_rewards.h (tests/test_rewards_host.py builds it
// once plain and once with -fsanitize=address,undefined and runs it directly).
//
//   rewards_check cases.bin dump.bin
//
// cases.bin (little endian, written by the test from tests/golden/rewards.npz and the tables envs/rewards.py makes):
//   int32 cases; per case: int32 n, terms, steps, actions, joint_rows, depth, bodies, timer_bodies, command_rows,
//   clamp; float32 dt, sim_dt; per step: the descriptor rows [terms][8], the index table [3][32][32], root_pos [3][n],
//   root_quat [4][n], root_lin [3][n], root_ang [3][n], q, qd, qd_prev [joint_rows][n], commands [command_rows][n],
//   net [depth][bodies][3][n], timers [4][timer_bodies][n], actions [n][actions], terminated [n] uint8, done [n] uint8.
// dump.bin: per case and step f [terms][n] (every term's value, whatever its weight), reward [n], episode_sums,
// step_reward, last_episode_sums [terms][n], prev_actions [n][actions], after the step.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../allsteps_isaaclab_amd/csrc/allsteps_rewards.h"

static_assert(sizeof(as_reward_term_t) == 8 * sizeof(uint32_t), "as_reward_term_t is 8 words");

template <typename T>
static std::vector<T> take(FILE* f, size_t count) {
  std::vector<T> v(count);
  if (count && fread(v.data(), sizeof(T), count, f) != count) {
    fprintf(stderr, "cases file is truncated\n");
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
    fprintf(stderr, "usage: rewards_check cases.bin dump.bin\n");
    return 2;
  }
  FILE* in = fopen(argv[1], "rb");
  FILE* out = fopen(argv[2], "wb");
  if (!in || !out) return 2;
  const int cases = take<int32_t>(in, 1)[0];
  long items = 0, skipped = 0, done_envs = 0;
  for (int c = 0; c < cases; ++c) {
    const std::vector<int32_t> h = take<int32_t>(in, 10);
    const std::vector<float> dts = take<float>(in, 2);
    const size_t n = (size_t)h[0], T = (size_t)h[1], A = (size_t)h[3];
    const int steps = h[2];
    std::vector<float> reward(n), sums(T * n), step(T * n), last(T * n), prev(n * A), fv(T * n);
    for (int s = 0; s < steps; ++s) {
      const auto desc = take<as_reward_term_t>(in, T);
      const auto table = take<uint32_t>(in, (size_t)AS_REW_TABLE_ROWS * AS_MAX_REW_TERMS * AS_MAX_REW_IDS);
      const auto root_pos = take<float>(in, 3 * n), root_quat = take<float>(in, 4 * n);
      const auto root_lin = take<float>(in, 3 * n), root_ang = take<float>(in, 3 * n);
      const auto q = take<float>(in, (size_t)h[4] * n), qd = take<float>(in, (size_t)h[4] * n);
      const auto qd_prev = take<float>(in, (size_t)h[4] * n);
      const auto commands = take<float>(in, (size_t)h[8] * n);
      const auto net = take<float>(in, (size_t)h[5] * h[6] * 3 * n);
      const auto timers = take<float>(in, (size_t)4 * h[7] * n);
      const auto actions = take<float>(in, n * A);
      const auto terminated = take<uint8_t>(in, n), done = take<uint8_t>(in, n);
      as_reward_sources_t S{};
      S.root_pos = root_pos.data();
      S.root_quat = root_quat.data();
      S.root_lin = root_lin.data();
      S.root_ang = root_ang.data();
      S.q = q.data();
      S.qd = qd.data();
      S.qd_prev = qd_prev.data();
      S.commands = commands.data();
      S.net = net.data();
      S.timers = timers.data();
      S.actions = actions.data();
      S.terminated = terminated.data();
      S.joint_rows = S.qd_prev_rows = h[4];
      S.depth = h[5];
      S.bodies = h[6];
      S.timer_bodies = h[7];
      S.command_rows = h[8];
      S.action_cols = h[3];
      S.clamp_actions = h[9];
      S.sim_dt = dts[1];
      for (size_t e = 0; e < n; ++e) {
        const as::RewardEnv E{&S, n, e};
        for (size_t k = 0; k < T; ++k) {
          const int32_t* ids = reinterpret_cast<const int32_t*>(&table[as::rew_table_at(as::kRewTabId, (int)k, 0)]);
          const float* ca = reinterpret_cast<const float*>(&table[as::rew_table_at(as::kRewTabA, (int)k, 0)]);
          const float* cb = reinterpret_cast<const float*>(&table[as::rew_table_at(as::kRewTabB, (int)k, 0)]);
          fv[k * n + e] = as::reward_term_value(desc[k], ids, ca, cb, E, &prev[e * A]);
          ++items;
          skipped += desc[k].weight == 0.0f;
        }
        done_envs += done[e] != 0;
        as::rewards_env_step(desc.data(), (int)T, table.data(), S, n, e, done[e] != 0, dts[0], reward.data(),
                             sums.data(), step.data(), last.data(), prev.data());
      }
      put(out, fv);
      put(out, reward);
      put(out, sums);
      put(out, step);
      put(out, last);
      put(out, prev);
    }
  }
  fclose(in);
  fclose(out);
  printf("rewards fixture: %d cases, %ld (term, env) items, %ld skipped at weight 0, %ld done envs\n", cases, items,
         skipped, done_envs);
  return 0;
}
