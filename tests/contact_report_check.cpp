// Stand-alone check of csrc/allsteps_contact_report.h: the ids packing, the buffer indices and the per-env
// reductions k_contact_forces runs (report_load_env, report_pair_sum, report_body_sum), against a
// straightforward restatement that walks the records in a different way (per record, scattering into dense
// arrays kept per key).  Because every key's terms are still met in ascending slot order, and a sum that
// starts at +0 is unchanged by the +0 terms the header adds for the other keys, the results must agree in
// bits.  tests/test_contact_report_host.py builds it plain and with -fsanitize=address,undefined.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../allsteps_isaaclab_amd/csrc/allsteps_contact_report.h"

namespace {

struct Rec {
  float imp[3], pt[3], sep;
  int link, link2, stone, foot;
};

uint32_t bits(float f) {
  uint32_t u;
  std::memcpy(&u, &f, 4);
  return u;
}

uint64_t g_rng = 0x9E3779B97F4A7C15ull;
uint32_t rnd() {
  g_rng ^= g_rng << 13;
  g_rng ^= g_rng >> 7;
  g_rng ^= g_rng << 17;
  return (uint32_t)(g_rng >> 32);
}
float rndf() { return ((int)(rnd() % 20001) - 10000) * 1.37e-4f; }

int g_bad = 0, g_cases = 0;

// One case: `depth` slots of `n` envs; env `e_t` of slot `s_t` holds `recs`, every other env random filler, so a
// wrong index reads another env's data.  `links`: the body table.
void run_case(const char* name, const std::vector<Rec>& recs, const std::vector<int>& links) {
  const int n = 5, depth = 3, e_t = 3, s_t = 1;
  std::vector<int32_t> count(as::report_count_words(depth, n));
  std::vector<uint32_t> records(as::report_record_words(depth, n));
  for (auto& w : records) w = rnd();
  for (auto& c : count) c = (int32_t)(rnd() % (as::kRepMaxC + 1));
  count[as::report_count_index(s_t, e_t, n)] = (int32_t)recs.size();
  for (int c = 0; c < as::kRepMaxC; ++c) {
    Rec r{};
    r.link2 = r.stone = r.foot = -1;
    const bool live = c < (int)recs.size();
    if (live) r = recs[c];
    const uint32_t w[as::kRepWords] = {bits(r.imp[0]), bits(r.imp[1]), bits(r.imp[2]), bits(r.pt[0]),
                                       bits(r.pt[1]),  bits(r.pt[2]),  bits(r.sep),
                                       as::report_pack_ids(r.link, r.link2, r.stone, r.foot)};
    for (int k = 0; k < as::kRepWords; ++k) records[as::report_record_index(s_t, k, c, e_t, n)] = live ? w[k] : 0u;
    if (live) {  // the ids survive the packing
      int l, l2, st, f;
      as::report_unpack_ids(w[as::kRepIds], l, l2, st, f);
      if (l != r.link || l2 != r.link2 || st != r.stone || f != r.foot) {
        std::printf("%s: ids (%d %d %d %d) unpacked as (%d %d %d %d)\n", name, r.link, r.link2, r.stone, r.foot, l, l2,
                    st, f);
        ++g_bad;
      }
    }
  }
  // restatement: scatter record by record
  float fm[as::kRepFeet][AS_NUM_STONES][3] = {};
  std::vector<float> net(3 * links.size(), 0.f);
  for (const Rec& r : recs) {
    if (r.foot >= 0 && r.stone >= 0)
      for (int k = 0; k < 3; ++k) fm[r.foot][r.stone][k] += r.imp[k];
    for (size_t b = 0; b < links.size(); ++b)
      for (int k = 0; k < 3; ++k) {
        if (links[b] == r.link) net[3 * b + k] += r.imp[k];
        if (links[b] == r.link2) net[3 * b + k] -= r.imp[k];
      }
  }
  as::ReportEnv env;
  as::report_load_env(count.data(), records.data(), s_t, e_t, n, env);
  if (env.count != (int)recs.size()) {
    std::printf("%s: count %d, expected %zu\n", name, env.count, recs.size());
    ++g_bad;
  }
  for (int f = 0; f < as::kRepFeet; ++f)
    for (int st = 0; st < AS_NUM_STONES; ++st) {
      float v[3];
      as::report_pair_sum(env, f, st, v);
      for (int k = 0; k < 3; ++k)
        if (bits(v[k]) != bits(fm[f][st][k])) {
          std::printf("%s: force matrix (%d, %d, %d) %.9g, expected %.9g\n", name, f, st, k, v[k], fm[f][st][k]);
          ++g_bad;
        }
    }
  for (size_t b = 0; b < links.size(); ++b) {
    float v[3];
    as::report_body_sum(env, links[b], v);
    for (int k = 0; k < 3; ++k)
      if (bits(v[k]) != bits(net[3 * b + k])) {
        std::printf("%s: net (%zu, %d) %.9g, expected %.9g\n", name, b, k, v[k], net[3 * b + k]);
        ++g_bad;
      }
  }
  ++g_cases;
}

Rec make(int link, int link2, int stone, int foot) {
  Rec r;
  for (int k = 0; k < 3; ++k) {
    r.imp[k] = rndf();
    r.pt[k] = rndf();
  }
  r.sep = rndf();
  r.link = link;
  r.link2 = link2;
  r.stone = stone;
  r.foot = foot;
  return r;
}

}  // namespace

int main() {
  std::vector<int> links;  // a walker-like table: body b on link b, 17 bodies
  for (int b = 0; b < 17; ++b) links.push_back(b);
  run_case("zero contacts", {}, links);
  {
    std::vector<Rec> r;  // MAXC contacts, every one its own key
    for (int c = 0; c < as::kRepMaxC; ++c) r.push_back(make(5 + c % 2, -1, c, c % 2));
    run_case("MAXC contacts", r, links);
  }
  {
    std::vector<Rec> r;  // repeated keys, interleaved with another key and with a non-sensor geom on the stone
    for (int c = 0; c < as::kRepMaxC; ++c) r.push_back(make(c % 3 == 2 ? 4 : 5, -1, 7, c % 3 == 2 ? -1 : c % 3));
    run_case("repeated keys", r, links);
  }
  {
    std::vector<Rec> r;  // self-contacts only: both links are bodies, one pair twice
    r.push_back(make(3, 9, -1, -1));
    r.push_back(make(9, 12, -1, -1));
    r.push_back(make(3, 9, -1, -1));
    run_case("self-contacts", r, links);
  }
  {
    std::vector<Rec> r;  // foot = -1 on a stone: in no force-matrix entry, in its body's net impulse
    r.push_back(make(2, -1, 0, -1));
    r.push_back(make(2, -1, 19, -1));
    r.push_back(make(6, -1, 19, 3));
    run_case("foot = -1", r, links);
  }
  {
    std::vector<Rec> r;  // a sensor foot's link as the second link of a self-contact, beside its stone contacts
    r.push_back(make(6, -1, 4, 0));
    r.push_back(make(2, 6, -1, -1));
    r.push_back(make(6, -1, 4, 0));
    r.push_back(make(0, 6, -1, -1));
    run_case("link2 is a body's link", r, links);
  }
  {
    std::vector<int> sparse = {0, 6, 31};  // a table that leaves links out, and the largest ids a byte field holds
    std::vector<Rec> r;
    r.push_back(make(31, 6, -1, -1));
    r.push_back(make(31, -1, AS_NUM_STONES - 1, as::kRepFeet - 1));
    r.push_back(make(4, 5, -1, -1));
    run_case("sparse body table, largest ids", r, sparse);
  }
  for (int t = 0; t < 2000; ++t) {  // random mixes
    std::vector<Rec> r;
    const int cnt = (int)(rnd() % (as::kRepMaxC + 1));
    for (int c = 0; c < cnt; ++c) {
      const int kind = (int)(rnd() % 3);
      if (kind == 0) r.push_back(make((int)(rnd() % 17), -1, (int)(rnd() % 4), (int)(rnd() % 3) - 1));
      else if (kind == 1) r.push_back(make((int)(rnd() % 8), 8 + (int)(rnd() % 9), -1, -1));
      else r.push_back(make(6, -1, 3, 1));
    }
    run_case("random", r, links);
  }
  std::printf("contact report: %d cases, %d mismatches\n", g_cases, g_bad);
  return g_bad != 0;
}
