// contact_timers_check.cpp -- stand-alone host check of csrc/allsteps_contact_timers.h
// (tests/test_contact_timers_host.py builds and runs it, plain and under -fsanitize=address,undefined).
//
//   contact_timers_check <cases.bin>
//
// cases.bin (written by the test from tests/golden/contact_timers.npz, native endianness, 4-byte words):
//   int32 ncases, then per case
//     int32 n, bodies, updates, stride;  float dt, threshold
//     float impulses[updates][bodies][3][n];  int32 resets[updates][n]  (the envs reset after that update)
//     float timers_expect[updates / stride][4][bodies][n], timestamp_expect[updates / stride][n]
//   -- the reference's ContactSensor run on the forces impulse / dt.  The program is fed the IMPULSES: it goes
//   through the header's whole path, the division included (the fixture's generator keeps impulses whose float32
//   quotient by dt is the force the reference saw).  It replays a case the way k_contact_timers does -- per env:
//   timers_tick on the timestamp, a ReportEnv holding one record per body (a stone contact on link = body, and
//   on top a self-contact whose second link is the body, carrying the negated impulse, for odd bodies),
//   report_body_sum, timers_update_impulse, timers_reset -- on buffers laid out as the device's (timers_index),
//   and demands every timer and timestamp bit for bit.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../allsteps_isaaclab_amd/csrc/allsteps_contact_timers.h"

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

int check_cases(Reader& r) {
  const int32_t ncases = r.one<int32_t>();
  int bad = 0;
  long checked = 0, contacts = 0, resets_done = 0;
  for (int c = 0; c < ncases && r.ok; ++c) {
    const int32_t n = r.one<int32_t>(), nb = r.one<int32_t>(), updates = r.one<int32_t>(), stride = r.one<int32_t>();
    const float dt = r.one<float>(), threshold = r.one<float>();
    if (!r.ok || n < 1 || nb < 1 || nb > as::kRepMaxC || updates < 1 || stride < 1 || updates % stride) {
      printf("case %d: bad header\n", c);
      return bad + 1;
    }
    const std::vector<float> imp = r.many<float>((size_t)updates * nb * 3 * n);
    const std::vector<int32_t> resets = r.many<int32_t>((size_t)updates * n);
    const size_t records = (size_t)(updates / stride);
    const std::vector<float> want_t = r.many<float>(records * as::kTimerRows * nb * n);
    const std::vector<float> want_ts = r.many<float>(records * n);
    if (!r.ok) break;
    std::vector<float> timers((size_t)as::kTimerRows * nb * n, 0.f), ts((size_t)n, 0.f);
    int case_bad = 0;
    for (int u = 0; u < updates; ++u) {
      for (int e = 0; e < n; ++e) {
        // the env's records of this update: body b's impulse on link b; an odd body gets it as the second link
        // of a self-contact with link b + nb (which no body of the table carries), negated
        as::ReportEnv rep{};
        rep.count = nb;
        for (int b = 0; b < nb; ++b) {
          const bool self = b & 1;
          for (int k = 0; k < 3; ++k) {
            const float v = imp[(((size_t)u * nb + b) * 3 + k) * n + e];
            rep.imp[b][k] = self ? -v : v;
          }
          rep.ids[b] = self ? as::report_pack_ids(b + nb, b, -1, -1) : as::report_pack_ids(b, -1, 0, b);
        }
        const float elapsed = as::timers_tick(&ts[e], dt);
        for (int b = 0; b < nb; ++b) {
          as::ContactTimers t{timers[as::timers_index(as::kTimerCurrentAir, b, e, n, nb)],
                              timers[as::timers_index(as::kTimerLastAir, b, e, n, nb)],
                              timers[as::timers_index(as::kTimerCurrentContact, b, e, n, nb)],
                              timers[as::timers_index(as::kTimerLastContact, b, e, n, nb)]};
          float net[3];
          as::report_body_sum(rep, b, net);
          for (int k = 0; k < 3; ++k)  // 0 - (-v) = v, 0 + v = v: the sum hands the impulse through, as bits
            case_bad += bits(net[k]) != bits(imp[(((size_t)u * nb + b) * 3 + k) * n + e] + 0.f);
          as::timers_update_impulse(t, net, dt, threshold, elapsed);
          contacts += t.current_contact > 0.f;
          if (resets[(size_t)u * n + e]) as::timers_reset(t);
          timers[as::timers_index(as::kTimerCurrentAir, b, e, n, nb)] = t.current_air;
          timers[as::timers_index(as::kTimerLastAir, b, e, n, nb)] = t.last_air;
          timers[as::timers_index(as::kTimerCurrentContact, b, e, n, nb)] = t.current_contact;
          timers[as::timers_index(as::kTimerLastContact, b, e, n, nb)] = t.last_contact;
        }
        if (resets[(size_t)u * n + e]) {
          ts[e] = 0.f;
          ++resets_done;
        }
      }
      if ((u + 1) % stride) continue;
      const size_t rec = (size_t)((u + 1) / stride - 1);
      for (size_t i = 0; i < timers.size(); ++i) case_bad += bits(timers[i]) != bits(want_t[rec * timers.size() + i]);
      for (int e = 0; e < n; ++e) case_bad += bits(ts[e]) != bits(want_ts[rec * n + e]);
      checked += (long)timers.size() + n;
    }
    printf("case %d: n %d bodies %d updates %d stride %d threshold %g: %d mismatches\n", c, (int)n, (int)nb,
           (int)updates, (int)stride, (double)threshold, case_bad);
    bad += case_bad;
  }
  if (!r.ok) {
    printf("cases.bin: short read\n");
    return bad + 1;
  }
  printf("contact timers fixture: %d cases, %ld values, %ld updates in contact, %ld resets, %d mismatches\n",
         (int)ncases, checked, contacts, resets_done, bad);
  return bad;
}

// the layout helpers: timers_index is row-major [row][body][env], and the rows are in the documented order
int check_layout() {
  int bad = 0;
  const int n = 7, nb = 3;
  size_t next = 0;
  for (int row = 0; row < as::kTimerRows; ++row)
    for (int b = 0; b < nb; ++b)
      for (int e = 0; e < n; ++e) bad += as::timers_index(row, b, e, n, nb) != next++;
  bad += !(as::kTimerCurrentAir == 0 && as::kTimerLastAir == 1 && as::kTimerCurrentContact == 2 &&
           as::kTimerLastContact == 3 && as::kTimerRows == 4);
  // elapsed is the difference of the timestamps: at a large timestamp it is not dt
  float ts = 14.5f;
  const float dt = 1.f / 240.f;
  const float elapsed = as::timers_tick(&ts, dt);
  bad += !(bits(elapsed) != bits(dt) && bits(ts) == bits(14.5f + dt));
  printf("layout and elapsed time: %d mismatches\n", bad);
  return bad;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 2) {
    fprintf(stderr, "usage: %s <cases.bin>\n", argv[0]);
    return 2;
  }
  FILE* f = fopen(argv[1], "rb");
  if (!f) {
    fprintf(stderr, "cannot open %s\n", argv[1]);
    return 2;
  }
  Reader r{f};
  int bad = check_cases(r);
  fclose(f);
  bad += check_layout();
  return bad ? 1 : 0;
}
