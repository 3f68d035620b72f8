// imu_check.cpp -- stand-alone host run of csrc/allsteps_imu.h
// (tests/test_imu_host.py builds and runs it, plain and under -fsanitize=address,undefined).
//
//   imu_check <cases.bin> <out.bin>
//
// cases.bin (written by tests/_imu_cases.py, native endianness):
//   int32 ncases, then per case
//     int32 n, U, R;  float dt, offset_pos[3], offset_rot[4], com[3], gravity_bias[3]
//     float pose[U][7][n], vel[U][6][n];  int32 upd[R];  uint8 mask[R][n]
// out.bin, per case:
//     float data[R][19][n], prev[R][6][n]     the buffers after every record
// The program replays a case the way k_imu does, one sensor (S = 1) on buffers laid out as the device's
// (imu_index): per record the outdated flags are the record's mask; an outdated env gathers its pose, velocities
// and prev from the env-minor rows, runs imu_update, scatters data and prev and clears its flag; the others are
// not touched.  The comparison with the fixture and the NumPy restatement is the test's.
#include <cstdio>
#include <vector>

#include "../allsteps_isaaclab_amd/csrc/allsteps_imu.h"

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

template <typename T>
bool put(FILE* f, const std::vector<T>& v) {
  return v.empty() || fwrite(v.data(), sizeof(T), v.size(), f) == v.size();
}

int run_cases(Reader& r, FILE* out) {
  const int32_t ncases = r.one<int32_t>();
  long updates_done = 0, kept = 0;
  for (int c = 0; c < ncases && r.ok; ++c) {
    const int32_t n = r.one<int32_t>(), U = r.one<int32_t>(), R = r.one<int32_t>();
    const float dt = r.one<float>();
    as::ImuConst K;
    for (float& x : K.o) x = r.one<float>();
    for (float& x : K.r) x = r.one<float>();
    for (float& x : K.c) x = r.one<float>();
    for (float& x : K.g) x = r.one<float>();
    if (!r.ok || n < 1 || U < 1 || R < 1 || !(dt > 0.f)) {
      printf("case %d: bad header\n", c);
      return 1;
    }
    const std::vector<float> pose = r.many<float>((size_t)U * 7 * n), vel = r.many<float>((size_t)U * 6 * n);
    const std::vector<int32_t> upd = r.many<int32_t>((size_t)R);
    const std::vector<uint8_t> mask = r.many<uint8_t>((size_t)R * n);
    if (!r.ok) break;
    const int S = 1, s = 0;
    std::vector<float> data((size_t)as::kImuDataRows * S * n, 0.f), prev((size_t)as::kImuPrevRows * S * n, 0.f);
    std::vector<uint8_t> outdated((size_t)n, 1);
    std::vector<float> all_data, all_prev;
    for (int e = 0; e < n; ++e) data[as::imu_index(as::kImuQuat, s, e, n, S)] = 1.f;  // quat_w = identity at first
    for (int rec = 0; rec < R; ++rec) {
      const int u = upd[rec];
      if (u < 0 || u >= U) {
        printf("case %d: record %d names update %d\n", c, rec, u);
        return 1;
      }
      for (int e = 0; e < n; ++e) outdated[e] = mask[(size_t)rec * n + e];
      const float* ps = &pose[(size_t)u * 7 * n];
      const float* vl = &vel[(size_t)u * 6 * n];
      for (int e = 0; e < n; ++e) {
        if (!outdated[e]) {
          ++kept;
          continue;
        }
        const float p[3] = {ps[0 * n + e], ps[1 * n + e], ps[2 * n + e]};
        const float q[4] = {ps[3 * n + e], ps[4 * n + e], ps[5 * n + e], ps[6 * n + e]};
        const float v[3] = {vl[0 * n + e], vl[1 * n + e], vl[2 * n + e]};
        const float w[3] = {vl[3 * n + e], vl[4 * n + e], vl[5 * n + e]};
        float pv[as::kImuPrevRows], d[as::kImuDataRows];
        for (int k = 0; k < as::kImuPrevRows; ++k) pv[k] = prev[as::imu_index(k, s, e, n, S)];
        as::imu_update(p, q, v, w, K, dt, pv, d);
        for (int k = 0; k < as::kImuDataRows; ++k) data[as::imu_index(k, s, e, n, S)] = d[k];
        for (int k = 0; k < as::kImuPrevRows; ++k) prev[as::imu_index(k, s, e, n, S)] = pv[k];
        outdated[e] = 0;
        ++updates_done;
      }
      all_data.insert(all_data.end(), data.begin(), data.end());
      all_prev.insert(all_prev.end(), prev.begin(), prev.end());
    }
    if (!(put(out, all_data) && put(out, all_prev))) {
      printf("case %d: short write\n", c);
      return 1;
    }
    printf("case %d: n %d updates %d records %d\n", c, (int)n, (int)U, (int)R);
  }
  if (!r.ok) {
    printf("cases.bin: short read\n");
    return 1;
  }
  printf("imu: %d cases, %ld env updates, %ld env records kept\n", (int)ncases, updates_done, kept);
  return 0;
}

// the layout helper is row-major [row][sensor][env] and the row constants are the documented ones
int check_layout() {
  int bad = 0;
  const int n = 7, S = 3;
  size_t next = 0;
  for (int row = 0; row < as::kImuDataRows; ++row)
    for (int s = 0; s < S; ++s)
      for (int e = 0; e < n; ++e) bad += as::imu_index(row, s, e, n, S) != next++;
  bad += !(as::kImuPos == 0 && as::kImuQuat == 3 && as::kImuLinVel == 7 && as::kImuAngVel == 10 && as::kImuLinAcc == 13 &&
           as::kImuAngAcc == 16 && as::kImuDataRows == 19 && as::kImuPrevLin == 0 && as::kImuPrevAng == 3 &&
           as::kImuPrevRows == 6);
  printf("layout and rows: %d mismatches\n", bad);
  return bad;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: %s <cases.bin> <out.bin>\n", argv[0]);
    return 2;
  }
  FILE* f = fopen(argv[1], "rb");
  FILE* out = fopen(argv[2], "wb");
  if (!f || !out) {
    fprintf(stderr, "cannot open %s / %s\n", argv[1], argv[2]);
    if (f) fclose(f);
    if (out) fclose(out);
    return 2;
  }
  Reader r{f};
  int bad = run_cases(r, out);
  fclose(f);
  if (fclose(out) != 0) ++bad;
  bad += check_layout();
  return bad ? 1 : 0;
}
