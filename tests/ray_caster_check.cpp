// ray_caster_check.cpp -- stand-alone host run of csrc/allsteps_ray_caster.h
// (tests/test_ray_caster_host.py builds and runs it, plain and under -fsanitize=address,undefined).
//
//   ray_caster_check <cases.bin> <out.bin>
//
// cases.bin (written by tests/_ray_caster_cases.py, native endianness, 4-byte words):
//   int32 ncases, then per case
//     int32 n, R, attach_yaw_only, surfaces, num_steps;  float max_distance, ground_z, half[3]
//     float rays[6][R], root_pos[3][n], root_quat[4][n], stones[60][n]          (the device layouts)
// out.bin, per case:
//     float hits[3][R][n];  int8 surface[R][n];  float pose[7][n];  float starts_w[3][R][n], dirs_w[3][R][n]
// The program replays a case the way k_ray_cast does -- per env: the pose and the stones gathered from the
// env-minor rows, ray_frame once, then per ray ray_world, ray_inverse, the ground, the stones in order,
// ray_hit_point -- on buffers laid out as the device's (ray_hit_index, ray_surface_index), and checks that
// ray_cast_one, the header's one-call form, gives the same bits.  The comparison with the fixtures is the test's.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../allsteps_isaaclab_amd/csrc/allsteps_ray_caster.h"

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

uint32_t bits(float x) {
  uint32_t u;
  std::memcpy(&u, &x, sizeof u);
  return u;
}

int run_cases(Reader& r, FILE* out) {
  const int32_t ncases = r.one<int32_t>();
  int bad = 0;
  long rays_done = 0, stone_hits = 0, ground_hits = 0, misses = 0;
  for (int c = 0; c < ncases && r.ok; ++c) {
    const int32_t n = r.one<int32_t>(), R = r.one<int32_t>(), yaw = r.one<int32_t>(), surfaces = r.one<int32_t>(),
                  ns = r.one<int32_t>();
    const float max_distance = r.one<float>(), ground_z = r.one<float>();
    const float half[3] = {r.one<float>(), r.one<float>(), r.one<float>()};
    if (!r.ok || n < 1 || R < 1 || ns < 0 || ns > AS_NUM_STONES) {
      printf("case %d: bad header\n", c);
      return bad + 1;
    }
    const std::vector<float> rays = r.many<float>((size_t)6 * R), root_pos = r.many<float>((size_t)3 * n),
                             root_quat = r.many<float>((size_t)4 * n),
                             stones = r.many<float>((size_t)3 * AS_NUM_STONES * n);
    if (!r.ok) break;
    std::vector<float> hits((size_t)3 * R * n), pose((size_t)as::kRayPoseRows * n), starts((size_t)3 * R * n),
        dirs((size_t)3 * R * n);
    std::vector<int8_t> surface((size_t)R * n);
    int case_bad = 0;
    for (int e = 0; e < n; ++e) {
      float pos[3], q[4], st[3 * AS_NUM_STONES], qf[4];
      for (int k = 0; k < 3; ++k) pos[k] = pose[(size_t)k * n + e] = root_pos[(size_t)k * n + e];
      for (int k = 0; k < 4; ++k) q[k] = pose[(size_t)(3 + k) * n + e] = root_quat[(size_t)k * n + e];
      for (int k = 0; k < 3 * AS_NUM_STONES; ++k) st[k] = stones[(size_t)k * n + e];
      as::ray_frame(q, yaw != 0, qf);
      for (int ray = 0; ray < R; ++ray) {
        float start_l[3], dir_l[3], o[3], d[3], inv[3], hit[3], hit1[3];
        for (int k = 0; k < 3; ++k) {
          start_l[k] = rays[as::ray_local_index(k, ray, R)];
          dir_l[k] = rays[as::ray_local_index(3 + k, ray, R)];
        }
        as::ray_world(pos, qf, yaw != 0, start_l, dir_l, o, d);
        as::ray_inverse(d, inv);
        as::RayBest b;
        as::ray_begin(b);
        if (surfaces & as::kRaySurfGround) as::ray_ground(b, o, d, inv, ground_z, max_distance);
        if (surfaces & as::kRaySurfStones)
          for (int s = 0; s < ns; ++s) {
            const float ctr[3] = {st[3 * s], st[3 * s + 1], st[3 * s + 2]};
            as::ray_stone(b, o, d, inv, ctr, half, max_distance, s);
          }
        as::ray_hit_point(b, o, d, hit);
        const int s1 = as::ray_cast_one(pos, qf, yaw != 0, surfaces, start_l, dir_l, st, ns, half, ground_z,
                                        max_distance, hit1);
        case_bad += s1 != b.surface;
        for (int k = 0; k < 3; ++k) {
          case_bad += bits(hit[k]) != bits(hit1[k]);
          hits[as::ray_hit_index(k, ray, e, n, R)] = hit[k];
          starts[as::ray_hit_index(k, ray, e, n, R)] = o[k];
          dirs[as::ray_hit_index(k, ray, e, n, R)] = d[k];
        }
        surface[as::ray_surface_index(ray, e, n)] = (int8_t)b.surface;
        ++rays_done;
        stone_hits += b.surface >= 0;
        ground_hits += b.surface == as::kRayHitGround;
        misses += b.surface == as::kRayMiss;
      }
    }
    if (!(put(out, hits) && put(out, surface) && put(out, pose) && put(out, starts) && put(out, dirs))) {
      printf("case %d: short write\n", c);
      return bad + 1;
    }
    printf("case %d: n %d rays %d yaw_only %d surfaces %d: %d mismatches\n", c, (int)n, (int)R, (int)yaw,
           (int)surfaces, case_bad);
    bad += case_bad;
  }
  if (!r.ok) {
    printf("cases.bin: short read\n");
    return bad + 1;
  }
  printf("ray caster: %d cases, %ld rays, %ld stone hits, %ld ground hits, %ld misses, %d mismatches\n", (int)ncases,
         rays_done, stone_hits, ground_hits, misses, bad);
  return bad;
}

// the layout helpers are row-major [k][ray][env] / [ray][env], and the surface codes are the documented ones
int check_layout() {
  int bad = 0;
  const int n = 7, R = 5;
  size_t next = 0;
  for (int k = 0; k < 3; ++k)
    for (int ray = 0; ray < R; ++ray)
      for (int e = 0; e < n; ++e) bad += as::ray_hit_index(k, ray, e, n, R) != next++;
  next = 0;
  for (int ray = 0; ray < R; ++ray)
    for (int e = 0; e < n; ++e) bad += as::ray_surface_index(ray, e, n) != next++;
  bad += !(as::kRayHitGround == AS_RAY_HIT_GROUND && as::kRayMiss == AS_RAY_MISS && as::kRaySurfGround == AS_RAY_GROUND &&
           as::kRaySurfStones == AS_RAY_STONES && as::kRayPoseRows == 7);
  printf("layout and codes: %d mismatches\n", bad);
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
