// ray_camera_check.cpp -- stand-alone host run of csrc/allsteps_ray_camera.h
// (tests/test_ray_camera_host.py builds and runs it, plain and under -fsanitize=address,undefined).
//
//   ray_camera_check <cases.bin> <out.bin>
//
// cases.bin (written by tests/_ray_camera_cases.py, native endianness, 4-byte words):
//   int32 ncases, then per case
//     int32 n, width, height, surfaces, clipping, num_steps;  float max_distance, ground_z, half[3]
//     float dirs[3][R], offset[7][n], root_pos[3][n], root_quat[4][n], stones[60][n]    (the device layouts)
// out.bin, per case:
//     float pose[7][n], plane[n][R], camera[n][R], normals[n][R][3], dirs_w[n][R][3], t[n][R];  int32 surface[n][R]
// The program replays a case the way k_ray_camera does -- per env: the pose, the offset and cam_frame once, then per
// pixel quat_apply, ray_inverse, the ground, the stones in order read from the env-minor rows, the two distances and
// the normal from the re-read centre of the stone hit -- on buffers laid out as the device's, and checks that
// cam_pixel_one, the header's one-call form, gives the same bits.  The comparison with the fixtures is the test's.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../allsteps_isaaclab_amd/csrc/allsteps_ray_camera.h"

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
  long pixels = 0, stone_hits = 0, ground_hits = 0, misses = 0;
  for (int c = 0; c < ncases && r.ok; ++c) {
    const int32_t n = r.one<int32_t>(), W = r.one<int32_t>(), H = r.one<int32_t>(), surfaces = r.one<int32_t>(),
                  clipping = r.one<int32_t>(), ns = r.one<int32_t>();
    const float max_distance = r.one<float>(), ground_z = r.one<float>();
    const float half[3] = {r.one<float>(), r.one<float>(), r.one<float>()};
    if (!r.ok || n < 1 || W < 1 || H < 1 || (long)W * H > AS_MAX_CAMERA_RAYS || ns < 0 || ns > AS_NUM_STONES) {
      printf("case %d: bad header\n", c);
      return bad + 1;
    }
    const int R = W * H;
    const std::vector<float> dirs = r.many<float>((size_t)3 * R), offset = r.many<float>((size_t)7 * n),
                             root_pos = r.many<float>((size_t)3 * n), root_quat = r.many<float>((size_t)4 * n),
                             stones = r.many<float>((size_t)3 * AS_NUM_STONES * n);
    if (!r.ok) break;
    std::vector<float> pose((size_t)as::kCamPoseRows * n), plane((size_t)n * R), camera((size_t)n * R),
        normals((size_t)n * R * 3), dirs_w((size_t)n * R * 3), ts((size_t)n * R);
    std::vector<int32_t> surface((size_t)n * R);
    int case_bad = 0;
    for (int e = 0; e < n; ++e) {
      float rp[3], rq[4], op[3], oq[4];
      for (int k = 0; k < 3; ++k) rp[k] = root_pos[(size_t)k * n + e];
      for (int k = 0; k < 4; ++k) rq[k] = root_quat[(size_t)k * n + e];
      for (int k = 0; k < 3; ++k) op[k] = offset[(size_t)k * n + e];
      for (int k = 0; k < 4; ++k) oq[k] = offset[(size_t)(3 + k) * n + e];
      as::CamFrame f;
      as::cam_frame(rp, rq, op, oq, f);
      for (int k = 0; k < 3; ++k) pose[(size_t)k * n + e] = f.pos[k];
      for (int k = 0; k < 4; ++k) pose[(size_t)(3 + k) * n + e] = f.quat[k];
      const float* st = stones.data() + e;  // coordinate k of stone s at st[(3 s + k) n]
      for (int p = 0; p < R; ++p) {
        const float dir_l[3] = {dirs[as::cam_dir_index(0, p, R)], dirs[as::cam_dir_index(1, p, R)],
                                dirs[as::cam_dir_index(2, p, R)]};
        float d[3], inv[3], nrm[3];
        as::ray_quat_apply(f.quat, dir_l, d);
        as::ray_inverse(d, inv);
        as::RayBest b;
        as::ray_begin(b);
        if (surfaces & as::kRaySurfGround) as::ray_ground(b, f.pos, d, inv, ground_z, as::kCamCastMax);
        if (surfaces & as::kRaySurfStones)
          for (int s = 0; s < ns; ++s) {
            const float ctr[3] = {st[(size_t)(3 * s) * n], st[(size_t)(3 * s + 1) * n], st[(size_t)(3 * s + 2) * n]};
            as::ray_stone(b, f.pos, d, inv, ctr, half, as::kCamCastMax, s);
          }
        const int sh = b.surface >= 0 ? b.surface : 0;
        const float ctr[3] = {st[(size_t)(3 * sh) * n], st[(size_t)(3 * sh + 1) * n], st[(size_t)(3 * sh + 2) * n]};
        as::cam_normal(b, f.pos, d, inv, ctr, half, nrm);
        const float pl = as::cam_plane(f.q_inv, b.t, d, clipping, max_distance);
        const float cm = as::cam_clip_camera(b.t, clipping, max_distance);
        as::CamPixel px;
        as::cam_pixel_one(f, dir_l, surfaces, clipping, max_distance, st, (size_t)n, ns, half, ground_z, px);
        case_bad += px.surface != b.surface;
        case_bad += bits(px.t) != bits(b.t);
        case_bad += bits(px.plane) != bits(pl);
        case_bad += bits(px.camera) != bits(cm);
        plane[as::cam_pixel_index(e, p, R)] = pl;
        camera[as::cam_pixel_index(e, p, R)] = cm;
        ts[as::cam_pixel_index(e, p, R)] = b.t;
        surface[as::cam_pixel_index(e, p, R)] = b.surface;
        for (int k = 0; k < 3; ++k) {
          case_bad += bits(px.normal[k]) != bits(nrm[k]);
          case_bad += bits(px.d[k]) != bits(d[k]);
          normals[as::cam_normal_index(e, p, k, R)] = nrm[k];
          dirs_w[as::cam_normal_index(e, p, k, R)] = d[k];
        }
        ++pixels;
        stone_hits += b.surface >= 0;
        ground_hits += b.surface == as::kRayHitGround;
        misses += b.surface == as::kRayMiss;
      }
    }
    if (!(put(out, pose) && put(out, plane) && put(out, camera) && put(out, normals) && put(out, dirs_w) &&
          put(out, ts) && put(out, surface))) {
      printf("case %d: short write\n", c);
      return bad + 1;
    }
    printf("case %d: n %d image %d x %d surfaces %d clipping %d: %d mismatches\n", c, (int)n, (int)W, (int)H,
           (int)surfaces, (int)clipping, case_bad);
    bad += case_bad;
  }
  if (!r.ok) {
    printf("cases.bin: short read\n");
    return bad + 1;
  }
  printf("ray camera: %d cases, %ld pixels, %ld stone hits, %ld ground hits, %ld misses, %d mismatches\n", (int)ncases,
         pixels, stone_hits, ground_hits, misses, bad);
  return bad;
}

// the layout helpers are row-major [k][pixel] / [env][pixel] / [env][pixel][k], and the codes are the documented ones
int check_layout() {
  int bad = 0;
  const int n = 3, R = 5;
  size_t next = 0;
  for (int k = 0; k < 3; ++k)
    for (int p = 0; p < R; ++p) bad += as::cam_dir_index(k, p, R) != next++;
  next = 0;
  for (int e = 0; e < n; ++e)
    for (int p = 0; p < R; ++p) bad += as::cam_pixel_index(e, p, R) != next++;
  next = 0;
  for (int e = 0; e < n; ++e)
    for (int p = 0; p < R; ++p)
      for (int k = 0; k < 3; ++k) bad += as::cam_normal_index(e, p, k, R) != next++;
  bad += !(as::kCamClipNone == AS_CAM_CLIP_NONE && as::kCamClipMax == AS_CAM_CLIP_MAX &&
           as::kCamClipZero == AS_CAM_CLIP_ZERO && as::kCamPoseRows == 7 && as::kCamCastMax == 1e6f);
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
