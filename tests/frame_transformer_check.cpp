// frame_transformer_check.cpp -- stand-alone host run of csrc/allsteps_frame_transformer.h
// (tests/test_frame_transformer_host.py builds and runs it, plain and under -fsanitize=address,undefined).
//
//   frame_transformer_check <cases.bin> <out.bin>
//
// cases.bin (written by tests/_frame_transformer_cases.py, native endianness):
//   int32 ncases, then per case
//     int32 n, U, B, F, source, apply_source, apply_target;  float source_offset[7] (pos 3 | rot 4)
//     int32 frame_body[F];  float frame_offset[F][7];  float pose[U][B][7][n]
// out.bin, per case:
//     float source[U][7][n], target[U][14][F][n]     the buffers after every update
// The program replays a case the way k_frame_transformer does, one sensor (S = 1) on buffers laid out as the
// device's (frame_index): per update every env's every frame gathers the source body's and its own body's link
// pose from the env-minor rows, runs frame_source and frame_target and scatters the rows; the first frame stores
// the source rows.  The comparison with the fixture and the NumPy restatement is the test's.
#include <cstdio>
#include <vector>

#include "../allsteps_isaaclab_amd/csrc/allsteps_frame_transformer.h"

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

as::FrameOffset offset_of(const float* o) {
  as::FrameOffset r;
  for (int k = 0; k < 3; ++k) r.pos[k] = o[k];
  for (int k = 0; k < 4; ++k) r.rot[k] = o[3 + k];
  return r;
}

int run_cases(Reader& r, FILE* out) {
  const int32_t ncases = r.one<int32_t>();
  long frames_done = 0;
  for (int c = 0; c < ncases && r.ok; ++c) {
    const int32_t n = r.one<int32_t>(), U = r.one<int32_t>(), B = r.one<int32_t>(), F = r.one<int32_t>();
    const int32_t src = r.one<int32_t>(), apply_source = r.one<int32_t>(), apply_target = r.one<int32_t>();
    if (!r.ok || n < 1 || U < 1 || B < 1 || F < 1 || src < 0 || src >= B) {
      printf("case %d: bad header\n", c);
      return 1;
    }
    const std::vector<float> source_offset = r.many<float>(7);
    const std::vector<int32_t> body = r.many<int32_t>((size_t)F);
    const std::vector<float> offsets = r.many<float>((size_t)F * 7);
    const std::vector<float> pose = r.many<float>((size_t)U * B * 7 * n);
    if (!r.ok) break;
    for (int f = 0; f < F; ++f)
      if (body[f] < 0 || body[f] >= B) {
        printf("case %d: frame %d names body %d\n", c, f, (int)body[f]);
        return 1;
      }
    const int S = 1, s = 0;
    const as::FrameOffset so = offset_of(source_offset.data());
    std::vector<float> source((size_t)as::kFrameSourceRows * S * n, 0.f), target((size_t)as::kFrameTargetRows * F * n, 0.f);
    std::vector<float> all_source, all_target;
    for (int u = 0; u < U; ++u) {
      const float* ps = &pose[(size_t)u * B * 7 * n];
      for (int e = 0; e < n; ++e)
        for (int f = 0; f < F; ++f) {
          float p[3], q[4], srow[as::kFrameSourceRows], trow[as::kFrameTargetRows];
          for (int k = 0; k < 3; ++k) p[k] = ps[((size_t)src * 7 + k) * n + e];
          for (int k = 0; k < 4; ++k) q[k] = ps[((size_t)src * 7 + 3 + k) * n + e];
          as::frame_source(p, q, apply_source != 0, so, srow);
          for (int k = 0; k < 3; ++k) p[k] = ps[((size_t)body[f] * 7 + k) * n + e];
          for (int k = 0; k < 4; ++k) q[k] = ps[((size_t)body[f] * 7 + 3 + k) * n + e];
          as::frame_target(srow, p, q, apply_target != 0, offset_of(&offsets[(size_t)f * 7]), trow);
          if (f == 0)
            for (int k = 0; k < as::kFrameSourceRows; ++k) source[as::frame_index(k, s, e, n, S)] = srow[k];
          for (int k = 0; k < as::kFrameTargetRows; ++k) target[as::frame_index(k, f, e, n, F)] = trow[k];
          ++frames_done;
        }
      all_source.insert(all_source.end(), source.begin(), source.end());
      all_target.insert(all_target.end(), target.begin(), target.end());
    }
    if (!(put(out, all_source) && put(out, all_target))) {
      printf("case %d: short write\n", c);
      return 1;
    }
    printf("case %d: n %d updates %d bodies %d frames %d\n", c, (int)n, (int)U, (int)B, (int)F);
  }
  if (!r.ok) {
    printf("cases.bin: short read\n");
    return 1;
  }
  printf("frame_transformer: %d cases, %ld frames\n", (int)ncases, frames_done);
  return 0;
}

// the layout helper is row-major [row][slot][env] and the row constants are the documented ones
int check_layout() {
  int bad = 0;
  const int n = 7, F = 5;
  size_t next = 0;
  for (int row = 0; row < as::kFrameTargetRows; ++row)
    for (int f = 0; f < F; ++f)
      for (int e = 0; e < n; ++e) bad += as::frame_index(row, f, e, n, F) != next++;
  bad += !(as::kFrameSourcePos == 0 && as::kFrameSourceQuat == 3 && as::kFrameSourceRows == 7 && as::kFramePosW == 0 &&
           as::kFrameQuatW == 3 && as::kFramePosSource == 7 && as::kFrameQuatSource == 10 && as::kFrameTargetRows == 14);
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
