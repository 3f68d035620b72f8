// Stand-alone host check of csrc/allsteps_pair_group.h (built and run by tests/test_pair_group.py, plain
// and with -fsanitize=address,undefined).  A group of 2^L lanes (L = 2, 3, 4) is emulated serially: every
// sub-lane's slope sign at its point, the walk on the sign bits, 12 / L rounds.  After every group round
// lo and hi must be the bits the 12-round one-lane loop (oracle/physics.c collide()) holds after the same
// number of rounds, every t that loop evaluated must be one of the group's points of that round, bit for
// bit, and the final t = 0.5 (lo + hi) must match.  sd_box_slope is restated from the oracle.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../allsteps_isaaclab_amd/csrc/allsteps_pair_group.h"

static float sd_box_slope(const float a[3], const float b[3], float t, const float c[3], const float h[3]) {
  float d[3], sD[3];
  for (int k = 0; k < 3; ++k) {
    const float D = b[k] - a[k];
    const float r = fmaf(t, D, a[k] - c[k]);
    sD[k] = r >= 0.f ? D : -D;
    d[k] = fabsf(r) - h[k];
  }
  if (fmaxf(d[0], fmaxf(d[1], d[2])) > 0.f) {
    float o0 = d[0] > 0.f ? d[0] : 0.f, o1 = d[1] > 0.f ? d[1] : 0.f, o2 = d[2] > 0.f ? d[2] : 0.f;
    return fmaf(o2, sD[2], fmaf(o1, sD[1], o0 * sD[0]));
  }
  int ax = 0;
  if (d[1] > d[ax]) ax = 1;
  if (d[2] > d[ax]) ax = 2;
  return sD[ax];
}

static uint32_t bits_of(float x) { uint32_t u; std::memcpy(&u, &x, 4); return u; }

static long long g_cases = 0, g_bad = 0;

static void fail(const char* what, int L, int round, float got, float want, const float* a, const float* b,
                 const float* c) {
  if (g_bad++ < 20)
    std::printf("L=%d round %d %s: got %.9g want %.9g  a=(%g %g %g) b=(%g %g %g) c=(%g %g %g)\n", L, round, what,
                (double)got, (double)want, a[0], a[1], a[2], b[0], b[1], b[2], c[0], c[1], c[2]);
}

static void check(const float a[3], const float b[3], const float c[3], const float h[3]) {
  ++g_cases;
  // the one-lane loop, with its t and interval per round
  float slo[as::kPairGroupIters + 1], shi[as::kPairGroupIters + 1], st[as::kPairGroupIters];
  float lo = 0.f, hi = 1.f;
  slo[0] = lo; shi[0] = hi;
  for (int it = 0; it < as::kPairGroupIters; ++it) {
    const float t = 0.5f * (lo + hi);
    st[it] = t;
    if (sd_box_slope(a, b, t, c, h) > 0.f) hi = t; else lo = t;
    slo[it + 1] = lo; shi[it + 1] = hi;
  }
  const float tfin = 0.5f * (lo + hi);
  for (int L = 2; L <= 4; ++L) {
    float glo = 0.f, gd = 1.f;  // the group's state: lo and the width hi - lo
    for (int r = 0; r < as::kPairGroupIters / L; ++r) {
      const float w = gd * as::pair_group_scale(L);
      float pt[16];
      uint32_t bits = 0u;
      for (int k = 0; k < (1 << L); ++k) {  // every lane of the group evaluates; the last one's sign is not read
        pt[k] = as::pair_group_point(glo, w, k);
        if (k < (1 << L) - 1 && sd_box_slope(a, b, pt[k], c, h) > 0.f) bits |= 1u << k;
      }
      for (int s = 0; s < L; ++s) {
        bool found = false;
        for (int k = 0; k < (1 << L) - 1; ++k) found = found || bits_of(pt[k]) == bits_of(st[r * L + s]);
        if (!found) fail("t not among the group's points", L, r, pt[0], st[r * L + s], a, b, c);
      }
      as::pair_group_walk(glo, w, L, bits);
      gd = w;
      const float ghi = glo + gd;
      if (bits_of(glo) != bits_of(slo[(r + 1) * L])) fail("lo", L, r, glo, slo[(r + 1) * L], a, b, c);
      if (bits_of(ghi) != bits_of(shi[(r + 1) * L])) fail("hi", L, r, ghi, shi[(r + 1) * L], a, b, c);
    }
    const float tg = 0.5f * (glo + (glo + gd));
    if (bits_of(tg) != bits_of(tfin)) fail("t*", L, -1, tg, tfin, a, b, c);
  }
}

// xorshift64*: uniform floats in [0, 1)
static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static float urand() {
  g_rng ^= g_rng >> 12; g_rng ^= g_rng << 25; g_rng ^= g_rng >> 27;
  return (float)((g_rng * 0x2545F4914F6CDD1Dull) >> 40) * (1.0f / 16777216.0f);
}
static float sym(float m) { return (2.f * urand() - 1.f) * m; }

int main() {
  const float h[3] = {0.4f, 0.25f, 0.1f};
  // adversarial cases, each at the origin and at the far end of the stones' 15 m range
  for (int far = 0; far < 2; ++far) {
    const float o = far ? 15.f : 0.f;
    const float c[3] = {o, -o, 0.5f * o};
    auto at = [&](float x, float y, float z, float* p) { p[0] = c[0] + x; p[1] = c[1] + y; p[2] = c[2] + z; };
    float a[3], b[3];
    at(-1.f, 0.1f, 0.3f, a); at(1.f, 0.1f, 0.3f, b); check(a, b, c, h);        // parallel to the top face, above it
    at(-1.f, 0.25f, 0.1f, a); at(1.f, 0.25f, 0.1f, b); check(a, b, c, h);      // along an edge, on the faces' planes
    at(0.7f, -1.f, 0.f, a); at(0.7f, 1.f, 0.f, b); check(a, b, c, h);          // parallel to a side face
    at(0.3f, 0.2f, 0.5f, a); at(0.3f, 0.2f, 0.5f, b); check(a, b, c, h);       // zero length, outside
    at(0.f, 0.f, 0.f, a); at(0.f, 0.f, 0.f, b); check(a, b, c, h);             // zero length, at the centre
    at(-0.2f, 0.1f, 0.02f, a); at(0.3f, -0.1f, -0.05f, b); check(a, b, c, h);  // inside the box
    at(-0.39f, 0.f, 0.09f, a); at(0.39f, 0.f, 0.09f, b); check(a, b, c, h);    // inside, parallel to a face
    at(0.5f, 0.3f, 0.2f, a); at(2.f, 1.f, 1.5f, b); check(a, b, c, h);         // minimum at t = 0
    at(2.f, 1.f, 1.5f, a); at(0.5f, 0.3f, 0.2f, b); check(a, b, c, h);         // minimum at t = 1
    at(0.5f, 0.f, 0.3f, a); at(0.5f, 0.f, 1.3f, b); check(a, b, c, h);         // minimum at t = 0, along the normal
    at(-1.f, -1.f, 0.f, a); at(1.f, 1.f, 0.f, b); check(a, b, c, h);           // through the centre, in the z = 0 plane
    at(0.f, 0.f, -1.f, a); at(0.f, 0.f, 1.f, b); check(a, b, c, h);            // through the centre along z
    at(-3.f, 0.f, 0.f, a); at(3.f, 0.f, 0.f, b); check(a, b, c, h);            // the x = y = z centre planes at t = 0.5
    at(-30.f, 4.f, 0.2f, a); at(30.f, -4.f, 0.1f, b); check(a, b, c, h);       // long, through the box
    at(-1e-3f, 0.f, 0.1f, a); at(1e-3f, 0.f, 0.1f, b); check(a, b, c, h);      // tiny, on the top face
  }
  // random segments and boxes: near the box, far from it, long and short, magnitudes up to 15 m
  for (int i = 0; i < 1200000; ++i) {
    const float range = (i & 3) == 0 ? 15.f : ((i & 3) == 1 ? 2.f : 0.6f);
    const float c[3] = {sym(15.f), sym(15.f), sym(15.f)};
    const float hh[3] = {0.05f + urand(), 0.05f + urand(), 0.05f + 0.5f * urand()};
    float a[3], b[3];
    for (int k = 0; k < 3; ++k) {
      a[k] = c[k] + sym(range);
      b[k] = (i & 12) == 0 ? a[k] + sym(0.6f) : c[k] + sym(range);
    }
    if ((i & 48) == 16) b[i % 3] = a[i % 3];  // axis-parallel in one coordinate
    check(a, b, c, (i & 1) ? hh : h);
  }
  std::printf("pair group: %lld cases, %lld mismatches\n", g_cases, g_bad);
  return g_bad ? 1 : 0;
}
