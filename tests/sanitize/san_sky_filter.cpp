// Stand-alone driver for the host instantiation of cvk::sky_bilinear_taps and cvk::sky_bilinear_blend (curvis_amd/csrc/cv_device.h),
// built with -fsanitize=address,undefined and run by tests/test_sky_filter_host.py.  For every sky size and direction it checks what
// the definition promises about the taps (all inside the sky, weights below 256, the nearest indices those of sky_indices, the wrap
// and the clamps) and reads the four texels from a heap image of exactly w * h texels, so that an index one past the end is an
// AddressSanitizer report and a shift or overflow a UBSan one.  Prints "sky filter ok: <n> lookups".
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "../../curvis_amd/csrc/cv_device.h"

static std::vector<double> g_dirs;

static void add(double x, double y, double z) {
  g_dirs.push_back(x), g_dirs.push_back(y), g_dirs.push_back(z);
}
static void add_ulps(double x, double y, double z) {
  const double inf = std::numeric_limits<double>::infinity();
  add(x, y, z);
  for (double to : {inf, -inf}) {
    add(std::nextafter(x, to), y, z);
    add(x, std::nextafter(y, to), z);
    add(x, y, std::nextafter(z, to));
  }
}

static void fail(const char *what, unsigned w, unsigned h, const double *d, const cvk::SkyTaps &t) {
  std::fprintf(stderr, "san_sky_filter: %s: sky %u x %u, direction (%a, %a, %a): x0 %u x1 %u y0 %u y1 %u fx %u fy %u tx %u ty %u oob %d\n", what, w, h,
               d[0], d[1], d[2], t.x0, t.x1, t.y0, t.y1, t.fx, t.fy, t.tx, t.ty, (int)t.oob);
  std::exit(1);
}

int main() {
  const double pi = 3.14159265358979323846;
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  // +-z, the seam, every texel-centre and texel-edge longitude and latitude of a 13 x 7 sky, each +- 1 ulp; zeros, NaN, infinities
  for (double z : {1.0, -1.0, -2.5}) add_ulps(0.0, 0.0, z), add_ulps(-0.0, 1e-300, z);
  for (double y : {0.0, -0.0, 5e-324, -5e-324}) add_ulps(-1.0, y, 0.0), add_ulps(-3.0, y, 0.3);
  for (int k = 0; k <= 26; ++k) {
    const double phi = 2.0 * pi * (0.5 - 0.5 * k / 13.0);
    for (double z : {0.0, 0.25, -3.0}) add_ulps(std::cos(phi), std::sin(phi), z);
    for (int j = 0; j <= 14; ++j) {
      const double th = pi * 0.5 * j / 7.0;
      add_ulps(std::sin(th) * std::cos(phi), std::sin(th) * std::sin(phi), std::cos(th));
    }
  }
  const double special[] = {nan, inf, -inf, 0.0, -0.0, 1.0, -0.5, 1e-320, 1e300};
  for (double a : special)
    for (double b : special)
      for (double c : special) add(a, b, c);
  uint64_t s = 0x9E3779B97F4A7C15ull; /* and pseudo-random ones over the exponent range */
  for (int i = 0; i < 20000; ++i) {
    double v[3];
    for (double &c : v) {
      s = s * 6364136223846793005ull + 1442695040888963407ull;
      c = std::ldexp((double)(int64_t)(s >> 11) / 9007199254740992.0 - 0.5, (int)((s >> 3) % 400) - 200);
    }
    add(v[0], v[1], v[2]);
  }

  const unsigned sizes[][2] = {{1, 1}, {3, 2}, {13, 7}, {1000, 500}, {4095, 2047}, {1u << 23, 1}, {1, 1u << 23}};
  const double rots[][9] = {{1, 0, 0, 0, 1, 0, 0, 0, 1}, {0, 0, 1, 0, 1, 0, -1, 0, 0}, {0.36, 0.48, -0.8, -0.8, 0.6, 0.0, 0.48, 0.64, 0.6}};
  unsigned long long n = 0, sum = 0;
  for (const auto &size : sizes) {
    const unsigned w = size[0], h = size[1];
    std::vector<unsigned> texels((size_t)w * h); /* exactly w * h: one past the end is a report */
    for (size_t i = 0; i < texels.size(); ++i) texels[i] = (unsigned)(i * 2654435761u) ^ 0x00A5C33Cu;
    for (const auto &rot : rots) {
      cvk::SkyParams S;
      S.texels = texels.data();
      S.w = w;
      S.h = h;
      for (int i = 0; i < 9; ++i) S.inv_rot[i] = rot[i];
      for (size_t i = 0; i < g_dirs.size(); i += 3) {
        const double *d = &g_dirs[i];
        cvk::SkyTaps t;
        cvk::sky_bilinear_taps(S, d[0], d[1], d[2], t);
        unsigned tx, ty;
        cvk::sky_indices(S, d[0], d[1], d[2], tx, ty);
        if (t.x0 >= w || t.x1 >= w || t.y0 >= h || t.y1 >= h || t.fx > 255u || t.fy > 255u) fail("tap outside the sky", w, h, d, t);
        if (t.tx != tx || t.ty != ty || t.oob != (tx >= w || ty >= h)) fail("X >> 8, Y >> 8 are not sky_indices' tx, ty", w, h, d, t);
        if (t.x1 != (t.x0 + 1u == w ? 0u : t.x0 + 1u)) fail("longitude does not wrap", w, h, d, t);
        if (t.y1 != (t.y0 + 1u < h ? t.y0 + 1u : h - 1u)) fail("colatitude does not clamp", w, h, d, t);
        const unsigned cx = tx < w ? tx : w - 1u, cy = ty < h ? ty : h - 1u; /* the nearest texel is one of the four, and the heaviest */
        const bool near_x = (t.fx < 128u ? t.x0 : t.x1) == cx, near_y = (t.fy < 128u ? t.y0 : t.y1) == cy || (t.y0 == 0u && t.fy == 0u && cy == 0u);
        if (!near_x || !near_y) fail("the nearest texel is not the heaviest tap", w, h, d, t);
        const unsigned *row0 = S.texels + (size_t)t.y0 * w, *row1 = S.texels + (size_t)t.y1 * w;
        const unsigned a = row0[t.x0], b = row0[t.x1], c = row1[t.x0], e = row1[t.x1];
        const unsigned out = cvk::sky_bilinear_blend(a, b, c, e, t.fx, t.fy);
        for (unsigned sh = 0; sh < 24; sh += 8) { /* a blend lies between the smallest and the largest of its four values */
          const unsigned v[4] = {(a >> sh) & 255u, (b >> sh) & 255u, (c >> sh) & 255u, (e >> sh) & 255u};
          unsigned lo = v[0], hi = v[0];
          for (unsigned x : v) lo = x < lo ? x : lo, hi = x > hi ? x : hi;
          const unsigned o = (out >> sh) & 255u;
          if (o < lo || o > hi) fail("blend outside its inputs", w, h, d, t);
        }
        if ((out >> 24) != 255u) fail("alpha", w, h, d, t);
        sum += out;
        ++n;
      }
    }
  }
  std::printf("sky filter ok: %llu lookups (checksum %llu)\n", n, sum);
  return 0;
}
