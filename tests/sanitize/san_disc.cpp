// Stand-alone driver for the host instantiation of cvk::disc_crossing (curvis_amd/csrc/cv_device.h), the body of the ABI's host accessor
// curvis_disc_crossing; built with -fsanitize=address,undefined and run by tests/test_disc_host.py.  Directed inputs: cosines one ulp
// either side of a sign change, t at 0 and 1, l_hit one ulp inside and outside each bound, phi_hit at 0, 2 pi +- ulp, negative and
// huge, s < 0, NaN and infinity in every argument, textures of 1 and of 2^23 texels per side; then the step hands the probe the sincos
// the strict step evaluates.  Every texel index lives in a heap block of exactly one unsigned.  Prints "disc ok: <n> values".
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <memory>

#include "../../curvis_amd/csrc/cv_device.h"

static void fail(const char *what, const double *a, unsigned w, unsigned h) {
  std::fprintf(stderr, "san_disc: %s: c %a %a s %a l %a %a phi %a %a bounds %a %a size %u x %u\n", what, a[0], a[1], a[2], a[3], a[4], a[5],
               a[6], a[7], a[8], w, h);
  std::exit(1);
}

static unsigned as_u32(double v) {
  if (!(v == v) || v <= 0.0) return 0u;
  if (v >= 4294967295.0) return 4294967295u;
  return (unsigned)v;
}
static double rem_euclid(double a, double b) {
  double r = (std::fabs(a) < b || a != a) ? a : std::fmod(a, b);
  return r < 0.0 ? r + b : r;
}
/* the definition's steps 1-7, written out */
static bool definition(const double *a, unsigned w, unsigned h, unsigned *tx, unsigned *ty) {
  const double c0 = a[0], c1 = a[1], s1 = a[2], l0 = a[3], l1 = a[4], p0 = a[5], p1 = a[6], lin = a[7], lout = a[8];
  if ((c0 < 0.0) == (c1 < 0.0)) return false;
  const volatile double t = c0 / (c0 - c1);
  const volatile double dl = l1 - l0, dp = p1 - p0;
  const volatile double tl = t * dl, tp = t * dp;
  const volatile double lh = l0 + tl;
  volatile double ph = p0 + tp;
  if (!(lin <= lh && lh <= lout)) return false;
  if (s1 < 0.0) ph = ph + CV_PI;
  const double two_pi = 2.0 * CV_PI;
  const volatile double u = rem_euclid(ph, two_pi) / two_pi;
  const volatile double v = (lh - lin) / (lout - lin);
  const unsigned x = as_u32(u * (double)w), y = as_u32(v * (double)h);
  *tx = x < w - 1u ? x : w - 1u;
  *ty = y < h - 1u ? y : h - 1u;
  return true;
}

static unsigned long long n_values = 0;
static void one(const double *a, unsigned w, unsigned h) {
  std::unique_ptr<unsigned> tx(new unsigned(0xDEADu)), ty(new unsigned(0xBEEFu));
  unsigned ex = 0xDEADu, ey = 0xBEEFu;
  const bool got = cvk::disc_crossing(a[0], a[1], a[2], a[3], a[4], a[5], a[6], a[7], a[8], w, h, tx.get(), ty.get());
  const bool want = definition(a, w, h, &ex, &ey);
  if (got != want) fail("hit or miss", a, w, h);
  if (*tx != ex || *ty != ey) fail("texel", a, w, h); /* a miss writes neither */
  if (got && (*tx >= w || *ty >= h)) fail("texel outside the texture", a, w, h);
  ++n_values;
}

int main() {
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  const double up = inf, two_pi = 2.0 * CV_PI;
  const unsigned sizes[4][2] = {{97u, 53u}, {1u, 1u}, {1u << 23, 1u << 23}, {1u, 1u << 23}};
  for (const auto &wh : sizes) {
    const unsigned w = wh[0], h = wh[1];
    /* cosines either side of a sign change, the smallest cosines a double has, equal signs */
    const double cs[][2] = {{6.123233995736766e-17, -6.123233995736766e-17}, {-6.123233995736766e-17, 6.123233995736766e-17}, {0.3, -0.2}, {-0.3, 0.2},
                            {5e-324, -5e-324}, {-5e-324, 1.0}, {1.0, -5e-324}, {1.0, -1.0}, {0.25, 0.5}, {-0.25, -0.5}, {0.0, -0.0}, {-0.0, 0.0},
                            {0.0, -1.0}, {-1.0, 0.0}, {std::nextafter(0.0, -1.0), std::nextafter(0.0, 1.0)}};
    for (const auto &c : cs)
      for (double s : {1.0, -1.0, 0.5, -1e-300})
        for (double lin : {1.5, -6.0})
          for (double lout : {5.0, -0.8, 1e300}) {
            /* l_hit at, one ulp inside and one ulp outside each bound (l_prev = l_cur = the value: l_hit is that value for every t) */
            const double ls[] = {lin, std::nextafter(lin, up), std::nextafter(lin, -up), lout, std::nextafter(lout, up), std::nextafter(lout, -up), 0.5 * (lin + lout)};
            for (double l : ls)
              for (double ph : {0.0, -0.0, two_pi, std::nextafter(two_pi, up), std::nextafter(two_pi, 0.0), -1.0, -two_pi, 1e300, -1e300, 3.0, 5e-324}) {
                const double a[9] = {c[0], c[1], s, l, l, ph, ph, lin, lout};
                one(a, w, h);
              }
            /* t = 0 and t = 1 in effect: one cosine dwarfs the other, distinct end points */
            const double b0[9] = {5e-324, -1.0, s, lin, lout, 0.0, 6.0, lin, lout}, b1[9] = {1.0, -5e-324, s, lin, lout, 0.0, 6.0, lin, lout};
            one(b0, w, h);
            one(b1, w, h);
          }
    /* NaN and infinity in every argument, one at a time and all at once */
    const double base[9] = {0.3, -0.2, 1.0, 2.0, 2.5, 1.0, 1.1, 1.5, 5.0};
    for (double v : {nan, inf, -inf}) {
      double all[9];
      for (int i = 0; i < 9; ++i) {
        double a[9];
        std::memcpy(a, base, sizeof a);
        a[i] = v;
        all[i] = v;
        one(a, w, h);
      }
      one(all, w, h);
    }
  }
  { /* the sincos a step hands its probe is the one the strict step evaluates, and the state is untouched when it arrives */
    struct Probe {
      double *s, *c, *l_seen;
      const cvk::Ray *q;
      void sincos(double s_, double c_) const { *s = s_, *c = c_, *l_seen = q->l; }
    };
    cvk::MetricParams M;
    M.rho = 1.0, M.rho2 = 1.0, M.m = 0.5, M.a = 2.0, M.pim = CV_PI * M.m, M.inv_pim = 1.0 / M.pim, M.two_o_pi = 2.0 / CV_PI;
    M.T = cv_sc_table(), M.LT = cv_log_table(), M.AT = cv_atan_table();
    for (int r = 0; r < 16; ++r) {
      cvk::Ray a = {}, b = {};
      a.l = 5.0, a.th = 1.2 + 0.02 * r, a.ph = 0.0, a.p1 = -0.98, a.p2 = 0.4 * (r - 8), a.p3 = 0.3 + 0.1 * r, a.p3sq = a.p3 * a.p3;
      b = a;
      for (int k = 0; k < 2048 && std::fabs(a.l) <= 30.0; ++k) {
        std::unique_ptr<double> s(new double(0.0)), c(new double(0.0)), l_seen(new double(0.0));
        double es, ec;
        cv_sincos_t(a.th, M.T, &es, &ec);
        const double l_before = a.l;
        cvk::ray_step_probed<cvk::METRIC_ELLIS, true, false>(M, a, 0.05, Probe{s.get(), c.get(), l_seen.get(), &a});
        cvk::ray_step<cvk::METRIC_ELLIS, true>(M, b, 0.05);
        if (std::memcmp(&a, &b, sizeof a) != 0 || std::memcmp(s.get(), &es, 8) != 0 || std::memcmp(c.get(), &ec, 8) != 0 || *l_seen != l_before) {
          std::fprintf(stderr, "san_disc: the probed step differs from the strict step at ray %d step %d\n", r, k);
          return 1;
        }
        ++n_values;
      }
    }
  }
  std::printf("disc ok: %llu values\n", n_values);
  return 0;
}
