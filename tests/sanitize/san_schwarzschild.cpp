// Stand-alone driver for the host instantiation of the Schwarzschild kind (curvis_amd/csrc/cv_device.h metric_eval, cv_math.h
// cv_tortoise_u): the fast form of the Euler step (ray_step_fast) against the strict one (ray_step_core behind ray_step), bit for bit,
// built with -fsanitize=address,undefined and run by tests/test_schwarzschild_host.py.  Directed states: l at and around 0 (the rim
// of the funnel, -0 included) and deep inside it, the photon sphere (the l whose u is 1/2 and its neighbours, where R' changes sign
// through an exact zero), |l| up to and beyond 2^90, sin(theta) tiny, p_phi = 0; then whole rays walked with both forms, Euler and
// Heun, captured and escaping.  Every state lives in a heap block of exactly its size.  Prints "schwarzschild ok: <n> values".
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "../../curvis_amd/csrc/cv_device.h"

constexpr int K = cvk::METRIC_SCHWARZSCHILD;

static void fail(const char *what, double l, double got) {
  std::fprintf(stderr, "san_schwarzschild: %s: l %a: %a\n", what, l, got);
  std::exit(1);
}
static bool same(double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0 || (a != a && b != b); }

static cvk::MetricParams metric(double mass) {
  cvk::MetricParams M;
  M.rho = 0.0, M.rho2 = 0.0, M.m = mass, M.a = 0.0, M.pim = 2.0 * mass, M.inv_pim = 1.0 / M.pim, M.two_o_pi = 2.0 / CV_PI;
  M.T = cv_sc_table(), M.LT = cv_log_table(), M.AT = cv_atan_table();
  return M;
}

static unsigned long long one_state(const cvk::MetricParams &M, double max_radius, double l, double th, double p1, double p2, double p3, double delta) {
  std::unique_ptr<cvk::Ray> a(new cvk::Ray()), b(new cvk::Ray());
  a->l = l, a->th = th, a->ph = 0.25, a->p1 = p1, a->p2 = p2, a->p3 = p3, a->p3sq = p3 * p3;
  *b = *a;
  const bool ok = cvk::metric_fast_ok(K, M, max_radius) && cvk::ray_fast_ok(*a);
  cvk::ray_step<K, true>(M, *a, delta);
  cvk::ray_step_fast<K, true>(M, *b, delta, ok);
  if (!same(a->l, b->l) || !same(a->th, b->th) || !same(a->ph, b->ph) || !same(a->p1, b->p1) || !same(a->p2, b->p2))
    fail("the fast step leaves the strict one's bits", l, b->p1);
  return 5;
}

static unsigned long long directed(double mass) {
  const cvk::MetricParams M = metric(mass);
  unsigned long long n = 0;
  /* the l whose u is 1/2: y = 1/2 + log(1/2), l = 2M (y + 1); the neighbours within a few ulp cover u = 1/2 - ulp, 1/2, 1/2 + ulp */
  const double l_ps = 2.0 * mass * (1.5 + std::log(0.5));
  std::unique_ptr<double[]> ls(new double[64]);
  int nl = 0;
  for (double v : {0.0, -0.0, 5e-324, -5e-324, 1e-120, -1e-120, 0x1p-100, 0x1p-101, -0x1p-99, 1e-9, -1e-9, -3.0, -24.0, 0.3, 2.0, 8.0, 29.99, -29.99, 0x1p89, 0x1.fp89,
                   0x1p90, -0x1p90, 0x1p91, 1e300})
    ls[nl++] = v * (std::fabs(v) < 1e80 && std::fabs(v) > 1e-80 ? mass : 1.0);
  double v = l_ps;
  for (int k = 0; k < 6; ++k) v = std::nextafter(v, 0.0);
  int neg = 0, zero = 0, pos = 0;
  for (int k = 0; k < 13; ++k, v = std::nextafter(v, INFINITY)) {
    ls[nl++] = v;
    double r, r2, rd;
    cvk::metric_eval<K>(M, v, r, r2, rd);
    const double u = cvk::schwarzschild_u(M, v), t = 2.0 * u - 1.0;
    if ((rd < 0.0) != (t < 0.0) || (rd > 0.0) != (t > 0.0)) fail("R' has not the sign of 2u - 1", v, rd);
    neg += rd < 0.0, zero += rd == 0.0, pos += rd > 0.0;
  }
  if (!neg || !pos) fail("the sweep does not straddle the photon sphere", l_ps, (double)zero);
  /* the funnel: the values of l = 0, bit for bit */
  double r0, r20, rd0;
  cvk::metric_eval<K>(M, 0.0, r0, r20, rd0);
  if (!(rd0 < 0.0)) fail("R'(0) is not negative", 0.0, rd0);
  for (double l : {-0.0, -5e-324, -1e-300, -1.0, -25.0, -1e300}) {
    double r, r2, rd;
    cvk::metric_eval<K>(M, l, r, r2, rd);
    if (!same(r, r0) || !same(r2, r20) || !same(rd, rd0)) fail("the funnel is not constant", l, r);
    n += 3;
  }
  const double ths[] = {1.2, 1.5707963267948966, 1e-9, 1e-70, 3.141592653589, -0.4, 7.0};
  const double p3s[] = {0.7, 0.0, -2.5e-3};
  for (int i = 0; i < nl; ++i)
    for (double th : ths)
      for (double p3 : p3s)
        for (double delta : {0.05, 3.0})
          for (double p1 : {-0.9, 0.8}) n += one_state(M, 30.0 * (mass > 1.0 ? mass : 1.0), ls[i], th, p1, 0.3, p3 * mass, delta * mass);
  return n;
}

/* whole rays: captured (small impact parameter), grazing and escaping, Euler and Heun, both forms of the step */
static unsigned long long rays(double mass) {
  const cvk::MetricParams M = metric(mass);
  const double R = 25.0 * mass, delta = 0.05 * mass;
  unsigned long long n = 0, captured = 0, escaped = 0;
  for (int heun = 0; heun < 2; ++heun)
    for (int r = 0; r < 24; ++r) {
      std::unique_ptr<cvk::Ray> a(new cvk::Ray()), b(new cvk::Ray());
      double rr, r2, rd;
      cvk::metric_eval<K>(M, 8.0 * mass, rr, r2, rd);
      const double ang = 0.05 + 0.04 * r; /* angle from the inward radial direction */
      a->l = 8.0 * mass, a->th = 1.1, a->ph = 0.0, a->p1 = -std::cos(ang), a->p2 = 0.6 * std::sin(ang) * rr, a->p3 = 0.8 * std::sin(ang) * rr * std::sin(1.1);
      a->p3sq = a->p3 * a->p3;
      *b = *a;
      const bool ok = cvk::metric_fast_ok(K, M, R) && cvk::ray_fast_ok(*a);
      if (!ok) fail("the guard refuses an ordinary ray", a->l, a->p3sq);
      int k = 0;
      for (; k < 8192 && std::fabs(a->l) <= R; ++k) {
        if (heun) {
          cvk::ray_step_heun<K, true, false>(M, *a, delta, false);
          cvk::ray_step_heun<K, true, true>(M, *b, delta, ok);
        } else {
          cvk::ray_step<K, true>(M, *a, delta);
          cvk::ray_step_fast<K, true>(M, *b, delta, ok);
        }
        if (std::memcmp(a.get(), b.get(), sizeof(cvk::Ray)) != 0) fail("the fast step leaves the strict one's bits on a ray", a->l, b->l);
        ++n;
      }
      if (k == 8192) fail("a ray neither escaped nor was captured", a->l, (double)r);
      captured += a->l < 0.0, escaped += a->l > 0.0;
    }
  if (captured < 8 || escaped < 8) fail("too few rays of one class", (double)captured, (double)escaped);
  return n;
}

int main() {
  unsigned long long n = 0;
  for (double mass : {1.0, 0.37, 0x1p-20, 1000.0}) n += directed(mass);
  n += rays(1.0) + rays(0.37);
  std::printf("schwarzschild ok: %llu values\n", n);
  return 0;
}
