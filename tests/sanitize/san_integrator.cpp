// Stand-alone driver for the host instantiation of cvk::ray_step_heun and of cvk::heun_step_all, the body of the ABI's host accessor
// curvis_heun_step (curvis_amd/csrc/cv_device.h), under option "integrator" = 1; built with -fsanitize=address,undefined and run by
// tests/test_integrator_host.py.  One Heun step against the definition written out (two Euler steps from a saved state, one add and
// one halving per component) on directed states: the Interstellar strict zone, theta outside [0, pi], p_phi = 0, huge and tiny l, a
// stage state at and beyond 2^90 (the second stage's own guard); then whole rays walked with scaled Heun steps through the strict
// and the fast Euler step, past the escape radius in a stage.  Every state lives in heap blocks of exactly its size.  Prints
// "integrator ok: <n> values".
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "../../curvis_amd/csrc/cv_device.h"

static void fail(const char *what, int kind, double l, double got) {
  std::fprintf(stderr, "san_integrator: %s: metric %d, l %a: %a\n", what, kind, l, got);
  std::exit(1);
}
static bool same(double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0 || (a != a && b != b); }

template <int KIND>
static void euler_all(const cvk::MetricParams &M, double *x, double *p, double delta) {
  cvk::Ray q;
  q.l = x[1], q.th = x[2], q.ph = x[3], q.p1 = p[1], q.p2 = p[2], q.p3 = p[3], q.p3sq = p[3] * p[3];
  cvk::ray_step<KIND, true>(M, q, delta);
  x[0] = x[0] + (p[0] * (1.0 / -1.0)) * delta;
  x[1] = q.l, x[2] = q.th, x[3] = q.ph, p[1] = q.p1, p[2] = q.p2;
}
/* the definition, written out */
template <int KIND>
static void definition(const cvk::MetricParams &M, double *x, double *p, double delta) {
  double x0[4], p0[4];
  std::memcpy(x0, x, sizeof x0), std::memcpy(p0, p, sizeof p0);
  euler_all<KIND>(M, x, p, delta);
  euler_all<KIND>(M, x, p, delta);
  for (int i = 0; i < 4; ++i) x[i] = (x0[i] + x[i]) * 0.5;
  p[1] = (p0[1] + p[1]) * 0.5, p[2] = (p0[2] + p[2]) * 0.5;
}

template <int KIND>
static unsigned long long directed(const cvk::MetricParams &M) {
  unsigned long long n = 0;
  const double ls[] = {5.0, -4.0, 0.3, 2.1, -2.4, 3.5, 0.0, 29.99, -30.5, 1e-120, 0x1p89, 0x1.fp89, 0x1p90, -0x1p91, 1e300};
  const double ths[] = {1.2, 1.5707963267948966, -0.4, 3.5, 7.0, 1e-9};
  const double p3s[] = {0.7, 0.0, -2.5};
  const double deltas[] = {0.1, 0.05, 3.0, 0x1p88, 0x1p91};
  for (double l : ls)
    for (double th : ths)
      for (double p3 : p3s)
        for (double delta : deltas) {
          std::unique_ptr<double[]> x(new double[4]{1.5, l, th, 0.25}), p(new double[4]{1.0, -0.9, 0.3, p3});
          std::unique_ptr<double[]> wx(new double[4]{1.5, l, th, 0.25}), wp(new double[4]{1.0, -0.9, 0.3, p3});
          cvk::heun_step_all<KIND>(M, x.get(), p.get(), delta);
          definition<KIND>(M, wx.get(), wp.get(), delta);
          for (int i = 0; i < 4; ++i)
            if (!same(x[i], wx[i]) || !same(p[i], wp[i])) fail("heun_step_all is not the definition", KIND, l, x[i]);
          n += 8;
          /* the fast form of the step, second-stage guard included, returns the same bits: from a state inside the escape radius, as
           * in the kernels' loops -- the stage state lies where the first stage puts it, with the last two deltas near and beyond 2^90 */
          if (!(std::fabs(l) <= 30.0)) continue;
          std::unique_ptr<cvk::Ray> a(new cvk::Ray()), b(new cvk::Ray());
          a->l = l, a->th = th, a->ph = 0.25, a->p1 = -0.9, a->p2 = 0.3, a->p3 = p3, a->p3sq = p3 * p3;
          *b = *a;
          const bool ok = cvk::metric_fast_ok(KIND, M, 30.0) && cvk::ray_fast_ok(*a);
          cvk::ray_step_heun<KIND, true, false>(M, *a, delta, false);
          cvk::ray_step_heun<KIND, true, true>(M, *b, delta, ok);
          if (!same(a->l, b->l) || !same(a->th, b->th) || !same(a->ph, b->ph) || !same(a->p1, b->p1) || !same(a->p2, b->p2))
            fail("the fast Heun step leaves the strict one's bits", KIND, l, b->l);
          if (!same(a->l, wx[1]) || !same(a->p2, wp[2])) fail("ray_step_heun is not the definition", KIND, l, a->l);
          n += 5;
        }
  return n;
}

template <int KIND>
static unsigned long long rays(const cvk::MetricParams &M) {
  unsigned long long n = 0, beyond = 0;
  for (int r = 0; r < 16; ++r)
    for (long long S : {0ll, 870ll}) {
      std::unique_ptr<cvk::Ray> a(new cvk::Ray()), b(new cvk::Ray());
      a->l = 5.0, a->th = 1.2 + 0.02 * r, a->ph = 0.0, a->p1 = -0.98, a->p2 = 0.4 * (r - 8), a->p3 = 0.3 + 0.1 * r, a->p3sq = a->p3 * a->p3;
      *b = *a;
      const double kappa = S ? cvk::step_kappa(0.1, S) : 0.0; /* S = 0: the kernels' one path, kappa = +0 */
      const bool ok = cvk::metric_fast_ok(KIND, M, 30.0) && cvk::ray_fast_ok(*a);
      for (int k = 0; k < 4096 && std::fabs(a->l) <= 30.0; ++k) {
        std::unique_ptr<double> dk(new double(cvk::step_delta(0.1, kappa, a->l)));
        if (S == 0 && !same(*dk, 0.1)) fail("kappa = +0 does not give delta", KIND, a->l, *dk);
        cvk::Ray stage = *a;
        cvk::ray_step<KIND, true>(M, stage, *dk);
        beyond += std::fabs(stage.l) > 30.0;
        cvk::ray_step_heun<KIND, true, false>(M, *a, *dk, false);
        cvk::ray_step_heun<KIND, true, true>(M, *b, *dk, ok);
        if (std::memcmp(a.get(), b.get(), sizeof(cvk::Ray)) != 0) fail("the fast Heun step leaves the strict one's bits on a ray", KIND, a->l, b->l);
        ++n;
      }
    }
  if (beyond < 8) fail("too few second stages begun beyond the radius", KIND, 0.0, (double)beyond);
  return n;
}

int main() {
  cvk::MetricParams M;
  M.rho = 1.0, M.rho2 = 1.0, M.m = 0.5, M.a = 2.0, M.pim = CV_PI * M.m, M.inv_pim = 1.0 / M.pim, M.two_o_pi = 2.0 / CV_PI;
  M.T = cv_sc_table(), M.LT = cv_log_table(), M.AT = cv_atan_table();
  unsigned long long n = 0;
  n += directed<cvk::METRIC_ELLIS>(M) + directed<cvk::METRIC_INTERSTELLAR>(M) + directed<cvk::METRIC_FLAT>(M);
  n += rays<cvk::METRIC_ELLIS>(M) + rays<cvk::METRIC_INTERSTELLAR>(M);
  std::printf("integrator ok: %llu values\n", n);
  return 0;
}
