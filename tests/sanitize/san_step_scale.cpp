// Stand-alone driver for the host instantiation of cvk::step_delta and of cvk::step_delta_of_scale, the body of the ABI's host accessor
// curvis_step_delta (curvis_amd/csrc/cv_device.h), under option "step_scale"; built with -fsanitize=address,undefined and run by
// tests/test_step_scale_host.py.  Directed inputs: |l| kappa one ulp either side of delta, l = +-0, +-L0, NaN, +-inf, subnormal, a
// scale whose kappa is inexact, S = 1 and S = 2^20, the refusals; then whole rays walked with the scaled step through the strict
// and the fast Euler step.  Every result lives in a heap block of exactly one double.  Prints "step_scale ok: <n> values".
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <memory>

#include "../../curvis_amd/csrc/cv_device.h"

static void fail(const char *what, double delta, long long S, double l, double got) {
  std::fprintf(stderr, "san_step_scale: %s: delta %a, S %lld, l %a: %a\n", what, delta, S, l, got);
  std::exit(1);
}
static bool same(double a, double b) { return std::memcmp(&a, &b, sizeof a) == 0; }

/* the definition, written out: L0 = S / 256, kappa = delta / L0, a = |l| kappa, a > delta ? a : delta */
static double definition(double delta, long long S, double l) {
  if (S == 0) return delta;
  const double L0 = (double)S / 256.0, kappa = delta / L0, a = std::fabs(l) * kappa;
  return a > delta ? a : delta;
}

int main() {
  unsigned long long n = 0;
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  const double deltas[4] = {0.05, 0.0125, 1.0, 0x1p-40};
  const long long scales[7] = {0, 1, 256, 870, 1024, 4097, 1ll << 20};
  for (double delta : deltas)
    for (long long S : scales) {
      const double L0 = S ? (double)S / 256.0 : 1.0;
      double ls[24] = {0.0, -0.0, L0, -L0, nan, inf, -inf, 0x1p-1060, -0x1p-1074, 1.0, -3.0, 100.0, 1e300, -1e300};
      int m = 14;
      /* l with |l| kappa next to delta: L0 and its neighbours, both signs */
      ls[m++] = std::nextafter(L0, 0.0), ls[m++] = std::nextafter(L0, inf), ls[m++] = -std::nextafter(L0, 0.0), ls[m++] = -std::nextafter(L0, inf);
      ls[m++] = std::nextafter(std::nextafter(L0, inf), inf), ls[m++] = std::nextafter(std::nextafter(L0, 0.0), 0.0);
      for (int i = 0; i < m; ++i) {
        std::unique_ptr<double> out(new double(-1.0));
        if (!cvk::step_delta_of_scale(delta, S, ls[i], out.get())) fail("refused", delta, S, ls[i], *out);
        const double want = definition(delta, S, ls[i]);
        if (!same(*out, want)) fail("not the definition", delta, S, ls[i], *out);
        if (!(*out >= delta)) fail("below delta", delta, S, ls[i], *out);
        if (S && !same(cvk::step_delta(delta, cvk::step_kappa(delta, S), ls[i]), want)) fail("step_delta differs", delta, S, ls[i], *out);
        if ((ls[i] != ls[i] || std::fabs(ls[i]) <= std::nextafter(L0, 0.0) || S == 0) && !same(*out, delta)) fail("inside L0 is not delta", delta, S, ls[i], *out);
        ++n;
      }
    }
  { /* refusals: the output is not written */
    std::unique_ptr<double> out(new double(-1.0));
    if (cvk::step_delta_of_scale(0.05, -1, 1.0, out.get()) || cvk::step_delta_of_scale(0.05, (1ll << 20) + 1, 1.0, out.get()) ||
        cvk::step_delta_of_scale(0.0, 1024, 1.0, out.get()) || cvk::step_delta_of_scale(-0.05, 1024, 1.0, out.get()) ||
        cvk::step_delta_of_scale(nan, 1024, 1.0, out.get()) || cvk::step_delta_of_scale(0.05, 1024, 1.0, nullptr) || !same(*out, -1.0))
      fail("a refusal", 0.0, 0, 0.0, *out);
    if (!cvk::step_delta_of_scale(0.0, 0, 1.0, out.get()) || !same(*out, 0.0)) fail("S = 0 hands delta on", 0.0, 0, 1.0, *out);
  }
  /* whole rays: the scaled step through the strict and the fast Euler step (same bits), Ellis and Interstellar */
  cvk::MetricParams M;
  M.rho = 1.0, M.rho2 = 1.0, M.m = 0.5, M.a = 2.0, M.pim = CV_PI * M.m, M.inv_pim = 1.0 / M.pim, M.two_o_pi = 2.0 / CV_PI;
  M.T = cv_sc_table(), M.LT = cv_log_table(), M.AT = cv_atan_table();
  for (int kind = 0; kind < 2; ++kind)
    for (int r = 0; r < 16; ++r) {
      cvk::Ray a = {}, b = {};
      a.l = 5.0, a.th = 1.2 + 0.02 * r, a.ph = 0.0, a.p1 = -0.98, a.p2 = 0.4 * (r - 8), a.p3 = 0.3 + 0.1 * r, a.p3sq = a.p3 * a.p3;
      b = a;
      const double kappa = cvk::step_kappa(0.05, 870);
      const bool ok = cvk::metric_fast_ok(kind, M, 30.0) && cvk::ray_fast_ok(a);
      for (int k = 0; k < 4096 && std::fabs(a.l) <= 30.0; ++k) {
        std::unique_ptr<double> dk(new double(cvk::step_delta(0.05, kappa, a.l)));
        if (kind == 0) {
          cvk::ray_step<cvk::METRIC_ELLIS, true>(M, a, *dk);
          cvk::ray_step_fast<cvk::METRIC_ELLIS, true>(M, b, *dk, ok);
        } else {
          cvk::ray_step<cvk::METRIC_INTERSTELLAR, true>(M, a, *dk);
          cvk::ray_step_fast<cvk::METRIC_INTERSTELLAR, true>(M, b, *dk, ok);
        }
        if (std::memcmp(&a, &b, sizeof a) != 0) fail("the fast step leaves the strict step's bits", 0.05, 870, a.l, b.l);
        ++n;
      }
    }
  std::printf("step_scale ok: %llu values\n", n);
  return 0;
}
