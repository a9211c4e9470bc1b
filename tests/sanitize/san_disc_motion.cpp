// Stand-alone driver for the host instantiation of cvk::disc_shift and cvk::disc_shade (curvis_amd/csrc/cv_device.h), the bodies of the
// ABI's host accessors curvis_disc_shift and curvis_disc_shade; built with -fsanitize=address,undefined and run by
// tests/test_disc_motion_host.py.  Directed inputs: l_hit through the 256 doubles either side of the photon sphere (u_e = 1/2 and its
// neighbours), l_hit <= 0 (the funnel), den driven to 0 and below with an oversized p_phi, G = 0, F large enough to saturate, F tiny,
// NaN and infinity in every argument, channel values 0, 1, 254, 255.  Every result is compared with the definition's steps written out
// through volatiles.  Prints "disc motion ok: <n> values".
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <memory>

#include "../../curvis_amd/csrc/cv_device.h"

static cvk::MetricParams hole(double mass) {
  cvk::MetricParams M;
  M.rho = 1.0, M.rho2 = 1.0, M.m = mass, M.a = 0.0, M.pim = 2.0 * mass, M.inv_pim = 1.0 / M.pim, M.two_o_pi = 2.0 / CV_PI;
  M.T = cv_sc_table(), M.LT = cv_log_table(), M.AT = cv_atan_table();
  return M;
}

static unsigned as_u32(double v) {
  if (!(v == v) || v <= 0.0) return 0u;
  if (v >= 4294967295.0) return 4294967295u;
  return (unsigned)v;
}

/* the definition's steps 1-8, written out */
static double definition(const cvk::MetricParams &M, double l_hit, double l_cam, double sigma, double gain, double p_phi) {
  const volatile double u_e = cvk::schwarzschild_u(M, l_hit), u_c = cvk::schwarzschild_u(M, l_cam);
  const volatile double w = 1.0 + u_e;
  const volatile double n2 = 2.0 * u_e;
  const volatile double n = n2 - 1.0;
  if (!(n > 0.0)) return 0.0;
  const volatile double w2 = 2.0 * w;
  const volatile double a = n / w2;
  const volatile double root = std::sqrt(w2);
  const volatile double wr = w * root;
  const volatile double om = M.inv_pim / wr;
  const volatile double so = sigma * om;
  const volatile double sp = so * p_phi;
  const volatile double den = 1.0 + sp;
  if (!(den > 0.0)) return 0.0;
  const volatile double uc1 = 1.0 + u_c;
  const volatile double A_c = u_c / uc1;
  const volatile double dd = den * den;
  const volatile double ad = A_c * dd;
  const volatile double g2 = a / ad;
  const volatile double g4 = g2 * g2;
  const volatile double F = gain * g4;
  return F;
}
static unsigned shade_definition(unsigned texel, double F) {
  unsigned out = texel & 0xFF000000u;
  for (int k = 0; k < 3; ++k) {
    const volatile double c = (double)((texel >> (8 * k)) & 0xFFu);
    const volatile double cf = c * F;
    const volatile double v = cf + 0.5;
    out |= ((v >= 255.0) ? 255u : as_u32(v)) << (8 * k);
  }
  return out;
}

static unsigned long long n_values = 0, n_zero = 0, n_saturated = 0;
static bool same(double a, double b) { return std::memcmp(&a, &b, 8) == 0 || (a != a && b != b); }
static double one(const cvk::MetricParams &M, double l_hit, double l_cam, double sigma, double gain, double p_phi) {
  std::unique_ptr<double> F(new double(cvk::disc_shift(M, l_hit, l_cam, sigma, gain, p_phi)));
  const double want = definition(M, l_hit, l_cam, sigma, gain, p_phi);
  if (!same(*F, want)) {
    std::fprintf(stderr, "san_disc_motion: F: M %a l_hit %a l_cam %a sigma %a gain %a p_phi %a: %a, definition %a\n", M.m, l_hit, l_cam, sigma, gain, p_phi, *F, want);
    std::exit(1);
  }
  const double viaA = cvk::disc_shift_at(M, l_hit, cvk::disc_camera_factor(M, l_cam), sigma, gain, p_phi);
  if (!same(viaA, want)) {
    std::fprintf(stderr, "san_disc_motion: disc_shift_at over disc_camera_factor differs from disc_shift\n");
    std::exit(1);
  }
  n_zero += want == 0.0;
  const unsigned texels[] = {0xFF000000u, 0x80FF01FEu, 0xFFFEFF00u, 0x8001FE01u, 0xFFFFFFFFu, 0x00000000u, 0xC0804020u};
  for (unsigned t : texels) {
    std::unique_ptr<unsigned> out(new unsigned(cvk::disc_shade(t, want)));
    if (*out != shade_definition(t, want) || (*out >> 24) != (t >> 24)) {
      std::fprintf(stderr, "san_disc_motion: shade: texel %08x F %a: %08x, definition %08x\n", t, want, *out, shade_definition(t, want));
      std::exit(1);
    }
    n_saturated += (t & 0xFFu) != 0xFFu && (*out & 0xFFu) == 0xFFu;
    ++n_values;
  }
  ++n_values;
  return want;
}

int main() {
  const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
  for (double mass : {1.0, 0.37, 1.0 / 1024.0, 4096.0}) {
    const cvk::MetricParams M = hole(mass);
    /* the photon sphere: u = 1/2 at l = 2M (3/2 + ln(1/2)); 256 doubles either side of it */
    double l_ps = 2.0 * mass * (1.5 + std::log(0.5));
    for (int k = 0; k < 256; ++k) l_ps = std::nextafter(l_ps, -inf);
    bool saw_half = false, saw_below = false, saw_above = false;
    for (int k = 0; k < 512; ++k, l_ps = std::nextafter(l_ps, inf)) {
      const double u = cvk::schwarzschild_u(M, l_ps);
      saw_half |= u == 0.5, saw_below |= u == std::nextafter(0.5, 0.0), saw_above |= u == std::nextafter(0.5, 1.0);
      for (double sigma : {1.0, -1.0})
        for (double p : {0.0, 3.0 * mass, -5.19 * mass}) one(M, l_ps, 8.0 * mass, sigma, 1.0, p);
    }
    if (!saw_half || !saw_below || !saw_above) {
      std::fprintf(stderr, "san_disc_motion: the sweep over the photon sphere missed u = 1/2 or a neighbour (M = %a)\n", mass);
      return 1;
    }
    for (double l_hit : {0.0, -0.0, -1.0 * mass, -1e300, 5e-324, 1.7 * mass, 2.0 * mass, 4.0 * mass, 14.0 * mass, 1e6 * mass, 1e300})
      for (double l_cam : {8.0 * mass, 0.0, -3.0 * mass, 2.5 * mass, 1e6 * mass, 1e300})
        for (double sigma : {1.0, -1.0})
          for (double gain : {1.0, 0.0, 0.25, 4.0, 1e300, 5e-324, 1e-300})
            for (double p : {0.0, -0.0, 4.0 * mass, -4.0 * mass, 1e3 * mass, -1e3 * mass, 1e300, -1e300, 5e-324})
              one(M, l_hit, l_cam, sigma, gain, p);
    /* den towards 0 and through it: p_phi = -sigma / om, its neighbours, and twice that */
    for (double l_hit : {1.7 * mass, 3.0 * mass, 10.0 * mass}) {
      const double u = cvk::schwarzschild_u(M, l_hit), w = 1.0 + u;
      const double om = M.inv_pim / (w * std::sqrt(2.0 * w));
      double p = 1.0 / om;
      for (int k = 0; k < 8; ++k) p = std::nextafter(p, 0.0);
      for (int k = 0; k < 16; ++k, p = std::nextafter(p, inf))
        for (double sigma : {1.0, -1.0}) one(M, l_hit, 8.0 * mass, sigma, 1.0, -sigma * p), one(M, l_hit, 8.0 * mass, sigma, 1.0, sigma * p);
      one(M, l_hit, 8.0 * mass, 1.0, 1.0, -2.0 / om);
    }
    /* NaN and infinity in every argument, one at a time and all at once */
    const double base[5] = {4.0 * mass, 8.0 * mass, 1.0, 1.0, 2.0 * mass};
    for (double v : {nan, inf, -inf}) {
      for (int i = 0; i < 5; ++i) {
        double a[5];
        std::memcpy(a, base, sizeof a);
        a[i] = v;
        one(M, a[0], a[1], a[2], a[3], a[4]);
      }
      one(M, v, v, v, v, v);
    }
  }
  /* the colour alone: F at and around every rounding and saturation boundary of the four channel values */
  for (unsigned c : {0u, 1u, 254u, 255u})
    for (double F : {0.0, -0.0, 0.5, 1.0, std::nextafter(1.0, 0.0), std::nextafter(1.0, 2.0), 254.5 / 254.0, 255.0 / 254.0, 254.49, 254.5, 255.0, 1e300, 5e-324, 1e-300, -1.0, inf, -inf, nan}) {
      const unsigned t = 0x80000000u | c | (c << 8) | (c << 16);
      if (cvk::disc_shade(t, F) != shade_definition(t, F)) {
        std::fprintf(stderr, "san_disc_motion: shade: channel %u F %a\n", c, F);
        return 1;
      }
      ++n_values;
    }
  if (n_zero == 0 || n_saturated == 0) {
    std::fprintf(stderr, "san_disc_motion: the inputs reached no F = 0 (%llu) or no saturated channel (%llu)\n", n_zero, n_saturated);
    return 1;
  }
  std::printf("disc motion ok: %llu values, %llu with F = 0, %llu saturated channels\n", n_values, n_zero, n_saturated);
  return 0;
}
