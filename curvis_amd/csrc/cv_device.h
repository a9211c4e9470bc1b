/* cv_device.h -- per-ray device functions of the geodesic hot path (gfx950).
 *
 * One lane owns one ray.  The live state of the forward-Euler loop is five doubles
 * (l, theta, p_l, p_theta and -- only when the caller needs it -- phi) plus the constants
 * p_phi and p_phi^2; t and p_t are dead on this path (dp_t = dp_phi = 0, t is never read:
 * src/metrics.rs:259-264) and are reconstructed on the host for the debug dump.
 *
 * Arithmetic contract: every floating-point operation below is the operation the reference
 * performs, in the reference's order (src/metrics.rs:223-297 for the step), individually
 * rounded; the only fused operations are the explicit fma() calls inside cv_math.h.  The file
 * must be compiled with -ffp-contract=off.  Common sub-expressions are evaluated once
 * (sin/cos(theta), r(l), r^2(l)): they are pure functions of the old state, so the values are
 * identical to the reference's repeated evaluation.
 *
 * Functions are __host__ __device__ so the SAME source can be compiled for x86 by the CPU test
 * suite (tests/host_twin) -- a test vehicle, never a fallback: libcurvis_hip.so only launches
 * the __global__ kernels.
 */
#ifndef CURVIS_CV_DEVICE_H
#define CURVIS_CV_DEVICE_H

#include <math.h>

#include "cv_math.h"

#if defined(__clang__)
#pragma clang fp contract(off)
#endif

namespace cvk {

enum : int { METRIC_ELLIS = 0, METRIC_INTERSTELLAR = 1, METRIC_FLAT = 2, METRIC_SCHWARZSCHILD = 3 };
enum : int { CODE_NONE = 0, CODE_POS = 1, CODE_NEG = -1, CODE_DISC = 2 /* ended on the disc (the DISC kernels) */ };

struct MetricParams {
  double rho;      /* throat radius */
  double rho2;     /* rho*rho (rho.powi(2)) */
  double m, a;     /* Interstellar mass / half-length */
  double pim;      /* PI*m: denominator of scaled_distance (src/metrics.rs:461) */
  double inv_pim;  /* RN(1/(PI*m)) computed on the host: lets the fast step divide by the constant with the
                      three-instruction Markstein sequence (exact for a correctly rounded reciprocal) */
  /* Schwarzschild (m = the mass M; rho and a are ignored): the two slots above hold the kind's own constants, pim = 2M (exact) and
   * inv_pim = RN(1/(2M)), formed once on the host like the reciprocal they replace (make_metric) -- the struct, which is part of
   * every kernel's argument block, keeps its layout */
  double two_o_pi; /* 2.0/PI (src/metrics.rs:481) */
  cv_sc_tab_t T;   /* sin/cos table the per-ray functions read: LDS copy in the hot kernels, cv_sc_table()
                      (host static / device __constant__) everywhere else */
  cv_log_tab_t LT; /* same for cv_log_t and cv_atan_t (Interstellar only) */
  cv_atan_tab_t AT;
};

/* Interstellar metric of the FAST step: x = 2(|l| - a)/(pi m) first, the rest only for x >= 2.
 * Same values as metric_eval below with fewer instructions (each rewrite is exact, not merely close):
 *   2*(|l| - a)       = fma(2, |l|, -2a)          scaling by two commutes with the rounding
 *   xn / (pi m)       Markstein with the host-rounded reciprocal M.inv_pim (exact for a correctly rounded one)
 *   x*at - lg/2       = fma(-0.5, lg, RN(x*at))   lg/2 is exact
 *   (2/pi)*signum(l)*at = copysign(RN(2/pi * at), l)        multiplying by +-1 is exact, at > 0
 * x >= 2 holds for every step outside |l| < a + pi m (a dozen steps of a ray that crosses the throat): it is part of
 * the fast step's guard, so the throat (|l| <= a: r = rho, r' = 0), negative x, NaN and the small-argument forms
 * of atan / log never reach this code -- they take the strict step, i.e. the reference's own branches -- and the
 * fast path carries neither `max(x, 0)` nor a second form of either function. */
CV_HD double interstellar_x(const MetricParams &M, double l) {
  const double xn = CV_FMA(2.0, CV_FABS(l), -2.0 * M.a);
  const double q0 = xn * M.inv_pim;
  return CV_FMA(CV_FMA(-M.pim, q0, xn), M.inv_pim, q0);
}
CV_HD void interstellar_eval_x_ge2(const MetricParams &M, double l, double x, double &r, double &r2, double &rd) {
  const double at = cv_atan_row(cv_div_nr(-1.0, x), M.AT); /* = cv_atan(x) for x >= 2: reciprocal branch, no range test */
  const double lg = cv_log_ge2_t(1.0 + x * x, M.LT);       /* = cv_log(1 + x^2): the k >= 1 formula, no Fast2Sum */
  r = M.rho + M.m * CV_FMA(-0.5, lg, x * at);
  rd = __builtin_copysign(M.two_o_pi * at, l); /* (2/pi * signum(l)) * at: the product by +-1 is exact, and at >= atan 2 > 0
                                                  here, so the sign can be put on afterwards (one v_mul + one v_bfi) */
  r2 = r * r;
}

/* r(l), r^2(l), r'(l): src/metrics.rs:417-421 / 467-485 / 501-505. */
template <int KIND>
CV_HD void metric_eval(const MetricParams &M, double l, double &r, double &r2, double &rd) {
  if (KIND == METRIC_ELLIS) {
    r2 = M.rho2 + l * l;
    r = CV_SQRT(r2);
    rd = l / r;
  } else if (KIND == METRIC_INTERSTELLAR) {
    double al = CV_FABS(l);
    if (al > M.a) {
      const double xn = 2.0 * (al - M.a);
      const double x = xn / M.pim;
      const double at = cv_atan_t(x, M.AT);
      r = M.rho + M.m * (x * at - cv_log_t(1.0 + x * x, M.LT) / 2.0);
      double sg = (cv_bits(l) >> 63) ? -1.0 : 1.0; /* l.signum(), l != NaN-safe below */
      if (l != l) sg = l;
      rd = M.two_o_pi * sg * at;
    } else {
      r = M.rho;
      rd = 0.0;
    }
    r2 = r * r;
  } else if (KIND == METRIC_SCHWARZSCHILD) {
    /* the optical metric of Schwarzschild in the tortoise coordinate (include/curvis_hip.h has the definition; the lines below are
     * its steps in its order).  l < 0 takes the values of l = 0 -- the funnel: R constant, R' < 0 constant, so a ray that has come
     * this far inside the photon sphere keeps falling to -max_radius; -0 gives y = -1 like +0, a NaN stays a NaN */
    const double lc = l < 0.0 ? 0.0 : l;
    const double y = CV_FMA(lc, M.inv_pim, -1.0); /* l / 2M - 1 */
    const double u = cv_tortoise_u(y, M.LT);      /* r / 2M - 1 */
    const double w = 1.0 + u;
    const double sq = CV_SQRT(u * w);
    r = cv_div_nr((M.pim * w) * w, sq);           /* 2M (1 + u)^2 / sqrt(u (1 + u)) */
    rd = cv_div_nr(2.0 * u - 1.0, 2.0 * sq);      /* (2u - 1) / (2 sqrt(u (1 + u))) */
    r2 = r * r;
  } else {
    r = l;
    r2 = l * l;
    rd = 1.0;
  }
}
/* u = r / 2M - 1 of the Schwarzschild kind at radial coordinate l, by the lines above (the host accessor curvis_schwarzschild_u) */
CV_HD double schwarzschild_u(const MetricParams &M, double l) {
  const double lc = l < 0.0 ? 0.0 : l;
  return cv_tortoise_u(CV_FMA(lc, M.inv_pim, -1.0), M.LT);
}

/* r(l) only (photon construction) */
template <int KIND>
CV_HD double metric_r(const MetricParams &M, double l) {
  double r, r2, rd;
  metric_eval<KIND>(M, l, r, r2, rd);
  return r;
}

struct Ray {
  double l, th, ph; /* position (contravariant) */
  double p1, p2;    /* covariant momentum: radial, theta */
  double p3, p3sq;  /* covariant phi momentum (constant of motion) and its square */
};

/* One forward-Euler step given sin/cos(theta): src/metrics.rs:283-297 with :223-244 and :247-270
 * inlined, every division and the square root being the compiler's IEEE-754 operations. */
template <int KIND, bool PHI>
CV_HD void ray_step_core(const MetricParams &M, Ray &q, double delta, double s, double c) {
  double r, r2, rd;
  metric_eval<KIND>(M, q.l, r, r2, rd);
  const double ss = s * s;            /* theta.sin().powi(2) */
  const double g22c = 1.0 / r2;       /* g22.powi(-1) */
  const double dx1 = q.p1;            /* p1 * g11.powi(-1) == p1 * 1.0 */
  const double dx2 = q.p2 * g22c;
  const double b2 = q.p2 * q.p2 + q.p3sq / ss;
  const double dp1 = b2 * rd / (r * (r * r));         /* r.powi(3) */
  const double dp2 = q.p3sq * (c / (r2 * (s * ss)));  /* sin.powi(3) = s*(s*s) */
  if (PHI) {
    const double g33c = 1.0 / (r2 * ss);
    q.ph = q.ph + (q.p3 * g33c) * delta;
  }
  q.l = q.l + dx1 * delta;
  q.th = q.th + dx2 * delta;
  q.p1 = q.p1 + dp1 * delta;
  q.p2 = q.p2 + dp2 * delta;
}

/* WIDE_T: M.T is the 256-row form of the sin/cos table (cv_sincos_tw) */
template <int KIND, bool PHI, bool WIDE_T = false>
CV_HD void ray_step(const MetricParams &M, Ray &q, double delta) {
  double s, c;
  if (WIDE_T)
    cv_sincos_tw(q.th, M.T, &s, &c);
  else
    cv_sincos_t(q.th, M.T, &s, &c);
  ray_step_core<KIND, PHI>(M, q, delta, s, c);
}
/* the same step under a probe that is handed the (sin, cos) of theta before the state moves (ray_step_fast's PROBE has the contract) */
template <int KIND, bool PHI, bool WIDE_T, class PROBE>
CV_HD void ray_step_probed(const MetricParams &M, Ray &q, double delta, const PROBE &probe) {
  double s, c;
  if (WIDE_T)
    cv_sincos_tw(q.th, M.T, &s, &c);
  else
    cv_sincos_t(q.th, M.T, &s, &c);
  probe.sincos(s, c);
  ray_step_core<KIND, PHI>(M, q, delta, s, c);
}

/* Option "step_scale" (include/curvis_hip.h): the step of a ray whose radial coordinate BEFORE the step is l.  kappa = RN(delta / L0)
 * is formed once per call on the host; a = RN(|l| kappa), and the step is a where a > delta, else delta (a NaN l fails the compare and
 * takes delta).  One text for host and device: every integrating loop that honours the option calls it, and curvis_step_delta is
 * its host accessor.  Two FP64 instructions per step and lane: a multiply with an |l| source modifier and a maximum. */
CV_HD double step_kappa(double delta, long long step_scale) { return delta / ((double)step_scale / 256.0); }
CV_HD double step_delta(double delta, double kappa, double l) {
  const double a = CV_FABS(l) * kappa;
  /* (a > delta) ? a : delta, written as the IEEE maximum: the same value in every case -- a > delta gives a, a <= delta gives delta, and
   * a NaN a gives the operand that is a number, delta (delta > 0 is checked on the host, so it is never the NaN) -- and ONE v_max_f64
   * on the device where the compare-select is a v_cmp and two v_cndmask_b32 */
  return __builtin_fmax(a, delta);
}
/* the body of the host accessor curvis_step_delta: kappa as the render calls form it, then step_delta; S = 0 is delta.  false for S
 * outside [0, 2^20], a null `out`, and S != 0 with !(delta > 0) */
constexpr long long kStepScaleMax = 1ll << 20;
CV_HD bool step_delta_of_scale(double delta, long long step_scale, double l, double *out) {
  if (!out || step_scale < 0 || step_scale > kStepScaleMax) return false;
  if (step_scale == 0) {
    *out = delta;
    return true;
  }
  if (!(delta > 0.0)) return false;
  *out = step_delta(delta, step_kappa(delta, step_scale), l);
  return true;
}

/* ------------------------------------------------------------------------------------------------
 * Fast step: the same IEEE results with far fewer instructions.
 *
 * The AMDGPU expansion of an f64 division n/d is  y = rcp(d) + 2 Newton steps;  q0 = n*y;
 * rem = fma(-d, q0, n);  q = fma(rem, y, q0)  (plus div_scale / div_fixup for extreme exponents),
 * and that of sqrt(x) is a Goldschmidt iteration on rsq(x) (plus ldexp scaling below 2^-767).  The
 * final fma of either sequence returns the correctly rounded result for ANY y within a few ulp of
 * 1/d (Markstein), so the five divisions of a step do not each need their own rcp + Newton chain:
 * 1/r^2, 1/r^3 and 1/(r^2 sin^3) are products of ONE refined 1/r (a by-product of the sqrt) and
 * ONE refined 1/sin(theta).  The result of each division is still the individually rounded quotient
 * the reference computes -- correctly rounded unless a rounding boundary lies within
 * (|kappa| + 1)^2 2^-106 (relative) below the exact quotient, y = (1 + kappa 2^-53)/d.  MEASURED on
 * the reciprocals the step really forms (probe hook below; tools/gpu_fast_step_rounding.py ->
 * profiles/round5_fast_step_rounding.txt): |kappa| <= 2 .. 9 (Ellis), <= 6 .. 14
 * (Interstellar), and summed over the quotients of a step 1.0e-15 (Ellis) / 1.9e-15 (Interstellar)
 * expected mis-rounded operations per step = 4e-6 per 1080p frame, 1.5e-2 per configs[4] render; an
 * event is ONE quotient one ulp low (tests/test_gpu_fast_step.py drives it there on purpose).
 *
 * Guards: the shortcut skips div_scale/div_fixup, so it is only taken when every operand is finite,
 * non-zero and far from the exponent limits; any lane failing the guard executes ray_step_core
 * (the compiler's IEEE operations) for that step instead. */
CV_HD double rcp_seed(double x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_rcp(x); /* v_rcp_f64 */
#else
  return 1.0 / x;
#endif
}
CV_HD double rsq_seed(double x) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_rsq(x); /* v_rsq_f64 */
#else
  return 1.0 / CV_SQRT(x);
#endif
}
/* y ~ 1/d to about an ulp: hardware seed (2^-23) + ONE third-order step, y0 (1 + e + e^2) with e = 1 - d y0,
 * i.e. 1/d (1 - e^3): 2^-69 before the final rounding, in three fmas (two Newton steps take four) */
CV_HD double recip_refined(double d) {
  const double y0 = rcp_seed(d);
  const double e = CV_FMA(-d, y0, 1.0);
  const double p = CV_FMA(e, e, e);
  return CV_FMA(y0, p, y0);
}
/* correctly rounded n/d given y ~ 1/d */
CV_HD double div_with_recip(double n, double d, double y) {
  const double q0 = n * y;
  const double rem = CV_FMA(-d, q0, n);
  return CV_FMA(rem, y, q0);
}
/* ---- quotients that share their reciprocal (the per-pixel kernel of the efficient renderer; device only) -------------------------
 * The AMDGPU expansion of an f64 quotient n/d is  y = v_rcp_f64(d) refined by two Newton steps;  q0 = n y;  rem = fma(-d, q0, n);
 * q = fma(rem, y, q0)  -- wrapped in v_div_scale / v_div_fmas / v_div_fixup, which only act when an operand or the quotient is zero,
 * subnormal, infinite, NaN or within 2^-/+768 of the exponent limits, and pass their operands through otherwise.  A pixel forms
 * twelve such quotients, nine of them in groups that share the denominator (v / |v| twice) or divide by a constant of the call (the
 * resolution, pi, 2 pi).  recip_chain is the FIRST HALF of that very sequence -- same instructions, same operand -- and
 * div_with_recip (cv_device.h) its second half, so a quotient formed from a shared y is the quotient the compiler's own expansion
 * returns, operation for operation: nothing is assumed about how close y is to 1/d (unlike the fast Euler step, whose
 * reciprocals are products).  The guards keep every operand inside [2^-300, 2^300), where none of the wrappers acts; a lane outside
 * takes the `/` operator.  The x86 build keeps the operator throughout (its quotients are IEEE by construction); device == twin ==
 * oracle is what the parity tests assert, and tests/test_gpu_fast_step.py puts the helpers themselves on operands whose quotient sits
 * within 2^-106 of a rounding boundary and on every class of special value.  Measured: 914 -> 887 VALU instructions per wave (the
 * guards and their joins give back more than half of what the 36 + 31 + 8 wrapper, Newton and seed instructions save), 0.0559 ->
 * 0.0534 ms per 1080p frame = -4.4 % on one box, interleaved (profiles/round6_eff_pixel_shared_div.txt). */
CV_HD double recip_chain(double d) {
  double y = rcp_seed(d);
  y = CV_FMA(y, CV_FMA(-d, y, 1.0), y);
  return CV_FMA(y, CV_FMA(-d, y, 1.0), y);
}
/* y of the call's constant denominators, formed once per context and resolution by recip_chain ON THE DEVICE (recip_chain_kernel)
 * and handed to the pixel kernel as arguments */
struct PixelRecips {
  double y_res_x, y_res_y, y_pi, y_two_pi;
};
/* v / n for the three components of a vector and its Euclidean norm n (so |v_i| <= n up to rounding: one bound per operand) */
template <bool SHARED>
CV_HD void unit3(const double *v, double n, double *u) {
#if defined(__HIP_DEVICE_COMPILE__)
  if (SHARED) {
    if (n >= 0x1p-300 && n < 0x1p300 && CV_FABS(v[0]) >= 0x1p-300 && CV_FABS(v[1]) >= 0x1p-300 && CV_FABS(v[2]) >= 0x1p-300) {
      const double y = recip_chain(n);
      u[0] = div_with_recip(v[0], n, y);
      u[1] = div_with_recip(v[1], n, y);
      u[2] = div_with_recip(v[2], n, y);
      return;
    }
  }
#endif
  u[0] = v[0] / n;
  u[1] = v[1] / n;
  u[2] = v[2] / n;
}
/* sqrt(x) the same way: the AMDGPU expansion of an f64 square root is v_rsq_f64 and a Goldschmidt / Newton chain of nine
 * operations, wrapped in a scaling by 2^256 for arguments below 2^-767 and a class test that passes zeros and infinities through
 * (v_cmp, v_cndmask, v_ldexp twice, v_cmp_class, two v_cndmask).  Inside [2^-700, 2^700) the wrappers do nothing; the chain below is
 * the compiler's, operation for operation, and a lane outside the range (zero, negative, NaN, ...) takes the operator. */
template <bool SHARED>
CV_HD double sqrt_plain(double x) {
#if defined(__HIP_DEVICE_COMPILE__)
  if (SHARED) {
    if (x >= 0x1p-700 && x < 0x1p700) {
      const double y = rsq_seed(x);
      double g = x * y, h = y * 0.5;
      const double e = CV_FMA(-h, g, 0.5);
      g = CV_FMA(g, e, g);
      h = CV_FMA(h, e, h);
      double d = CV_FMA(-g, g, x);
      g = CV_FMA(d, h, g);
      d = CV_FMA(-g, g, x);
      return CV_FMA(d, h, g);
    }
  }
#endif
  return CV_SQRT(x);
}

/* a / d for a constant d of the call, 2^-300 <= d < 2^300, with y = recip_chain(d):
 * div_index: a is an integer-valued 0 <= a < 2^32 (a pixel index) -- always inside the range, no guard.  (+0: 0 y = +0,
 *            fma(-d, +0, +0) = +0, fma(+0, y, +0) = +0, the IEEE quotient.)
 * div_angle: a is an angle, 0 <= a < 8 or NaN by construction; zero (of either sign), anything below 2^-300 and NaN take the operator. */
template <bool SHARED>
CV_HD double div_index(double a, double d, double y) {
#if defined(__HIP_DEVICE_COMPILE__)
  if (SHARED) return div_with_recip(a, d, y);
#endif
  (void)y;
  return a / d;
}
template <bool SHARED>
CV_HD double div_angle(double a, double d, double y) {
#if defined(__HIP_DEVICE_COMPILE__)
  if (SHARED) {
    if (a >= 0x1p-300 && a < 8.0) return div_with_recip(a, d, y);
  }
#endif
  (void)y;
  return a / d;
}

/* root = sqrt(x) correctly rounded, y ~ 1/sqrt(x) to about an ulp (Goldschmidt on the hardware seed, no
 * scaling).  With g0 = x y0 and E = 1 - g0 y0 (= 1 - x y0^2):  sqrt(x) = g0 (1 - E)^(-1/2) = g0 (1 + E/2 + 3/8 E^2
 * + 5/16 E^3 ...), and the same factor takes y0 to 1/sqrt(x).  One third-order step p = E/2 + 3/8 E^2 brings BOTH
 * to rounding accuracy (seed 2^-23 -> 2^-70 before rounding); the final residual step g + (x - g^2) y/2 then sees
 * the exact residual (fma) and a y good to 2^-53, i.e. a value within ~2^-53 ulp of sqrt(x) before its single
 * rounding.  10 instructions; the compiler's expansion (second-order step, two residual steps with a 2^-45
 * multiplier) plus a reciprocal refinement took 13. */
CV_HD void sqrt_and_rsqrt(double x, double &root, double &y) {
  const double y0 = rsq_seed(x);
  double g = x * y0;
  const double E = CV_FMA(-g, y0, 1.0);
  const double p = E * CV_FMA(0.375, E, 0.5);
  g = CV_FMA(g, p, g);
  y = CV_FMA(y0, p, y0);
  const double d = CV_FMA(-g, g, x);
  root = CV_FMA(d, 0.5 * y, g);
}
/* finite, non-zero, not subnormal (one v_cmp_class_f64) */
CV_HD bool is_normal_number(double v) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __builtin_amdgcn_class(v, 0x108); /* -normal | +normal */
#else
  const uint32_t e = (cv_hi(v) >> 20) & 0x7ffu;
  return e != 0u && e != 0x7ffu;
#endif
}
/* lo_hi <= (high word of |v|) < hi_hi : exponent-range test with two integer ops */
CV_HD bool hi_word_in(double v, uint32_t lo_hi, uint32_t hi_hi) {
  return ((cv_hi(v) & 0x7fffffffu) - lo_hi) < (hi_hi - lo_hi);
}
#define CV_HI_2POW(e) ((uint32_t)(1023 + (e)) << 20)

/* per-ray part of the guard.  p_phi^2 is a constant of the motion; the bounds keep b^2 = p_theta^2 + p_phi^2 /
 * sin^2 >= 2^-300 (the dp_l class test relies on it) and the products away from overflow.  A ray with p_phi == 0
 * exactly -- the middle pixel ROW of an axis-aligned camera: 1920 rays of a 1080p frame -- is served as well:
 * with a zero numerator the shared-reciprocal quotients are exact zeros of the IEEE sign (0 * y = 0, fma(-d, 0, 0)
 * = +0, fma(+0, y, 0) = 0), dp_theta = 0 * q = +-0 adds nothing, so p_theta is a constant of the motion too
 * and b^2 = p_theta^2 is bounded once, here.  (p_theta == 0 as well -- the central pixel -- keeps the strict
 * step.)  Before this, that row executed the IEEE step in every iteration, and the 240 waves holding it were
 * among the last to finish. */
CV_HD bool ray_fast_ok(const Ray &q) {
  if (q.p3sq == 0.0) return hi_word_in(q.p2 * q.p2, CV_HI_2POW(-300), CV_HI_2POW(300));
  return hi_word_in(q.p3sq, CV_HI_2POW(-300), CV_HI_2POW(300));
}

/* host-side part of the guard: metric parameters / escape radius far from the exponent limits */
CV_HD bool metric_fast_ok(int kind, const MetricParams &M, double max_radius) {
  bool ok = hi_word_in(max_radius, CV_HI_2POW(-90), CV_HI_2POW(90));
  if (kind == METRIC_ELLIS) ok = ok && hi_word_in(M.rho, CV_HI_2POW(-90), CV_HI_2POW(90));
  if (kind == METRIC_INTERSTELLAR)
    ok = ok && hi_word_in(M.rho, CV_HI_2POW(-90), CV_HI_2POW(90)) && hi_word_in(M.m, CV_HI_2POW(-90), CV_HI_2POW(90)) &&
         hi_word_in(M.a, CV_HI_2POW(-300), CV_HI_2POW(90)) &&
         /* x = 2(|l| - a)/(pi m) stays finite and far below overflow for every |l| <= max_radius (interstellar_eval_x_ge2
          * takes -1/x of it without range handling) */
         2.0 * max_radius * M.inv_pim < 0x1p200;
  /* Schwarzschild: 2^-90 <= M < 2^88 gives y = l / 2M - 1 < 2^180 for |l| < 2^90 -- every operand of the solver and of the two
   * quotients is a normal number far from the limits -- and 3 sqrt(3) M <= R < max(7.4 M, |l|) < 2^91 */
  if (kind == METRIC_SCHWARZSCHILD) ok = ok && hi_word_in(M.m, CV_HI_2POW(-90), CV_HI_2POW(88));
  return ok;
}

/* Probe hook of the fast step's quotients.  The hot kernels pass none (NoProbe: every call is an empty inline and
 * leaves no instruction); curvis_selftest_fast_step passes a recorder, so that the numerators, denominators and SHARED
 * reciprocals the step really forms -- products of one refined 1/r and one refined 1/sin(theta) -- can be looked at
 * from outside: how far each y is from 1/d decides how often div_with_recip can mis-round.
 * k: 0 r' = l/r (Ellis), 1 1/r^2, 2 p_phi^2/sin^2, 3 dp_l = (b^2 r')/r^3, 4 cos/(r^2 sin^3), 5 1/(r^2 sin^2) (PHI). */
struct NoProbe {
#if defined(__HIPCC__) || defined(__HIP__)
  __host__ __device__
#endif
  inline void rec(int, double, double, double) const {}
};
/* The other thing a probe can be handed: the (sin, cos) of theta that the step evaluates anyway, from whichever branch forms them,
 * BEFORE the step touches the state -- `probe.sincos(s, c)`.  The disc test of the per-pixel kernels lives there (kernels_geodesic.h
 * DiscProbe: the signs of two consecutive cosines say whether the ray crossed the equatorial plane, disc_crossing below).  Only a probe
 * type that says so is asked -- a specialisation of probe_takes_sincos -- so the instantiations under every other probe are compiled
 * from the text they had. */
template <class PROBE>
struct probe_takes_sincos {
  static constexpr bool value = false;
};

/* one Newton step on an approximate reciprocal.  For y within an ulp of 1/d the result is RN(1/d) unless d's
 * significand is all ones (Markstein); with y = RN(1/d) div_with_recip is correctly rounded, not just almost always.
 * Only the CV_CERTIFIED_DIV build (an A/B measurement, tools/gpu_ab.py) calls it inside the step. */
CV_HD double recip_newton(double d, double y) {
  const double e = CV_FMA(-d, y, 1.0);
  return CV_FMA(y, e, y);
}
#ifndef CV_CERTIFIED_DIV
#define CV_CERTIFIED_DIV 0
#endif

/* EQ (the sampling kernel of the efficient renderer only): every photon of compute_escape_angle starts at
 * theta = fl(pi/2) with p_theta = 0 (src/systems.rs:221-230) and keeps that theta for ever, so
 * while theta has exactly those bits the step is taken in its equatorial form: sin = 1 and cos = RN(pi/2 - fl(pi/2))
 * are what cv_sincos returns for this argument, and with s = 1 the generic operations collapse EXACTLY --
 * 1/s = 1, s^2 = s^3 = 1, p_phi^2/s^2 = p_phi^2 (zero remainder), r^2 s^3 = r^2, 1/(r^2 s^2) = 1/r^2 -- so
 * the state is the generic step's bit for bit, with ~40 of ~95 instructions less in the dependency chain of the
 * lone waves these launches consist of.  A ray whose theta has moved takes the generic step (never observed). */
template <int KIND, bool PHI, bool WIDE_T = false, bool EQ = false, class PROBE = NoProbe>
CV_HD void ray_step_fast(const MetricParams &M, Ray &q, double delta, bool lane_ok, const PROBE &probe = PROBE()) {
  double s, c;
  int s_ok;
  const bool eq = EQ && cv_bits(q.th) == 0x3FF921FB54442D18ULL;
  if (eq) {
    s = 1.0;
    c = 6.123233995736766036e-17; /* 0x3C91A62633145C07 */
    s_ok = 1;
  } else {
    s_ok = cv_sincos_guarded(q.th, M.T, WIDE_T ? 1 : 0, &s, &c);
  }
  if constexpr (probe_takes_sincos<PROBE>::value) probe.sincos(s, c);
  /* guard (branch-free, one compare each): sin(theta) and l non-zero, not NaN and far from the underflow
   * limit.  Upper bounds are implied: |sin| <= 1, and a step is only executed for a ray that has not
   * escaped, |l| <= max_radius < 2^90 (metric_fast_ok; an infinite l has escaped, a NaN fails the compare).
   * (The second stage of a Heun step starts from a state nobody tested: ray_step_heun clears lane_ok for it unless |l| < 2^90,
   * which is all that the bounds below use.)
   * The Interstellar step tests x = 2(|l| - a)/(pi m) >= 2 instead of l (false for a NaN l): inside |l| < a + pi m
   * -- the throat and the few steps next to it -- a ray takes the strict step; outside, atan x >= atan 2, so r' is
   * far from zero and from the underflow of the quotient's remainder.
   * cos(theta) needs no test of its own: it is finite iff sin(theta) is, and the cosine of a double is never
   * zero or subnormal. */
  const double x_i = KIND == METRIC_INTERSTELLAR ? interstellar_x(M, q.l) : 0.0;
  const bool ok = (int)lane_ok & s_ok & (int)(KIND == METRIC_INTERSTELLAR ? x_i >= 2.0 : CV_FABS(q.l) > 0x1p-100);
  if (!ok) {
    ray_step_core<KIND, PHI>(M, q, delta, s, c);
    return;
  }
  double r, r2, rd, y_r, y_s;
  if (KIND == METRIC_ELLIS) {
    r2 = M.rho2 + q.l * q.l;
    sqrt_and_rsqrt(r2, r, y_r);
    if (CV_CERTIFIED_DIV) y_r = recip_newton(r, y_r);
    probe.rec(0, q.l, r, y_r);
    rd = div_with_recip(q.l, r, y_r);
    y_s = recip_refined(s);
  } else {
    if (KIND == METRIC_INTERSTELLAR)
      interstellar_eval_x_ge2(M, q.l, x_i, r, r2, rd);
    else
      metric_eval<KIND>(M, q.l, r, r2, rd);
    /* no square root here, so 1/r would need a seed of its own: ONE v_rcp_f64 (a quarter-rate instruction) serves
     * both reciprocals -- y ~ 1/(r s), 1/r ~ y s, 1/s ~ y r (each ~1.5 ulp; the quotients below stay correctly
     * rounded, see div_with_recip).  r s cannot leave the normal range: 2^-90 < r < 2^91 and |s| > 2^-60. */
    if (eq) {
      y_r = recip_refined(r);
      y_s = 1.0;
    } else {
      const double y_rs = recip_refined(r * s);
      y_r = y_rs * s;
      y_s = y_rs * r;
    }
  }
  if (eq) { /* s == 1: see above; same operations as below with the factors that are exactly 1 left out */
    const double y_r2e = y_r * y_r;
    const double g22e = div_with_recip(1.0, r2, y_r2e);
    const double b2e = q.p2 * q.p2 + q.p3sq;
    const double nume = b2e * rd;
    const double r3e = r * (r * r);
    double dp1e = div_with_recip(nume, r3e, y_r2e * y_r);
    if (!is_normal_number(dp1e)) {
#if defined(__HIP_DEVICE_COMPILE__)
      asm volatile("; IEEE division for dp_l (equatorial step)");
#endif
      dp1e = nume / r3e;
    }
    const double dp2e = q.p3sq * div_with_recip(c, r2, y_r2e);
    if (PHI) q.ph = q.ph + (q.p3 * g22e) * delta;
    q.l = q.l + q.p1 * delta;
    q.th = q.th + (q.p2 * g22e) * delta;
    q.p1 = q.p1 + dp1e * delta;
    q.p2 = q.p2 + dp2e * delta;
    return;
  }
  double y_r2 = y_r * y_r;
  double y_ss = y_s * y_s;
  const double ss = s * s;
  if (CV_CERTIFIED_DIV) {
    y_r2 = recip_newton(r2, y_r2);
    y_ss = recip_newton(ss, y_ss);
  }
  probe.rec(1, 1.0, r2, y_r2);
  const double g22c = div_with_recip(1.0, r2, y_r2);
  const double dx1 = q.p1;
  const double dx2 = q.p2 * g22c;
  probe.rec(2, q.p3sq, ss, y_ss);
  const double b2 = q.p2 * q.p2 + div_with_recip(q.p3sq, ss, y_ss);
  const double num = b2 * rd;
  const double r3 = r * (r * r);
  double y_r3 = y_r2 * y_r;
  if (CV_CERTIFIED_DIV) y_r3 = recip_newton(r3, y_r3);
  probe.rec(3, num, r3, y_r3);
  /* dp_l = num / r^3: the shared-reciprocal quotient is checked AFTERWARDS with one class test.  Inside the guarded
   * domain a non-zero num has |num| >= 2^-300 |r'| >= 2^-745 (Ellis: |r'| = |l|/r >= 2^-191; Interstellar:
   * |r'| >= (2/pi) atan 2), hence the remainder fma cannot underflow and the true quotient
   * is a normal number (>= 2^-745 / 2^273) or overflows.  Whatever else can happen shows in the result: an
   * overflowing n*y or a non-finite num (|p_theta| exploding at a pole) gives inf or NaN; those are "not a normal
   * number" and take the IEEE division. */
  double dp1 = div_with_recip(num, r3, y_r3);
  if (!is_normal_number(dp1)) {
#if defined(__HIP_DEVICE_COMPILE__)
    asm volatile("; IEEE division for dp_l"); /* not speculatable: keeps this a branch around ~25 instructions
                                                 (as a select they would run in every step) */
#endif
    dp1 = num / r3;
  }
  const double r2s3 = r2 * (s * ss);
  double y_r2s3 = y_r2 * (y_ss * y_s);
  if (CV_CERTIFIED_DIV) y_r2s3 = recip_newton(r2s3, y_r2s3);
  probe.rec(4, c, r2s3, y_r2s3);
  const double dp2 = q.p3sq * div_with_recip(c, r2s3, y_r2s3);
  if (PHI) {
    double y_g33 = y_r2 * y_ss;
    if (CV_CERTIFIED_DIV) y_g33 = recip_newton(r2 * ss, y_g33);
    probe.rec(5, 1.0, r2 * ss, y_g33);
    const double g33c = div_with_recip(1.0, r2 * ss, y_g33);
    q.ph = q.ph + (q.p3 * g33c) * delta;
  }
  q.l = q.l + dx1 * delta;
  q.th = q.th + dx2 * delta;
  q.p1 = q.p1 + dp1 * delta;
  q.p2 = q.p2 + dp2 * delta;
}

/* Option "integrator" = 1 (include/curvis_hip.h): one step of Heun's method, the explicit trapezoid, written as a composition of the
 * Euler step E this file already has:  y + delta/2 (f(y) + f(y + delta f(y))) = 1/2 (y + E(E(y, delta), delta)).  The state is saved,
 * the step is taken twice with the SAME delta (under "step_scale" the caller forms it once, from l before the step), and every
 * integrated component becomes (saved + twice-stepped) * 0.5: one IEEE add, one exact halving.  p_phi is a constant of the step and
 * is not touched.  One text for host and device: every integrating loop that honours the option calls it, and curvis_heun_step is its
 * host accessor (FAST = false there).
 *
 * The guard of the fast step, re-read for stage states.  ray_step_fast's bounds rest on "a step is only executed FROM a state with
 * |l| <= max_radius < 2^90" (metric_fast_ok).  The first stage starts from y_k, which has passed the escape test, so nothing changes for
 * it.  The second stage starts from y' = E(y_k), which is tested by nobody: |l'| = |l + p_l delta_k| lies beyond max_radius on the last
 * step of almost every escaping ray, and p_l has no bound from the host.  So the second stage carries a per-lane test of its own,
 * |l'| < 2^90 (false for a NaN and for an infinity), and a lane that fails it takes the strict step, which is always right.  With it
 * every statement of the guard holds for a stage state by the argument that held for a step state, because each of them used only
 * |l| < 2^90 and never max_radius itself:
 *   r^3 < 2^273:  Ellis r^2 = rho^2 + l^2 < 2^181; Interstellar r = rho + m (x atan x - log(1 + x^2)/2) <= rho + m x pi/2 = rho + |l| - a
 *     < 2^91; flat r = l.
 *   the dp_l class test:  a non-zero numerator is >= 2^-300 |r'|, with |r'| = |l|/r >= 2^-100 / 2^91 (Ellis; the lower bound on |l| is
 *     tested inside the step, per stage) or >= (2/pi) atan 2 (Interstellar, x >= 2 tested inside the step, per stage).
 *   2 max_radius inv_pim < 2^200:  it keeps x = 2(|l| - a)/(pi m) far below overflow; m >= 2^-90 gives inv_pim < 2^90, so
 *     |l| < 2^90 alone gives x < 2^181.
 * One v_cmp_lt_f64 with an |l| modifier and one scalar and per Heun step.  Almost every lane passes (2^90 is not a radius any scene
 * has), so the second stage of a last step is a fast step like the others.
 *
 * EQ (the samplers' equatorial shortcut): a ray that keeps theta = fl(pi/2) through both stages keeps it through the average, since
 * (theta + theta) * 0.5 is exact; a ray whose theta moved in a stage takes the generic step from then on, as under Euler.
 *
 * The stages call ray_step_fast under a probe type of their own, HeunStage (as empty as NoProbe): an instantiation apart from the one
 * the Euler loops call.  With the same instantiation the compiler's inliner, which weighs a function by all of its callers, compiled
 * the Interstellar direct, escape-angle and sampler kernels of the EULER step with two instructions in another order. */
struct HeunStage : NoProbe {};
/* STAGE1: the probe of the first stage (FAST only) -- the disc test is handed that stage's (sin, cos), those of the state the step starts
 * from; stage states are never looked at */
template <int KIND, bool PHI, bool FAST, bool WIDE_T = false, bool EQ = false, class STAGE1 = HeunStage>
CV_HD void ray_step_heun(const MetricParams &M, Ray &q, double delta, bool lane_ok, const STAGE1 &stage1 = STAGE1()) {
  const double l0 = q.l, th0 = q.th, p10 = q.p1, p20 = q.p2;
  [[maybe_unused]] const double ph0 = PHI ? q.ph : 0.0;
  if (FAST) {
    ray_step_fast<KIND, PHI, WIDE_T, EQ, STAGE1>(M, q, delta, lane_ok, stage1);
    ray_step_fast<KIND, PHI, WIDE_T, EQ, HeunStage>(M, q, delta, lane_ok && CV_FABS(q.l) < 0x1p90);
  } else {
    ray_step<KIND, PHI, WIDE_T>(M, q, delta);
    ray_step<KIND, PHI, WIDE_T>(M, q, delta);
  }
  q.l = (l0 + q.l) * 0.5;
  q.th = (th0 + q.th) * 0.5;
  if (PHI) q.ph = (ph0 + q.ph) * 0.5;
  q.p1 = (p10 + q.p1) * 0.5;
  q.p2 = (p20 + q.p2) * 0.5;
}
/* x[0] of the debug dump over one Heun step: the reference's line t + (p_t g^tt) delta with p_t = 1, g^tt = -1, twice, then averaged */
CV_HD double heun_time(double t, double delta) {
  const double t2 = (t + (1.0 * -1.0) * delta) + (1.0 * -1.0) * delta;
  return (t + t2) * 0.5;
}

/* the body of the host accessor curvis_heun_step: one Heun step of all eight components of (x, p_cov) in place, with the IEEE form of
 * the step (ray_step; the fast step returns the same bits).  x[0] takes the reference's line x0 + (p0 g00^-1) delta through both
 * stages and is averaged like the others; p[0] and p[3] are constants of the step and keep their bits. */
template <int KIND>
CV_HD void heun_step_all(const MetricParams &M, double x[4], double p[4], double delta) {
  Ray q;
  q.l = x[1], q.th = x[2], q.ph = x[3];
  q.p1 = p[1], q.p2 = p[2], q.p3 = p[3];
  q.p3sq = q.p3 * q.p3;
  ray_step_heun<KIND, true, false>(M, q, delta, false);
  const double t2 = (x[0] + (p[0] * (1.0 / -1.0)) * delta) + (p[0] * (1.0 / -1.0)) * delta;
  x[0] = (x[0] + t2) * 0.5;
  x[1] = q.l, x[2] = q.th, x[3] = q.ph;
  p[1] = q.p1, p[2] = q.p2;
}

struct CameraParams {
  double pos[4];
  double rot[9];
  double focal, sensor_w, sensor_h;
  double res_x, res_y; /* as f64 */
};

CV_HD void mat3_vec(const double *m, double v0, double v1, double v2, double &o0, double &o1, double &o2) {
  /* nalgebra gemv: ((m_i0*x0) + m_i1*x1) + m_i2*x2 */
  o0 = (m[0] * v0 + m[1] * v1) + m[2] * v2;
  o1 = (m[3] * v0 + m[4] * v1) + m[5] * v2;
  o2 = (m[6] * v0 + m[7] * v1) + m[8] * v2;
}

/* ---- option "projection": pixel -> UN-NORMALISED camera-space vector (x forward, y left, z up), the one place where the three
 * renderers and the host accessor form it (include/curvis_hip.h has the definition; every operation below is one of its steps, in
 * its order).  0 is outward_vector_on_camera_space (src/cameras.rs:150-164) expression for expression; 1 and 2 sample the pixel at
 * its centre, u = (2 px + 1) / (2 res_x): with SHARED (the efficient pixel kernel) that quotient is formed as (px + 0.5) / res_x --
 * the same real number, px + 0.5 exact below 2^32 -- from the call's shared reciprocal, under div_index's contract.  sin and cos are
 * cv_math.h's on the constant table (host and device agree bit for bit); sqrt and the other quotients are the IEEE operators.
 * `projection` is uniform over a launch, so the switch is a scalar branch; nothing of it is live once the vector is formed.  Always inlined:
 * its callers with a constant projection 0 are then compiled from the text they had before this function existed. */
enum { PROJ_PERSPECTIVE = 0, PROJ_EQUIRECTANGULAR = 1, PROJ_FISHEYE = 2 };
template <bool SHARED = false>
__attribute__((always_inline)) CV_HD void camera_pixel_vector(const CameraParams &C, int projection, unsigned px, unsigned py, double &vx, double &vy, double &vz,
                                                              const PixelRecips *R = nullptr) {
  if (projection == PROJ_PERSPECTIVE) {
    const double h = 0.5 - (SHARED ? div_index<SHARED>((double)py, C.res_y, R->y_res_y) : (double)py / C.res_y);
    const double w = (SHARED ? div_index<SHARED>((double)px, C.res_x, R->y_res_x) : (double)px / C.res_x) - 0.5;
    vx = C.focal * 1.0;
    vy = -C.sensor_w * w;
    vz = C.sensor_h * h;
    return;
  }
  const double pu = SHARED ? div_index<SHARED>((double)px + 0.5, C.res_x, R->y_res_x) : (2.0 * (double)px + 1.0) / (2.0 * C.res_x);
  const double pv = SHARED ? div_index<SHARED>((double)py + 0.5, C.res_y, R->y_res_y) : (2.0 * (double)py + 1.0) / (2.0 * C.res_y);
  if (projection == PROJ_EQUIRECTANGULAR) {
    const double psi = (0.5 - pu) * (2.0 * CV_PI);
    const double th = pv * CV_PI;
    double st, ct, sp, cp;
    cv_sincos(th, &st, &ct);
    cv_sincos(psi, &sp, &cp);
    vx = st * cp;
    vy = st * sp;
    vz = ct;
    return;
  }
  /* equidistant fisheye: image radius = focal * angle from the axis */
  const double ys = -C.sensor_w * (pu - 0.5);
  const double zs = C.sensor_h * (0.5 - pv);
  const double rho = CV_SQRT(ys * ys + zs * zs);
  if (rho == 0.0) { /* the centre pixel of an odd x odd frame */
    vx = 1.0;
    vy = 0.0;
    vz = 0.0;
    return;
  }
  const double b = rho / C.focal;
  double sb, cb;
  cv_sincos(b, &sb, &cb);
  vx = cb;
  vy = sb * (ys / rho);
  vz = sb * (zs / rho);
}

/* ---- the moving camera (curvis_ctx_set_camera_velocities; include/curvis_hip.h has the definition, the lines below are its steps in
 * its order, every operation one rounded FP64 operation).  A frame's velocity becomes five doubles once per frame on the host
 * (camera_boost_prepare); camera_boost then turns the un-normalised camera-space vector of a pixel of the MOVING camera into that of
 * the static observer at the same place, between camera_pixel_vector and the normalisation that follows it.  Nothing else of a
 * renderer knows about the motion.  The kernels that hold it are the PROJ = 1 ones: their `projection` argument carries PROJ_BOOSTED
 * on top of the projection's number, a launch-uniform bit, so the boost sits behind a scalar branch and a call without a velocity
 * runs the instructions it ran before. */
enum { PROJ_BOOSTED = 0x100, PROJ_KIND_MASK = 0xFF };
struct CameraBoost {
  double u[3]; /* the camera-space direction of travel */
  double A, B; /* gamma - 1 and gamma beta; B == 0 says "not boosted" (a boosted frame has B > 0) */
};
/* rot: the camera's 3 x 3, row-major; beta: (b_l, b_theta, b_phi).  Returns 1 boosted, 0 not boosted (K all zeros), -1 for a speed that
 * is not below 1 (a NaN included) */
CV_HD int camera_boost_prepare(const double *rot, const double *beta, CameraBoost &K) {
  double c[3];
  for (int i = 0; i < 3; ++i) c[i] = ((rot[i] * beta[0]) + rot[3 + i] * beta[1]) + rot[6 + i] * beta[2];
  const double b2 = (c[0] * c[0] + c[1] * c[1]) + c[2] * c[2];
  K.u[0] = K.u[1] = K.u[2] = K.A = K.B = 0.0;
  if (b2 == 0.0) return 0;
  if (!(b2 < 1.0)) return -1;
  const double b = CV_SQRT(b2), g = 1.0 / CV_SQRT(1.0 - b2);
  for (int i = 0; i < 3; ++i) K.u[i] = c[i] / b;
  K.A = g - 1.0;
  K.B = g * b;
  return 1;
}
/* SHARED (the efficient pixel kernel): the square root is sqrt_plain's, which returns the correctly rounded root like the operator;
 * the rest is products and sums */
template <bool SHARED = false>
__attribute__((always_inline)) CV_HD void camera_boost(const CameraBoost &K, double &vx, double &vy, double &vz) {
  if (K.B == 0.0) return; /* a frame at rest in a call whose other frames move: its vector keeps its bits, the sign of a zero included */
  const double n = sqrt_plain<SHARED>((vx * vx + vy * vy) + vz * vz);
  const double p = (vx * K.u[0] + vy * K.u[1]) + vz * K.u[2];
  const double s = K.A * p - K.B * n;
  vx = vx + K.u[0] * s;
  vy = vy + K.u[1] * s;
  vz = vz + K.u[2] * s;
}

/* pixel -> photon: src/cameras.rs:150-172 then src/metrics.rs:301-334; projection: camera_pixel_vector above, with PROJ_BOOSTED on top
 * while the frame has a velocity (B: its CameraBoost, read only then) */
template <int KIND, bool BOOST = false> /* BOOST: the instantiation the PROJ = 1 kernels call; the other is the function it was, text for text */
CV_HD void ray_init(const MetricParams &M, const CameraParams &C, unsigned px, unsigned py, Ray &q, int projection = PROJ_PERSPECTIVE,
                    const CameraBoost *B = nullptr) {
  double vx, vy, vz;
  camera_pixel_vector(C, BOOST ? projection & PROJ_KIND_MASK : projection, px, py, vx, vy, vz);
  if constexpr (BOOST)
    if (projection & PROJ_BOOSTED) camera_boost(*B, vx, vy, vz);
  double n = CV_SQRT(vx * vx + vy * vy + vz * vz); /* Vector3::normalize */
  vx = vx / n;
  vy = vy / n;
  vz = vz / n;
  double d0, d1, d2;
  mat3_vec(C.rot, vx, vy, vz, d0, d1, d2);
  n = CV_SQRT(d0 * d0 + d1 * d1 + d2 * d2); /* direction.normalize() in new_photon */
  d0 = d0 / n;
  d1 = d1 / n;
  d2 = d2 / n;
  const double r = metric_r<KIND>(M, C.pos[1]);
  q.l = C.pos[1];
  q.th = C.pos[2];
  q.ph = C.pos[3];
  q.p1 = d0;
  q.p2 = d1 * r;
  q.p3 = d2 * r * cv_sin_t(C.pos[2], M.T);
  q.p3sq = q.p3 * q.p3;
}

/* photon from an explicit tangent-space direction (compute_escape_angle, src/systems.rs:221-230) */
template <int KIND>
CV_HD void ray_init_dir(const MetricParams &M, const double pos[4], double dx, double dy, double dz, Ray &q) {
  double n = CV_SQRT(dx * dx + dy * dy + dz * dz);
  double d0 = dx / n, d1 = dy / n, d2 = dz / n;
  const double r = metric_r<KIND>(M, pos[1]);
  q.l = pos[1];
  q.th = pos[2];
  q.ph = pos[3];
  q.p1 = d0;
  q.p2 = d1 * r;
  q.p3 = d2 * r * cv_sin_t(pos[2], M.T);
  q.p3sq = q.p3 * q.p3;
}

/* final photon -> tangent-space direction: src/metrics.rs:339-349 (+ :190-203).
 * z uses frame_field_22 (no sin theta), exactly as line 347. */
template <int KIND>
CV_HD void ray_direction(const MetricParams &M, const Ray &q, double &d0, double &d1, double &d2) {
  double r, r2, rd;
  metric_eval<KIND>(M, q.l, r, r2, rd);
  const double s = cv_sin_t(q.th, M.T);
  const double g22c = 1.0 / r2;
  const double g33c = 1.0 / (r2 * (s * s));
  const double v1 = q.p1; /* * 1.0 */
  const double v2 = q.p2 * g22c;
  const double v3 = q.p3 * g33c;
  d0 = v1; /* * frame_field_11 = 1.0 */
  d1 = v2 * r;
  d2 = v3 * r;
}

CV_HD unsigned rust_as_u32(double v) { /* `as u32`: NaN -> 0, saturating */
#if defined(__HIP_DEVICE_COMPILE__)
  unsigned r; /* v_cvt_u32_f64 IS that conversion: truncation, NaN and negatives to 0, 2^32 and above to 0xFFFFFFFF -- one instruction
                 instead of three compares and their selects (tests/test_gpu_fast_step.py checks it on every class of value) */
  asm("v_cvt_u32_f64 %0, %1" : "=v"(r) : "v"(v));
  return r;
#endif
  if (!(v == v)) return 0u;
  if (v <= 0.0) return 0u;
  if (v >= 4294967295.0) return 4294967295u;
  return (unsigned)v;
}

/* f64::rem_euclid(a, b) for b > 0.  On this path |a| < b always holds (a is an atan2 result
 * against 2*pi, or 0.5 - phi/(2*pi) against 1), where fmod(a, b) == a exactly; the general
 * branch keeps the function total. */
CV_HD double rem_euclid_pos(double a, double b) {
  double r;
  if (CV_FABS(a) < b || a != a) {
    r = a;
  } else {
    r = fmod(a, b);
  }
  return (r < 0.0) ? r + b : r;
}

/* ---- the accretion disc (include/curvis_hip.h has the definition; the lines below are its steps 1-7 in its order, every operation
 * individually rounded, no fma of their own).  Between two consecutive states of a ray -- (c_prev, l_prev, ph_prev) of y_{k-1}, (s_cur, c_cur,
 * l_cur, ph_cur) of y_k, s and c being the sincos evaluation of theta the step from that state performs anyway -- did the ray cross the
 * plane theta = pi/2 (mod pi) at a radial coordinate inside [l_in, l_out], and at which texel of a w x h texture?  One text for host and
 * device: the per-pixel kernels call it inside their rarely taken crossing branch, curvis_disc_crossing is its host accessor.  The
 * quotients are the correctly rounded ones: t and the column's through cv_div_nr (operands a cosine apart resp. an angle below 2 pi
 * over a constant: far inside the range where its Markstein form is exact), the row's through the operator, whose operands are the
 * caller's bounds and may sit anywhere in the exponent range.  A NaN anywhere fails the range compare. */
/* disc_crossing_at hands out step 3's l_hit as well (written where the crossing is on the disc): the emission shift below needs it. */
CV_HD bool disc_crossing_at(double c_prev, double c_cur, double s_cur, double l_prev, double l_cur, double ph_prev, double ph_cur, double l_in,
                            double l_out, unsigned w, unsigned h, unsigned *tx, unsigned *ty, double *l_at) {
  if ((c_prev < 0.0) == (c_cur < 0.0)) return false;                    /* 1 */
  const double t = cv_div_nr(c_prev, c_prev - c_cur);                   /* 2 */
  const double dl = l_cur - l_prev, dph = ph_cur - ph_prev;
  const double l_hit = l_prev + t * dl;                                 /* 3 */
  double ph_hit = ph_prev + t * dph;
  if (!(l_in <= l_hit && l_hit <= l_out)) return false;                 /* 4 */
  if (s_cur < 0.0) ph_hit = ph_hit + CV_PI;                             /* 5 */
  const double TWO_PI = 2.0 * CV_PI;
  const unsigned x = rust_as_u32(cv_div_nr(rem_euclid_pos(ph_hit, TWO_PI), TWO_PI) * (double)w); /* 6 */
  const unsigned y = rust_as_u32(((l_hit - l_in) / (l_out - l_in)) * (double)h);                 /* 7 */
  *tx = x < w - 1u ? x : w - 1u;
  *ty = y < h - 1u ? y : h - 1u;
  *l_at = l_hit;
  return true;
}
CV_HD bool disc_crossing(double c_prev, double c_cur, double s_cur, double l_prev, double l_cur, double ph_prev, double ph_cur, double l_in,
                         double l_out, unsigned w, unsigned h, unsigned *tx, unsigned *ty) {
  double l_hit;
  return disc_crossing_at(c_prev, c_cur, s_cur, l_prev, l_cur, ph_prev, ph_cur, l_in, l_out, w, h, tx, ty, &l_hit);
}

/* ---- the disc's emission shift (include/curvis_hip.h has the definition; the lines below are its steps 1-8 in its order, every operation
 * individually rounded, no fma).  One text for host and device: the DISC = 2 kernels call disc_shift_at and disc_shade inside the
 * crossing branch, at the moment a lane gets its texel; curvis_disc_shift and curvis_disc_shade are the host accessors.  The camera's
 * half of the ratio (steps 1 and 6 for l_camera) depends on the frame alone: the host evaluates disc_camera_factor once per frame and
 * the kernels read the result, so no lane solves the tortoise equation a second time.
 * The quotients are the correctly rounded ones.  Steps 3, 4 and 6 through the operator: their operands scale with the caller's l and M
 * (w grows like l / 2M, the numerator of step 4 is 1/2M itself) and may sit anywhere in the exponent range.  Step 7 through cv_div_nr:
 * behind steps 2 and 5, a = n / 2w lies in [2^-55, 1) (n >= one ulp of 1 where it is positive, and then w is next to 3/2; a -> 1 for
 * large w), A_c in [0.21, 1] (u >= 0.278, the root of u + ln u = -1, at every l) and den in [2^-53, 2] for the p_phi of a traced ray, so
 * the divisor lies in [2^-109, 4] and the quotient in [2^-57, 2^112]: far inside the range where its Markstein form is exact. */
CV_HD double disc_camera_factor(const MetricParams &M, double l_camera) {
  const double u_c = schwarzschild_u(M, l_camera);                      /* 1 */
  return u_c / (1.0 + u_c);                                             /* 6 */
}
/* sigma is the motion as a double, +1.0 or -1.0: the product sigma * om is exact */
CV_HD double disc_shift_at(const MetricParams &M, double l_hit, double A_c, double sigma, double gain, double p_phi) {
  const double u_e = schwarzschild_u(M, l_hit);                         /* 1 */
  const double w = 1.0 + u_e, n = 2.0 * u_e - 1.0;                      /* 2 */
  if (!(n > 0.0)) return 0.0;
  const double a = n / (2.0 * w);                                       /* 3 */
  const double om = M.inv_pim / (w * CV_SQRT(2.0 * w));                 /* 4 */
  const double den = 1.0 + (sigma * om) * p_phi;                        /* 5 */
  if (!(den > 0.0)) return 0.0;
  const double g2 = cv_div_nr(a, A_c * (den * den));                    /* 7 */
  return gain * (g2 * g2);                                              /* 8 */
}
CV_HD double disc_shift(const MetricParams &M, double l_hit, double l_camera, double sigma, double gain, double p_phi) {
  return disc_shift_at(M, l_hit, disc_camera_factor(M, l_camera), sigma, gain, p_phi);
}
/* the colour: the three channels of an RGBA8 texel scaled by F and rounded to nearest, saturating; alpha kept */
CV_HD unsigned disc_shade(unsigned texel, double F) {
  unsigned out = texel & 0xFF000000u;
  for (int k = 0; k < 3; ++k) {
    const double v = (double)((texel >> (8 * k)) & 0xFFu) * F + 0.5;
    const unsigned c = (v >= 255.0) ? 255u : rust_as_u32(v);
    out |= c << (8 * k);
  }
  return out;
}

struct SkyParams {
  const unsigned *texels; /* RGBA8 packed little-endian, row-major */
  unsigned w, h;
  double inv_rot[9];
};

/* direction -> texel indices: src/images.rs:132-142 -> src/algebra.rs:128-134 -> :106-116 ->
 * src/images.rs:115-121.  Returns raw `as u32` indices (may equal w / h: reference panics). */
template <bool SHARED = false> /* SHARED (device, the efficient renderer's pixel kernel): theta / pi and phi / 2 pi through the call's
                                  precomputed reciprocals -- div_angle above */
CV_HD void sky_indices(const SkyParams &S, double d0, double d1, double d2, unsigned &tx, unsigned &ty, double y_pi = 0.0,
                       double y_two_pi = 0.0) {
  double w0, w1, w2;
  mat3_vec(S.inv_rot, d0, d1, d2, w0, w1, w2);
  const double rn = sqrt_plain<SHARED>(w0 * w0 + w1 * w1 + w2 * w2);
  double theta = cv_acos(w2 / rn);
  double phi = cv_atan2(w1, w0);
  const double TWO_PI = 2.0 * CV_PI;
  /* normalize_theta_phi #1 (theta_phi_from_vector3) and #2 (pixel_indexes...) */
  for (int k = 0; k < 2; ++k) {
    if (theta < 0.0) {
      theta = CV_FABS(theta);
      phi = phi + CV_PI;
    }
    phi = rem_euclid_pos(phi, TWO_PI);
  }
  ty = rust_as_u32(div_angle<SHARED>(theta, CV_PI, y_pi) * (double)S.h);
  tx = rust_as_u32(rem_euclid_pos(0.5 - div_angle<SHARED>(phi, TWO_PI, y_two_pi), 1.0) * (double)S.w);
}

/* ---- option "sky_filter" = 1: bilinear lookup (include/curvis_hip.h has the definition; the numbers below are its steps).
 * The four texels a ray blends and their 8-bit weights, from the indices sky_indices returns on the virtual sky of 256 w x 256 h
 * texels: scaling by 2^8 commutes with every rounding, so X >> 8, Y >> 8 are sky_indices' raw tx, ty bit for bit and the filter costs
 * no FP64 operation of its own.  Needs w, h <= 2^23 (checked on the host: 256 w must stay a u32). */
struct SkyTaps {
  unsigned x0, x1, y0, y1; /* columns and rows of the four texels, all inside the sky */
  unsigned fx, fy;         /* weights of x1 and y1, 0..255 (those of x0 and y0: 256 - fx, 256 - fy) */
  unsigned tx, ty;         /* X >> 8, Y >> 8: the nearest lookup's raw indices */
  bool oob;                /* tx >= w or ty >= h: the rays the nearest lookup counts in n_oob */
};
template <bool SHARED = false>
CV_HD void sky_bilinear_taps(const SkyParams &S, double d0, double d1, double d2, SkyTaps &t, double y_pi = 0.0, double y_two_pi = 0.0) {
  const unsigned fine_w = S.w << 8, fine_h = S.h << 8;
  SkyParams F = S; /* 1: the same lookup, the same orientation, 256 times the size; texels are not read */
  F.w = fine_w;
  F.h = fine_h;
  unsigned X, Y;
  sky_indices<SHARED>(F, d0, d1, d2, X, Y, y_pi, y_two_pi);
  t.tx = X >> 8; /* 2 */
  t.ty = Y >> 8;
  t.oob = t.tx >= S.w || t.ty >= S.h;
  const unsigned Xc = X < fine_w - 1u ? X : fine_w - 1u, Yc = Y < fine_h - 1u ? Y : fine_h - 1u;
  const unsigned U = Xc >= 128u ? Xc - 128u : Xc + fine_w - 128u; /* 3: texel centres at 256 x + 128; longitude wraps */
  t.x0 = U >> 8;
  t.fx = U & 255u;
  t.x1 = t.x0 + 1u == S.w ? 0u : t.x0 + 1u;
  const unsigned V = Yc >= 128u ? Yc - 128u : 0u; /* 4: colatitude clamps */
  t.y0 = V >> 8;
  t.fy = V & 255u;
  t.y1 = t.y0 + 1u < S.h ? t.y0 + 1u : S.h - 1u;
}
/* 5: the blend of four packed RGBA8 texels -- t00 = T[y0][x0], t01 = T[y0][x1], t10 = T[y1][x0], t11 = T[y1][x1] -- per colour channel
 * (w00 c00 + w01 c01 + w10 c10 + w11 c11 + 32768) >> 16 with integer weights that sum to 65536: at most 255 * 65536 + 32768 < 2^32,
 * one rounding, half up.  Alpha is ignored (as put_pixel ignores it) and comes back as 255. */
CV_HD unsigned sky_bilinear_blend(unsigned t00, unsigned t01, unsigned t10, unsigned t11, unsigned fx, unsigned fy) {
  const unsigned w11 = fx * fy, w01 = fx * (256u - fy), w10 = (256u - fx) * fy, w00 = (256u - fx) * (256u - fy);
  const unsigned r = w00 * (t00 & 255u) + w01 * (t01 & 255u) + w10 * (t10 & 255u) + w11 * (t11 & 255u);
  const unsigned g = w00 * ((t00 >> 8) & 255u) + w01 * ((t01 >> 8) & 255u) + w10 * ((t10 >> 8) & 255u) + w11 * ((t11 >> 8) & 255u);
  const unsigned b = w00 * ((t00 >> 16) & 255u) + w01 * ((t01 >> 16) & 255u) + w10 * ((t10 >> 16) & 255u) + w11 * ((t11 >> 16) & 255u);
  return 0xFF000000u | ((r + 32768u) >> 16) | (((g + 32768u) >> 16) << 8) | (((b + 32768u) >> 16) << 16);
}

/* ---- option "sky_mipmap" = 1: the bilinear lookup on a mip pyramid of the sky, the level chosen per ray from how far its neighbours
 * in the 2 x 2 quad landed (include/curvis_hip.h has the definition: pyramid, footprint, level, colour).  All of it is integer work on
 * the (Xc, Yc) of the bilinear definition's step 2. */
struct SkyMipLevel {
  const unsigned *texels; /* w x h RGBA8; level 0 is the sky itself */
  unsigned w, h;
};
/* sizes: w_{k+1} = (w_k + 1) >> 1, one level per halving until 1 x 1 */
CV_HD unsigned sky_mip_levels(unsigned w, unsigned h) {
  unsigned L = 1u;
  for (unsigned m = w > h ? w : h; m > 1u; m = (m + 1u) >> 1) ++L;
  return L;
}
/* one texel of level k + 1 from the four of level k under it (packed RGBA8): per colour channel (a + b + c + d + 2) >> 2, alpha 255.
 * Red and blue are summed in one dword, green in another: a channel's sum is at most 1022 and stays inside its 16 bits. */
CV_HD unsigned sky_mip_down(unsigned a, unsigned b, unsigned c, unsigned d) {
  const unsigned rb = (a & 0x00FF00FFu) + (b & 0x00FF00FFu) + (c & 0x00FF00FFu) + (d & 0x00FF00FFu) + 0x00020002u;
  const unsigned g = ((a >> 8) & 0xFFu) + ((b >> 8) & 0xFFu) + ((c >> 8) & 0xFFu) + ((d >> 8) & 0xFFu) + 2u;
  return 0xFF000000u | ((rb >> 2) & 0x00FF00FFu) | ((g >> 2) << 8);
}
/* steps 1 and 2 of the bilinear definition alone: (Xc, Yc), the nearest lookup's raw tx, ty, and -- returned -- whether those lie
 * outside the sky.  The first lines of sky_bilinear_taps, which keeps its own text. */
template <bool SHARED = false>
CV_HD bool sky_fine_indices(const SkyParams &S, double d0, double d1, double d2, unsigned &Xc, unsigned &Yc, unsigned &tx, unsigned &ty,
                            double y_pi = 0.0, double y_two_pi = 0.0) {
  const unsigned fine_w = S.w << 8, fine_h = S.h << 8;
  SkyParams F = S;
  F.w = fine_w;
  F.h = fine_h;
  unsigned X, Y;
  sky_indices<SHARED>(F, d0, d1, d2, X, Y, y_pi, y_two_pi);
  tx = X >> 8;
  ty = Y >> 8;
  Xc = X < fine_w - 1u ? X : fine_w - 1u;
  Yc = Y < fine_h - 1u ? Y : fine_h - 1u;
  return tx >= S.w || ty >= S.h;
}
/* footprint: the largest of |wrap(Xc' - Xc)| and |Yc' - Yc| over the horizontal partner (Xh, Yh) and the vertical one (Xv, Yv) of the
 * ray's quad; a partner with !ok (outside the frame, capped, on the other sky) contributes nothing.  fine_w = 256 w <= 2^31; wrap
 * reduces modulo fine_w into [-fine_w / 2, fine_w / 2). */
CV_HD unsigned sky_mip_wrap_abs(unsigned Xc, unsigned Xp, unsigned fine_w) {
  const unsigned d = Xp >= Xc ? Xp - Xc : Xp + (fine_w - Xc); /* (Xp - Xc) mod fine_w */
  return d < (fine_w >> 1) ? d : fine_w - d;
}
CV_HD unsigned sky_mip_rho(unsigned Xc, unsigned Yc, unsigned fine_w, unsigned Xh, unsigned Yh, bool okh, unsigned Xv, unsigned Yv, bool okv) {
  unsigned rho = 0u;
  if (okh) {
    const unsigned dx = sky_mip_wrap_abs(Xc, Xh, fine_w), dy = Yh >= Yc ? Yh - Yc : Yc - Yh;
    rho = dx > dy ? dx : dy;
  }
  if (okv) {
    const unsigned dx = sky_mip_wrap_abs(Xc, Xv, fine_w), dy = Yv >= Yc ? Yv - Yc : Yc - Yv;
    const unsigned m = dx > dy ? dx : dy;
    rho = rho > m ? rho : m;
  }
  return rho;
}
/* level k and the weight f (in 1/256) of level k + 1, for a pyramid of L >= 1 levels: total for every 32-bit rho */
CV_HD void sky_mip_level(unsigned rho, unsigned L, unsigned &k, unsigned &f) {
  k = 0u;
  f = 0u;
  if (rho >= 256u) {
    k = 23u - (unsigned)__builtin_clz(rho); /* msb(rho) - 8 */
    f = (rho >> k) & 255u;
  }
  if (k >= L - 1u) {
    k = L - 1u;
    f = 0u;
  }
}
/* steps 3 and 4 of the bilinear definition on level k: (Xk, Yk) = (Xc >> k, Yc >> k) over wk x hk texels; Xk < 256 wk always holds.
 * Fills the columns, rows and weights of t; tx, ty and oob are the nearest lookup's and are not touched. */
CV_HD void sky_mip_taps(unsigned Xk, unsigned Yk, unsigned wk, unsigned hk, SkyTaps &t) {
  const unsigned U = Xk >= 128u ? Xk - 128u : Xk + (wk << 8) - 128u;
  t.x0 = U >> 8;
  t.fx = U & 255u;
  t.x1 = t.x0 + 1u == wk ? 0u : t.x0 + 1u;
  const unsigned V = Yk >= 128u ? Yk - 128u : 0u;
  t.y0 = V >> 8;
  t.fy = V & 255u;
  t.y1 = t.y0 + 1u < hk ? t.y0 + 1u : hk - 1u;
}
/* the blend of the colours of level k and level k + 1: per channel ((256 - f) ck + f ck1 + 128) >> 8, alpha 255 */
CV_HD unsigned sky_mip_mix(unsigned ck, unsigned ck1, unsigned f) {
  const unsigned g = 256u - f;
  const unsigned r = (g * (ck & 255u) + f * (ck1 & 255u) + 128u) >> 8;
  const unsigned gr = (g * ((ck >> 8) & 255u) + f * ((ck1 >> 8) & 255u) + 128u) >> 8;
  const unsigned b = (g * ((ck >> 16) & 255u) + f * ((ck1 >> 16) & 255u) + 128u) >> 8;
  return 0xFF000000u | r | (gr << 8) | (b << 16);
}
/* the whole per-ray colour from (Xc, Yc, rho) over the level table of a sky: the gathers of both levels are independent and are
 * issued together, four when f = 0 */
CV_HD unsigned sky_mip_colour(const SkyMipLevel *tab, unsigned L, unsigned Xc, unsigned Yc, unsigned rho) {
  unsigned k, f;
  sky_mip_level(rho, L, k, f);
  const SkyMipLevel A = tab[k], B = tab[f ? k + 1u : k];
  SkyTaps a, b;
  sky_mip_taps(Xc >> k, Yc >> k, A.w, A.h, a);
  const unsigned *a0 = A.texels + (size_t)a.y0 * A.w, *a1 = A.texels + (size_t)a.y1 * A.w;
  const unsigned a00 = a0[a.x0], a01 = a0[a.x1], a10 = a1[a.x0], a11 = a1[a.x1];
  if (f == 0u) return sky_bilinear_blend(a00, a01, a10, a11, a.fx, a.fy);
  sky_mip_taps(Xc >> (k + 1u), Yc >> (k + 1u), B.w, B.h, b);
  const unsigned *b0 = B.texels + (size_t)b.y0 * B.w, *b1 = B.texels + (size_t)b.y1 * B.w;
  const unsigned b00 = b0[b.x0], b01 = b0[b.x1], b10 = b1[b.x0], b11 = b1[b.x1];
  return sky_mip_mix(sky_bilinear_blend(a00, a01, a10, a11, a.fx, a.fy), sky_bilinear_blend(b00, b01, b10, b11, b.fx, b.fy), f);
}

}  // namespace cvk

#endif /* CURVIS_CV_DEVICE_H */
