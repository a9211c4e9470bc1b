// Stand-alone driver for the host instantiation of cvk::camera_boost_prepare and cvk::camera_boost (curvis_amd/csrc/cv_device.h), the
// moving camera of curvis_ctx_set_camera_velocities, built with -fsanitize=address,undefined and run by
// tests/test_camera_boost_sanitize.py.  The five doubles and the vectors live in heap blocks of exactly their size.  It covers the
// classes of input the definition names -- zero velocity, the largest speed below 1 (b2 = 1 - 2^-53), b2 = 1 and beyond, NaN and
// infinite components, vectors of zeros, tiny, huge and NaN components -- and checks what the definition promises: the return value,
// zeros for a frame at rest, u a unit vector, a frame at rest leaving the vector's bits alone (the sign of a zero included), a boost
// along the optical axis leaving the axis, ray_init and efficient_pixel_geometry taking the boost behind PROJ_BOOSTED and being the
// unboosted call without it.  Prints "camera boost ok: <n> cases".
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <memory>

#include "../../curvis_amd/csrc/cv_efficient.h"

static void fail(const char *what, const double *beta, const double *v) {
  std::fprintf(stderr, "san_camera_boost: %s: beta (%a, %a, %a), vec (%a, %a, %a)\n", what, beta[0], beta[1], beta[2], v[0], v[1], v[2]);
  std::exit(1);
}

static bool same(const double *a, const double *b, unsigned n = 3) { return std::memcmp(a, b, n * sizeof(double)) == 0; }

int main() {
  const double nan = std::numeric_limits<double>::quiet_NaN(), inf = std::numeric_limits<double>::infinity();
  const double eye[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0};
  /* a tilted camera: the rotation about (1, 2, 3) / sqrt(14) by one radian, rounded to four digits */
  const double tilt[9] = {0.5731, -0.6091, 0.5482, 0.7403, 0.6716, -0.0277, -0.3513, 0.4217, 0.8359};
  const double top = std::sqrt(1.0 - 0x1p-53); /* its square rounds to 1 - 2^-53 or just below: the largest speeds */
  struct Case {
    double beta[3];
    int identity, tilted; /* the expected return value under either rotation; 2: either 1 or -1 (the matrix is not exactly orthonormal) */
  };
  const Case cases[] = {
      {{0.0, 0.0, 0.0}, 0, 0},          {{-0.0, 0.0, -0.0}, 0, 0},        {{0.3, -0.4, 0.5}, 1, 1},    {{0.0, 0.0, 0.9}, 1, 1},
      {{top, 0.0, 0.0}, 1, 2},          {{0.0, -top, 0.0}, 1, 2},         {{1.0, 0.0, 0.0}, -1, 2},    {{0.6, 0.8, 0.0}, 2, 2},
      {{0.6, 0.8, 0x1p-20}, -1, 2},    {{2.0, 0.0, 0.0}, -1, -1},        {{nan, 0.0, 0.0}, -1, -1},   {{0.1, nan, 0.2}, -1, -1},
      {{inf, 0.0, 0.0}, -1, -1},        {{0.0, -inf, 0.0}, -1, -1},       {{0x1p-600, 0.0, 0.0}, 0, 0}, /* b2 underflows to 0: at rest */
      {{0x1p-500, 0x1p-510, 0.0}, 1, 1}, {{1e-8, 0.0, 0.0}, 1, 1},        {{0.999, 0.0, 0.0}, 1, 1},   {{1e300, 1e300, 1e300}, -1, -1},
  };
  const double vecs[][3] = {{7.0, 1.5, -2.25},  {7.0, -0.0, 0.0},      {0.0, 0.0, 0.0},      {-0.0, -0.0, -0.0},   {0x1p-600, 0x1p-601, 0.0},
                            {0x1p-1074, 0.0, 0.0}, {1e200, -1e200, 1e199}, {1e308, 1e308, 1e308}, {nan, 1.0, 0.0},   {1.0, inf, 0.0},
                            {1.0, 0.0, 0.0},    {-1.0, 0.0, 0.0}};
  cvk::MetricParams M;
  M.rho = 1.0, M.rho2 = 1.0, M.m = 0.1, M.a = 1e-4, M.pim = CV_PI * M.m, M.inv_pim = 1.0 / M.pim, M.two_o_pi = 2.0 / CV_PI;
  M.T = cv_sc_table(), M.LT = cv_log_table(), M.AT = cv_atan_table();
  cvk::EfficientFrame F;
  const double cam_bg[3] = {6.123233995736766e-17, 0.0, 1.0};
  const double rot_bg[9] = {6.123233995736766e-17, 0.0, -1.0, 0.0, 1.0, 0.0, 1.0, 0.0, 6.123233995736766e-17};
  std::memcpy(F.cam_bg, cam_bg, sizeof cam_bg);
  std::memcpy(F.rot_bg, rot_bg, sizeof rot_bg);
  unsigned long long n = 0;
  for (int r = 0; r < 2; ++r) {
    std::unique_ptr<double[]> rot(new double[9]);
    std::memcpy(rot.get(), r ? tilt : eye, sizeof eye);
    for (const Case &c : cases) {
      std::unique_ptr<double[]> beta(new double[3]);
      std::memcpy(beta.get(), c.beta, sizeof c.beta);
      std::unique_ptr<cvk::CameraBoost> K(new cvk::CameraBoost);
      const int rc = cvk::camera_boost_prepare(rot.get(), beta.get(), *K);
      const int want = r ? c.tilted : c.identity;
      if (want == 2 ? (rc != 1 && rc != -1) : rc != want) fail("camera_boost_prepare: return value", c.beta, c.beta);
      const double zeros[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
      if (rc <= 0 && !same(K->u, zeros, 5)) fail("a frame that is not boosted has other than zeros", c.beta, K->u);
      if (rc > 0) {
        const double un = std::sqrt(K->u[0] * K->u[0] + K->u[1] * K->u[1] + K->u[2] * K->u[2]);
        if (!(std::fabs(un - 1.0) < 1e-15 * 8) || !(K->B > 0.0) || !(K->A >= 0.0) || !std::isfinite(K->B)) fail("u, A or B", c.beta, K->u);
      }
      for (const auto &v0 : vecs) {
        std::unique_ptr<double[]> v(new double[3]), w(new double[3]);
        std::memcpy(v.get(), v0, sizeof v0);
        std::memcpy(w.get(), v0, sizeof v0);
        cvk::camera_boost(*K, v[0], v[1], v[2]);
        cvk::camera_boost<true>(*K, w[0], w[1], w[2]); /* on the host the shared form is the plain one */
        if (!same(v.get(), w.get())) fail("the shared instantiation differs", c.beta, v.get());
        if (rc <= 0 && !same(v.get(), v0)) fail("a frame at rest changed the vector", c.beta, v.get());
        const bool tame = std::isfinite(v0[0]) && std::isfinite(v0[1]) && std::isfinite(v0[2]) && std::fabs(v0[0]) < 1e150 && std::fabs(v0[1]) < 1e150 && std::fabs(v0[2]) < 1e150;
        if (rc > 0 && tame && !(std::isfinite(v[0]) && std::isfinite(v[1]) && std::isfinite(v[2]))) fail("a tame vector became infinite", c.beta, v.get());
        ++n;
      }
    }
  }
  /* a boost along the optical axis leaves the axis pixel's direction: vec = (f, 0, 0), u = (1, 0, 0) */
  for (const double b : {0.5, -0.5, 0.999, 1e-8}) {
    const double beta[3] = {b, 0.0, 0.0};
    cvk::CameraBoost K;
    if (cvk::camera_boost_prepare(eye, beta, K) != 1) fail("axis boost refused", beta, beta);
    double v[3] = {7.0, 0.0, 0.0};
    cvk::camera_boost(K, v[0], v[1], v[2]);
    if (!(v[0] > 0.0) || v[1] != 0.0 || v[2] != 0.0) fail("a boost along the axis moved the axis", beta, v);
    ++n;
  }
  /* ray_init and efficient_pixel_geometry: behind the bit, and without it the call they were */
  cvk::CameraParams C;
  C.pos[0] = 0.0, C.pos[1] = 1.0, C.pos[2] = CV_PI / 2.0, C.pos[3] = 0.0;
  std::memcpy(C.rot, tilt, sizeof tilt);
  C.focal = 7.0, C.sensor_w = 35.0, C.sensor_h = 25.0, C.res_x = 13.0, C.res_y = 9.0;
  const double beta[3] = {0.3, -0.4, 0.5};
  std::unique_ptr<cvk::CameraBoost> K(new cvk::CameraBoost), Z(new cvk::CameraBoost);
  const double rest[3] = {0.0, 0.0, 0.0};
  if (cvk::camera_boost_prepare(C.rot, beta, *K) != 1 || cvk::camera_boost_prepare(C.rot, rest, *Z) != 0) fail("prepare", beta, beta);
  for (int projection = 0; projection <= 2; ++projection)
    for (unsigned py = 0; py < 9; ++py)
      for (unsigned px = 0; px < 13; ++px) {
        cvk::Ray q = {}, q0 = {}, qz = {};
        cvk::ray_init<cvk::METRIC_ELLIS>(M, C, px, py, q0, projection);
        cvk::ray_init<cvk::METRIC_ELLIS, true>(M, C, px, py, qz, projection | cvk::PROJ_BOOSTED, Z.get());
        cvk::ray_init<cvk::METRIC_ELLIS, true>(M, C, px, py, q, projection | cvk::PROJ_BOOSTED, K.get());
        const double d[3] = {q.p1, q.p2, q.p3};
        if (std::memcmp(&q0, &qz, sizeof q0) != 0) fail("a frame at rest behind the bit is not the unboosted photon", rest, d);
        if (std::memcmp(&q0, &q, sizeof q0) == 0 || !std::isfinite(q.p1) || !std::isfinite(q.p2) || !std::isfinite(q.p3)) fail("boosted photon", beta, d);
        std::unique_ptr<double[]> axis(new double[3]), axis0(new double[3]);
        double alpha = 0.0, alpha0 = 0.0;
        cvk::efficient_pixel_geometry(C, F, px, py, alpha0, axis0.get(), nullptr, projection);
        cvk::efficient_pixel_geometry(C, F, px, py, alpha, axis.get(), nullptr, projection | cvk::PROJ_BOOSTED, Z.get());
        if (std::memcmp(&alpha, &alpha0, sizeof alpha) != 0 || !same(axis.get(), axis0.get())) fail("pixel geometry of a frame at rest", rest, axis.get());
        cvk::efficient_pixel_geometry(C, F, px, py, alpha, axis.get(), nullptr, projection | cvk::PROJ_BOOSTED, K.get());
        if (!(alpha >= 0.0 && alpha <= 3.1415926535897936)) fail("boosted pixel geometry", beta, axis.get());
        ++n;
      }
  std::printf("camera boost ok: %llu cases\n", n);
  return 0;
}
