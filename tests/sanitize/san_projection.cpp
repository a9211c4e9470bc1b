// Stand-alone driver for the host instantiation of cvk::camera_pixel_vector and cvk::ray_init (curvis_amd/csrc/cv_device.h) under
// option "projection", built with -fsanitize=address,undefined and run by tests/test_projection_host.py.  For every frame size and
// every projection it runs both functions (and efficient_pixel_geometry, which calls the first) over the pixels, with the output
// vectors in heap blocks of exactly three doubles, and checks what the definition promises: a finite vector, projection 0 the
// reference's three expressions bit for bit, the instantiation with the call's reciprocals equal to the plain one, the fisheye
// centre pixel of an odd x odd frame (1, 0, 0), a photon with finite momenta.  Prints "projection ok: <n> pixels".
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "../../curvis_amd/csrc/cv_efficient.h"

static void fail(const char *what, int projection, unsigned w, unsigned h, unsigned px, unsigned py, const double *v) {
  std::fprintf(stderr, "san_projection: %s: projection %d, %u x %u, pixel (%u, %u): (%a, %a, %a)\n", what, projection, w, h, px, py, v[0], v[1], v[2]);
  std::exit(1);
}

static bool same(const double *a, const double *b) { return std::memcmp(a, b, 3 * sizeof(double)) == 0; }

int main() {
  cvk::MetricParams M;
  M.rho = 1.0, M.rho2 = 1.0, M.m = 0.1, M.a = 1e-4, M.pim = CV_PI * M.m, M.inv_pim = 1.0 / M.pim, M.two_o_pi = 2.0 / CV_PI;
  M.T = cv_sc_table(), M.LT = cv_log_table(), M.AT = cv_atan_table();
  cvk::EfficientFrame F;
  const double cam_bg[3] = {6.123233995736766e-17, 0.0, 1.0}; /* camera on the equator */
  const double rot_bg[9] = {6.123233995736766e-17, 0.0, -1.0, 0.0, 1.0, 0.0, 1.0, 0.0, 6.123233995736766e-17};
  std::memcpy(F.cam_bg, cam_bg, sizeof cam_bg);
  std::memcpy(F.rot_bg, rot_bg, sizeof rot_bg);
  const unsigned sizes[6][3] = {{1, 1, 1}, {2, 1, 1}, {13, 9, 1}, {21, 15, 1}, {64, 32, 1}, {4096, 2048, 97}}; /* w, h, pixel stride */
  unsigned long long n = 0;
  for (const auto &s : sizes) {
    const unsigned w = s[0], h = s[1];
    cvk::CameraParams C;
    C.pos[0] = 0.0, C.pos[1] = 1.0, C.pos[2] = CV_PI / 2.0, C.pos[3] = 0.0;
    /* a tilted camera: the rotation about (1, 2, 3) / sqrt(14) by one radian, any orthonormal matrix will do */
    const double rot[9] = {0.5731, -0.6091, 0.5482, 0.7403, 0.6716, -0.0277, -0.3513, 0.4217, 0.8359};
    std::memcpy(C.rot, rot, sizeof rot);
    C.focal = 7.0;
    const double aspect = (double)w / (double)h;
    C.sensor_h = std::sqrt(43.0 * 43.0 / (aspect * aspect + 1.0));
    C.sensor_w = aspect * C.sensor_h;
    C.res_x = (double)w, C.res_y = (double)h;
    cvk::PixelRecips R;
    R.y_res_x = 1.0 / C.res_x, R.y_res_y = 1.0 / C.res_y, R.y_pi = 1.0 / CV_PI, R.y_two_pi = 1.0 / (2.0 * CV_PI);
    for (int projection = 0; projection <= 2; ++projection) {
      for (unsigned long long i = 0; i < (unsigned long long)w * h; i += s[2]) {
        const unsigned px = (unsigned)(i % w), py = (unsigned)(i / w);
        std::unique_ptr<double[]> v(new double[3]), vs(new double[3]), axis(new double[3]); /* exactly three doubles each */
        cvk::camera_pixel_vector(C, projection, px, py, v[0], v[1], v[2]);
        cvk::camera_pixel_vector<true>(C, projection, px, py, vs[0], vs[1], vs[2], &R);
        if (!std::isfinite(v[0]) || !std::isfinite(v[1]) || !std::isfinite(v[2])) fail("not finite", projection, w, h, px, py, v.get());
        if (!same(v.get(), vs.get())) fail("the shared-reciprocal instantiation differs", projection, w, h, px, py, vs.get());
        if (projection == 0) {
          const double hh = 0.5 - ((double)py / C.res_y), ww = ((double)px / C.res_x) - 0.5;
          const double ref[3] = {C.focal * 1.0, -C.sensor_w * ww, C.sensor_h * hh};
          if (!same(v.get(), ref)) fail("projection 0 is not the reference's mapping", projection, w, h, px, py, v.get());
        } else {
          const double nn = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
          if (!(std::fabs(nn - 1.0) < 1e-12)) fail("not a unit vector before the normalisation", projection, w, h, px, py, v.get());
        }
        if (projection == 2 && (w & 1u) && (h & 1u) && px == w / 2 && py == h / 2) {
          const double ex[3] = {1.0, 0.0, 0.0};
          if (!same(v.get(), ex)) fail("the centre pixel of an odd x odd fisheye frame is not (1, 0, 0)", projection, w, h, px, py, v.get());
        }
        cvk::Ray q = {}, q0 = {};
        cvk::ray_init<cvk::METRIC_ELLIS>(M, C, px, py, q, projection);
        if (!std::isfinite(q.p1) || !std::isfinite(q.p2) || !std::isfinite(q.p3) || !(q.p3sq >= 0.0)) fail("photon not finite", projection, w, h, px, py, v.get());
        if (projection == 0) { /* the call as the host twin writes it */
          cvk::ray_init<cvk::METRIC_ELLIS>(M, C, px, py, q0);
          if (std::memcmp(&q, &q0, sizeof q) != 0) fail("ray_init without the argument is not projection 0", projection, w, h, px, py, v.get());
        }
        cvk::ray_init<cvk::METRIC_INTERSTELLAR>(M, C, px, py, q, projection);
        if (!std::isfinite(q.p1) || !std::isfinite(q.p2) || !std::isfinite(q.p3)) fail("photon not finite (Interstellar)", projection, w, h, px, py, v.get());
        double alpha = 0.0, alpha_s = 0.0;
        cvk::efficient_pixel_geometry(C, F, px, py, alpha, axis.get(), nullptr, projection);
        cvk::efficient_pixel_geometry<true>(C, F, px, py, alpha_s, vs.get(), &R, projection);
        if (!(alpha >= 0.0 && alpha <= 3.1415926535897936) || std::memcmp(&alpha, &alpha_s, sizeof alpha) != 0 || !same(axis.get(), vs.get()))
          fail("pixel geometry", projection, w, h, px, py, axis.get());
        ++n;
      }
    }
  }
  std::printf("projection ok: %llu pixels\n", n);
  return 0;
}
