// Stand-alone driver for the host instantiation of the per-ray functions of library option "sky_mipmap" (curvis_amd/csrc/cv_device.h:
// sky_mip_levels, sky_mip_down, sky_mip_rho, sky_mip_level, sky_mip_taps, sky_mip_mix, sky_mip_colour), built with
// -fsanitize=address,undefined and run by tests/test_sky_mipmap_host.py.  For every sky size it builds the pyramid into heap blocks of
// exactly w_k * h_k texels each, so that a gather one past the end of a level is an AddressSanitizer report and a shift or overflow a
// UBSan one, and checks what the definition promises: the level count, the 1 x 1 last level, k < L, f < 256, f = 0 on the last level,
// taps inside their level, a mix between its inputs, and level 0 equal to the bilinear blend.  Prints "sky mipmap ok: <n> lookups".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../curvis_amd/csrc/cv_device.h"

static void fail(const char *what, unsigned w, unsigned h, unsigned Xc, unsigned Yc, unsigned rho) {
  std::fprintf(stderr, "san_sky_mipmap: %s: sky %u x %u, Xc %u Yc %u rho %u\n", what, w, h, Xc, Yc, rho);
  std::exit(1);
}

int main() {
  const unsigned sizes[][2] = {{1, 1}, {2, 2}, {3, 2}, {13, 7}, {16, 5}, {1, 37}, {37, 1}, {333, 777}, {1024, 512}, {1, 1u << 16}, {1u << 16, 1}};
  std::vector<unsigned> rhos = {0u, 1u, 255u, 256u, 257u, 511u, 512u, 0xFFFFFFFFu};
  for (unsigned k = 0; k < 24; ++k)
    for (int d = -1; d <= 1; ++d) rhos.push_back((256u << k) + (unsigned)d);
  unsigned long long n = 0, sum = 0;
  uint64_t s = 0x9E3779B97F4A7C15ull;
  for (const auto &size : sizes) {
    const unsigned w = size[0], h = size[1];
    const unsigned L = cvk::sky_mip_levels(w, h);
    std::vector<std::vector<unsigned>> texels(L);
    std::vector<cvk::SkyMipLevel> tab(L);
    texels[0].resize((size_t)w * h);
    for (size_t i = 0; i < texels[0].size(); ++i) texels[0][i] = ((unsigned)(i * 2654435761u) ^ 0x00A5C33Cu) | 0xFF000000u;
    tab[0] = cvk::SkyMipLevel{texels[0].data(), w, h};
    for (unsigned k = 1; k < L; ++k) {
      const unsigned ws = tab[k - 1].w, hs = tab[k - 1].h, wd = (ws + 1u) >> 1, hd = (hs + 1u) >> 1;
      texels[k].resize((size_t)wd * hd);
      for (unsigned y = 0; y < hd; ++y)
        for (unsigned x = 0; x < wd; ++x) {
          const unsigned x0 = 2u * x, x1 = x0 + 1u < ws ? x0 + 1u : ws - 1u, y0 = 2u * y, y1 = y0 + 1u < hs ? y0 + 1u : hs - 1u;
          const unsigned *src = texels[k - 1].data();
          texels[k][(size_t)y * wd + x] = cvk::sky_mip_down(src[(size_t)y0 * ws + x0], src[(size_t)y0 * ws + x1], src[(size_t)y1 * ws + x0], src[(size_t)y1 * ws + x1]);
        }
      tab[k] = cvk::SkyMipLevel{texels[k].data(), wd, hd};
    }
    if (tab[L - 1].w != 1u || tab[L - 1].h != 1u) fail("the last level is not 1 x 1", w, h, 0, 0, 0);
    if (L > 1u && tab[L - 2].w == 1u && tab[L - 2].h == 1u) fail("one level too many", w, h, 0, 0, 0);
    const unsigned fine_w = w << 8, fine_h = h << 8;
    std::vector<unsigned> xs = {0u, 1u, 127u, 128u, 129u, fine_w / 2u, fine_w - 129u, fine_w - 128u, fine_w - 1u};
    std::vector<unsigned> ys = {0u, 127u, 128u, fine_h / 2u, fine_h - 129u, fine_h - 128u, fine_h - 1u};
    for (int i = 0; i < 300; ++i) {
      s = s * 6364136223846793005ull + 1442695040888963407ull;
      xs.push_back((unsigned)(s >> 33) % fine_w);
      ys.push_back((unsigned)(s >> 13) % fine_h);
    }
    for (size_t i = 0; i < xs.size(); ++i) {
      const unsigned Xc = xs[i] % fine_w, Yc = ys[i % ys.size()] % fine_h;
      for (unsigned rho : rhos) {
        unsigned k, f;
        cvk::sky_mip_level(rho, L, k, f);
        if (k >= L || f > 255u || (k == L - 1u && f != 0u)) fail("level outside the pyramid", w, h, Xc, Yc, rho);
        if (rho < 256u && (k != 0u || f != 0u)) fail("rho < 256 is level 0", w, h, Xc, Yc, rho);
        cvk::SkyTaps t;
        cvk::sky_mip_taps(Xc >> k, Yc >> k, tab[k].w, tab[k].h, t);
        if (t.x0 >= tab[k].w || t.x1 >= tab[k].w || t.y0 >= tab[k].h || t.y1 >= tab[k].h || t.fx > 255u || t.fy > 255u)
          fail("tap outside its level", w, h, Xc, Yc, rho);
        const unsigned out = cvk::sky_mip_colour(tab.data(), L, Xc, Yc, rho);
        if ((out >> 24) != 255u) fail("alpha", w, h, Xc, Yc, rho);
        if (k == 0u && f == 0u) { /* level 0 is the bilinear blend of the sky itself */
          cvk::SkyTaps b;
          cvk::sky_mip_taps(Xc, Yc, w, h, b);
          const unsigned *r0 = tab[0].texels + (size_t)b.y0 * w, *r1 = tab[0].texels + (size_t)b.y1 * w;
          if (out != cvk::sky_bilinear_blend(r0[b.x0], r0[b.x1], r1[b.x0], r1[b.x1], b.fx, b.fy)) fail("level 0 differs from the bilinear blend", w, h, Xc, Yc, rho);
        }
        sum += out;
        ++n;
      }
      /* the footprint: symmetric, bounded by half the virtual width, and exactly half of it at opposite longitudes */
      const unsigned Xp = xs[(i + 7) % xs.size()] % fine_w, Yp = ys[(i + 3) % ys.size()] % fine_h;
      const unsigned a = cvk::sky_mip_rho(Xc, Yc, fine_w, Xp, Yp, true, 0u, 0u, false), b = cvk::sky_mip_rho(Xp, Yp, fine_w, Xc, Yc, true, 0u, 0u, false);
      const unsigned dy = Yp > Yc ? Yp - Yc : Yc - Yp;
      if (a != b || a < dy || (a > fine_w / 2u && a != dy)) fail("footprint", w, h, Xc, Yc, a);
      if (cvk::sky_mip_rho(Xc, Yc, fine_w, Xp, Yp, false, Xp, Yp, false) != 0u) fail("a partner that does not count counted", w, h, Xc, Yc, 0);
      const unsigned opposite = Xc >= fine_w / 2u ? Xc - fine_w / 2u : Xc + fine_w / 2u;
      if (cvk::sky_mip_rho(Xc, Yc, fine_w, opposite, Yc, true, Xc, Yc, true) != fine_w / 2u) fail("a difference of exactly 128 w", w, h, Xc, Yc, 0);
    }
    for (unsigned c0 : {0u, 0x00FFFFFFu, 0x00336699u})
      for (unsigned c1 : {0u, 0x00FFFFFFu, 0x00996633u})
        for (unsigned f = 0; f < 256u; ++f) {
          const unsigned m = cvk::sky_mip_mix(c0, c1, f);
          for (unsigned sh = 0; sh < 24; sh += 8) {
            const unsigned x = (c0 >> sh) & 255u, y = (c1 >> sh) & 255u, o = (m >> sh) & 255u;
            if (o < (x < y ? x : y) || o > (x > y ? x : y) || (f == 0u && o != x)) fail("mix outside its inputs", w, h, c0, c1, f);
          }
        }
  }
  std::printf("sky mipmap ok: %llu lookups (checksum %llu)\n", n, sum);
  return 0;
}
