// The brute renderer's call plan (curvis_amd/csrc/brute_plan.h) over the full cross product of its facts, stand-alone: one canonical
// line per combination -- "REFUSE <message>" or "<family> fused=<0|1> relay=<0|1>" -- the SHA-256 of that listing and the number of
// rows per distinct outcome.  tests/test_brute_plan_host.py compiles this under AddressSanitizer and UBSan, runs it and compares
// digest and counts with values recorded from the decision code the plan replaced.  With --dump the listing itself is printed, so
// that a mismatch can be diffed.  For every row that is not a refusal the named family must exist for the row's launch shape.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>

#include "../../curvis_amd/csrc/brute_plan.h"

namespace {

// SHA-256 (FIPS 180-4), written out here: the listing is hashed as it is produced
struct Sha256 {
  uint32_t h[8] = {0x6a09e667u, 0xbb67ae85u, 0x3c6ef372u, 0xa54ff53au, 0x510e527fu, 0x9b05688cu, 0x1f83d9abu, 0x5be0cd19u};
  unsigned char buf[64];
  size_t fill = 0;
  uint64_t bytes = 0;
  static uint32_t rotr(uint32_t x, int n) { return (x >> n) | (x << (32 - n)); }
  void block(const unsigned char *p) {
    static const uint32_t K[64] = {
        0x428a2f98u, 0x71374491u, 0xb5c0fbcfu, 0xe9b5dba5u, 0x3956c25bu, 0x59f111f1u, 0x923f82a4u, 0xab1c5ed5u, 0xd807aa98u, 0x12835b01u, 0x243185beu,
        0x550c7dc3u, 0x72be5d74u, 0x80deb1feu, 0x9bdc06a7u, 0xc19bf174u, 0xe49b69c1u, 0xefbe4786u, 0x0fc19dc6u, 0x240ca1ccu, 0x2de92c6fu, 0x4a7484aau,
        0x5cb0a9dcu, 0x76f988dau, 0x983e5152u, 0xa831c66du, 0xb00327c8u, 0xbf597fc7u, 0xc6e00bf3u, 0xd5a79147u, 0x06ca6351u, 0x14292967u, 0x27b70a85u,
        0x2e1b2138u, 0x4d2c6dfcu, 0x53380d13u, 0x650a7354u, 0x766a0abbu, 0x81c2c92eu, 0x92722c85u, 0xa2bfe8a1u, 0xa81a664bu, 0xc24b8b70u, 0xc76c51a3u,
        0xd192e819u, 0xd6990624u, 0xf40e3585u, 0x106aa070u, 0x19a4c116u, 0x1e376c08u, 0x2748774cu, 0x34b0bcb5u, 0x391c0cb3u, 0x4ed8aa4au, 0x5b9cca4fu,
        0x682e6ff3u, 0x748f82eeu, 0x78a5636fu, 0x84c87814u, 0x8cc70208u, 0x90befffau, 0xa4506cebu, 0xbef9a3f7u, 0xc67178f2u};
    uint32_t w[64];
    for (int i = 0; i < 16; ++i) w[i] = (uint32_t)p[4 * i] << 24 | (uint32_t)p[4 * i + 1] << 16 | (uint32_t)p[4 * i + 2] << 8 | (uint32_t)p[4 * i + 3];
    for (int i = 16; i < 64; ++i) {
      const uint32_t s0 = rotr(w[i - 15], 7) ^ rotr(w[i - 15], 18) ^ (w[i - 15] >> 3), s1 = rotr(w[i - 2], 17) ^ rotr(w[i - 2], 19) ^ (w[i - 2] >> 10);
      w[i] = w[i - 16] + s0 + w[i - 7] + s1;
    }
    uint32_t a = h[0], b = h[1], c = h[2], d = h[3], e = h[4], f = h[5], g = h[6], hh = h[7];
    for (int i = 0; i < 64; ++i) {
      const uint32_t t1 = hh + (rotr(e, 6) ^ rotr(e, 11) ^ rotr(e, 25)) + ((e & f) ^ (~e & g)) + K[i] + w[i];
      const uint32_t t2 = (rotr(a, 2) ^ rotr(a, 13) ^ rotr(a, 22)) + ((a & b) ^ (a & c) ^ (b & c));
      hh = g, g = f, f = e, e = d + t1, d = c, c = b, b = a, a = t1 + t2;
    }
    h[0] += a, h[1] += b, h[2] += c, h[3] += d, h[4] += e, h[5] += f, h[6] += g, h[7] += hh;
  }
  void update(const char *p, size_t n) {
    bytes += n;
    for (size_t i = 0; i < n; ++i) {
      buf[fill++] = (unsigned char)p[i];
      if (fill == 64) block(buf), fill = 0;
    }
  }
  std::string hex() {
    const uint64_t bits = bytes * 8;
    const char one = (char)0x80, zero = 0;
    update(&one, 1);
    while (fill != 56) update(&zero, 1);
    for (int i = 7; i >= 0; --i) {
      const char c = (char)(bits >> (8 * i));
      update(&c, 1);
    }
    char out[65];
    for (int i = 0; i < 8; ++i) snprintf(out + 8 * i, 9, "%08x", h[i]);
    return out;
  }
};

const char *family_name(brute::Family f) {
  switch (f) {
    case brute::Family::Persistent: return "persistent";
    case brute::Family::Unfused: return "unfused";
    case brute::Family::StagedAdapt: return "staged_adapt";
    case brute::Family::Fused: return "fused";
    case brute::Family::Relay: return "relay";
    case brute::Family::Disc: return "disc";
    case brute::Family::DiscMotion: return "disc_motion";
  }
  return "?";
}

std::string line_of(const brute::Facts &f) {
  const brute::Plan p = brute::plan(f);
  if (p.refusal) return std::string("REFUSE ") + p.refusal;
  if (!brute::family_exists(p.family, brute::launch_shape(f))) {
    fprintf(stderr, "the plan names family %s, which does not exist for the call's launch shape\n", family_name(p.family));
    exit(1);
  }
  return std::string(family_name(p.family)) + " fused=" + (p.fused ? "1" : "0") + " relay=" + (p.relay ? "1" : "0");
}

void expect(const char *what, const brute::Facts &f, const std::string &want) {
  const std::string got = line_of(f);
  if (got != want) {
    fprintf(stderr, "%s: got \"%s\", expected \"%s\"\n", what, got.c_str(), want.c_str());
    exit(1);
  }
}

}  // namespace

int main(int argc, char **argv) {
  const bool dump_listing = argc > 1 && !strcmp(argv[1], "--dump");
  // the Sha256 above on FIPS 180-4's own one-block message
  {
    Sha256 s;
    s.update("abc", 3);
    if (s.hex() != "ba7816bf8f01cfea414140de5dae2223b00361a396177a9cb410ff61f20015ad") return fprintf(stderr, "SHA-256 of \"abc\" is wrong\n"), 1;
  }
  // rows to check by eye against brute_plan.h's tables
  {
    brute::Facts plain; // variant = -1, every option off, Ellis (kind 0)
    plain.relay_size_ok = true;
    expect("plain call, size conditions true", plain, "relay fused=1 relay=1");
    brute::Facts f = plain;
    f.disc = brute::DISC_STATIC;
    expect("the same with a disc", f, "disc fused=1 relay=0");
    f = plain, f.sky_filter = f.sky_mipmap = true, f.variant = 0;
    expect("sky_mipmap + variant = 0", f, "REFUSE sky_mipmap = 1: variant = 0 (the persistent kernel) shades from the ray store, which has the nearest lookup only");
    f = plain, f.step_scale = true, f.dump = true;
    expect("step_scale + debug dump", f, "staged_adapt fused=0 relay=0");
    f = plain, f.step_scale = true, f.fuse_shade = false;
    expect("step_scale + fuse_shade = 0", f, "REFUSE step_scale != 0: fuse_shade = 0 (the unfused static kernel) takes the reference's fixed step only outside the debug dump");
    f = plain, f.disc = brute::DISC_MOVING;
    expect("disc motion on Ellis", f, "REFUSE the disc motion is Keplerian and needs the Schwarzschild metric: in the other kinds g00 = -1, free matter is at rest and nothing orbits (set the motion to 0: curvis_ctx_set_disc_motion)");
    f.kind = brute::KIND_SCHWARZSCHILD;
    expect("disc motion on Schwarzschild", f, "disc_motion fused=1 relay=0");
  }
  Sha256 sha;
  std::map<std::string, unsigned> counts;
  unsigned rows = 0;
  static const int variants[4] = {-1, 0, 1, 2};
  brute::Facts f;
  for (int dump = 0; dump < 2; ++dump)
  for (int variant : variants)
  for (int fuse_shade = 0; fuse_shade < 2; ++fuse_shade)
  for (int fast_math = 0; fast_math < 2; ++fast_math)
  for (int supersample = 0; supersample < 2; ++supersample)
  for (int sky_filter = 0; sky_filter < 2; ++sky_filter)
  for (int sky_mipmap = 0; sky_mipmap < 2; ++sky_mipmap)
  for (int projection = 0; projection < 2; ++projection)
  for (int step_scale = 0; step_scale < 2; ++step_scale)
  for (int integrator = 0; integrator < 2; ++integrator)
  for (int disc = 0; disc < 3; ++disc)
  for (int moving = 0; moving < 2; ++moving)
  for (int kind = 0; kind < 4; ++kind)
  for (int relay_size_ok = 0; relay_size_ok < 2; ++relay_size_ok) {
    f.dump = dump, f.variant = variant, f.fuse_shade = fuse_shade, f.fast_math = fast_math, f.supersample = supersample;
    f.sky_filter = sky_filter, f.sky_mipmap = sky_mipmap, f.projection = projection, f.step_scale = step_scale, f.integrator = integrator;
    f.disc = disc, f.moving = moving, f.kind = kind, f.relay_size_ok = relay_size_ok;
    const std::string line = line_of(f) + "\n";
    sha.update(line.data(), line.size());
    if (dump_listing) fputs(line.c_str(), stdout);
    counts[line]++;
    rows++;
  }
  if (dump_listing) return 0;
  printf("rows %u\noutcomes %zu\nsha256 %s\n", rows, counts.size(), sha.hex().c_str());
  for (const auto &kv : counts) printf("%6u %s", kv.second, kv.first.c_str());
  printf("brute plan ok\n");
  return 0;
}
