/* kernels_epilogue.h -- what the render kernels of kernels_geodesic.h and kernels_efficient.h share behind their loops: per-frame
 * counters and a wave's reduction into them, direction -> colour (sky_lookup_bilinear; sky_lookup, shade_ray's nearest-or-bilinear lookup),
 * colour -> frame buffer (store_rgb8, resolve_store).
 * Part of the ONE translation unit curvis_hip.hip (included there, nowhere else). */
#pragma once

namespace {

/* Statistics counters, PER FRAME (src/rendering.rs:291-316 renders frame by frame; BASELINE configs[4] asks for
 * per-frame early-termination statistics, and a batch of frames is ONE launch here).  Layout of the counter block,
 * in 128-byte lines of CNT_STRIDE words: line 0 holds the persistent kernel's queue head (CNT_NEXT) and nothing
 * else; then `slots` replica lines per frame, each {FC_STEPS, FC_RAYS, FC_POS, FC_NEG, FC_NONE, FC_OOB}.  A wave
 * adds its sums to the replica (blockIdx.x mod slots) of its frame: tens of thousands of waves adding to ONE
 * address serialise in a single L2 channel (it made the 0.06 ms per-pixel kernel of the efficient renderer take
 * 0.40 ms), so a frame's counters are spread over 64 lines in launches of a few frames and over 8 in larger
 * batches.  The host sums the replicas of a frame, and the frames for the totals of the call. */
enum { CNT_NEXT = 0 };
enum { FC_STEPS = 0, FC_RAYS, FC_POS, FC_NEG, FC_NONE, FC_OOB, FC_DISC /* rays that ended on the disc: the DISC kernels alone add to it */, FC_N };
enum { CNT_STRIDE = 16 };
struct FrameCounters {
  unsigned long long *base; /* device: CNT_STRIDE * (1 + n_frames * slots) words */
  unsigned slots;           /* replica lines per frame, a power of two */
};
__host__ __device__ inline unsigned counter_slots_for(unsigned n_frames) { return n_frames >= 8u ? 8u : 64u; }
__host__ __device__ inline size_t counter_words(unsigned n_frames, unsigned slots) {
  return (size_t)CNT_STRIDE * (1u + (size_t)n_frames * slots);
}
__device__ __forceinline__ unsigned long long *frame_counter_line(const FrameCounters &C, unsigned frame) {
  return C.base + (size_t)CNT_STRIDE * (1u + (size_t)frame * C.slots + (blockIdx.x & (C.slots - 1u)));
}
/* frame of a wave's 8x8 tile, as a scalar: computed in the epilogue from the wave-uniform tile number so that no
 * per-lane frame index stays live across the Euler loop (it cost the Interstellar relay kernel its fifth wave) */
__device__ __forceinline__ unsigned frame_of_tile(unsigned long long tile, unsigned rays_per_frame) {
  const unsigned t = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)tile); /* tiles < 2^32 (checked on the host) */
  return t / (rays_per_frame >> 6);
}
/* Add a wave's contribution to the per-frame counters.  `frame` is per lane; lanes with !valid contribute
 * nothing.  When every valid lane of the wave belongs to one frame (always true for the 8x8-tile kernels, and for
 * all but the waves straddling a frame boundary in the per-pixel kernels) the wave reduces first and one lane
 * issues the atomics; otherwise each valid lane adds its own. */
__device__ __forceinline__ void flush_frame_counts(const FrameCounters &C, unsigned frame, bool valid,
                                                   unsigned long long steps, unsigned rays, unsigned pos, unsigned neg,
                                                   unsigned none, unsigned oob) {
  const unsigned long long vm = __builtin_amdgcn_ballot_w64(valid);
  if (!vm) return;
  const unsigned f0 = (unsigned)__builtin_amdgcn_readlane((int)frame, (int)__builtin_ctzll(vm));
  if (!valid) steps = 0ull, rays = pos = neg = none = oob = 0u;
  if (__builtin_amdgcn_ballot_w64(valid && frame != f0) == 0ull) {
    for (int off = 32; off > 0; off >>= 1) {
      steps += __shfl_xor(steps, off);
      rays += __shfl_xor(rays, off);
      pos += __shfl_xor(pos, off);
      neg += __shfl_xor(neg, off);
      none += __shfl_xor(none, off);
      oob += __shfl_xor(oob, off);
    }
    if ((threadIdx.x & 63u) == 0u) {
      unsigned long long *c = frame_counter_line(C, f0);
      if (steps) atomicAdd(&c[FC_STEPS], steps);
      if (rays) atomicAdd(&c[FC_RAYS], (unsigned long long)rays);
      if (pos) atomicAdd(&c[FC_POS], (unsigned long long)pos);
      if (neg) atomicAdd(&c[FC_NEG], (unsigned long long)neg);
      if (none) atomicAdd(&c[FC_NONE], (unsigned long long)none);
      if (oob) atomicAdd(&c[FC_OOB], (unsigned long long)oob);
    }
  } else if (valid) {
    unsigned long long *c = frame_counter_line(C, frame);
    if (steps) atomicAdd(&c[FC_STEPS], steps);
    if (rays) atomicAdd(&c[FC_RAYS], (unsigned long long)rays);
    if (pos) atomicAdd(&c[FC_POS], (unsigned long long)pos);
    if (neg) atomicAdd(&c[FC_NEG], (unsigned long long)neg);
    if (none) atomicAdd(&c[FC_NONE], (unsigned long long)none);
    if (oob) atomicAdd(&c[FC_OOB], (unsigned long long)oob);
  }
}

/* option "sky_filter" = 1: the blend of the four texels around the direction instead of the nearest one (cv_device.h
 * sky_bilinear_taps / sky_bilinear_blend).  The four gathers are independent of each other: all are issued before the blend
 * waits for the first.  tx, ty and the return value (out of bounds) are those of the nearest lookup. */
template <bool SHARED>
__device__ __forceinline__ bool sky_lookup_bilinear(const cvk::SkyParams &S, double d0, double d1, double d2, unsigned &tx, unsigned &ty,
                                                    unsigned &texel, double y_pi = 0.0, double y_two_pi = 0.0) {
  cvk::SkyTaps t;
  cvk::sky_bilinear_taps<SHARED>(S, d0, d1, d2, t, y_pi, y_two_pi);
  const unsigned *row0 = S.texels + (size_t)t.y0 * S.w, *row1 = S.texels + (size_t)t.y1 * S.w;
  const unsigned t00 = row0[t.x0], t01 = row0[t.x1], t10 = row1[t.x0], t11 = row1[t.x1];
  texel = cvk::sky_bilinear_blend(t00, t01, t10, t11, t.fx, t.fy);
  tx = t.tx;
  ty = t.ty;
  return t.oob;
}

/* direction -> colour of sky S for shade_ray: the nearest texel (FILTER = 0; an index outside the sky is clamped) or the bilinear
 * blend (option "sky_filter" = 1).  tx, ty: the raw indices of the nearest lookup, what the debug dump records; oob is set when they
 * lie outside the sky and left alone otherwise.  The efficient pixel kernels and direct_kernel keep their own text of these two
 * branches (kernels_efficient.h says why). */
template <int FILTER>
__device__ __forceinline__ void sky_lookup(const cvk::SkyParams &S, double d0, double d1, double d2, unsigned &tx, unsigned &ty,
                                           unsigned &texel, unsigned &oob) {
  if constexpr (FILTER != 0) {
    if (sky_lookup_bilinear<false>(S, d0, d1, d2, tx, ty, texel)) oob = 1;
  } else {
    cvk::sky_indices(S, d0, d1, d2, tx, ty);
    unsigned cx = tx, cy = ty;
    if (cx >= S.w || cy >= S.h) oob = 1; /* reference: image::get_pixel panics; defined here: clamp + count */
    if (cx >= S.w) cx = S.w - 1;
    if (cy >= S.h) cy = S.h - 1;
    texel = S.texels[(size_t)cy * S.w + cx];
  }
}

/* The seventh counter, FC_DISC: the rays of a wave's tile that ended on the disc (include/curvis_hip.h), added to the counters of the
 * tile's frame.  A function of its own, called by the DISC kernels behind flush_frame_counts, which stays the text it was: `frame` is
 * the wave-uniform frame of the tile (frame_of_tile), lanes with !valid contribute nothing, one lane issues the one atomic. */
__device__ __forceinline__ void flush_disc_count(const FrameCounters &C, unsigned frame, bool valid, unsigned disc) {
  if (!valid) disc = 0u;
  for (int off = 32; off > 0; off >>= 1) disc += __shfl_xor(disc, off);
  if ((threadIdx.x & 63u) == 0u && disc) atomicAdd(&frame_counter_line(C, frame)[FC_DISC], (unsigned long long)disc);
}

/* the three colour bytes of a texel (Rgba, red in the low byte) -> one RGB8 pixel */
__device__ __forceinline__ void store_rgb8(unsigned char *dst, unsigned texel) {
  dst[0] = (unsigned char)(texel & 0xFF);
  dst[1] = (unsigned char)((texel >> 8) & 0xFF);
  dst[2] = (unsigned char)((texel >> 16) & 0xFF);
}

/* ---- supersampling (option "supersample" = SS in {2, 4, 8}): the launch runs over the SS x SS times finer ray grid, and the
 * wave that holds an 8x8 tile of it averages every SS x SS block into one output pixel.  SS divides 8, so a block never straddles
 * two waves: no atomics, no second pass.  Lane k of a tile is sub-pixel (k & 7, k >> 3), so the lanes of a block differ in the low
 * log2 SS bits of each half of the lane number: xor masks {1, 8}, {1, 2, 8, 16}, {1, 2, 4, 8, 16, 32}.
 *
 * v of lane (lane ^ MASK).  Every lane of the wave must be active: DPP for the masks that stay inside a row of 16 lanes
 * (quad_perm [1,0,3,2] and [2,3,0,1], row_ror:8), ds_swizzle in bit mode (and 0x1f, xor MASK) inside a half wave, ds_bpermute
 * across the two halves -- none of them touches LDS memory. */
template <unsigned MASK>
__device__ __forceinline__ unsigned lane_xor(unsigned v) {
  static_assert(MASK == 1u || MASK == 2u || MASK == 4u || MASK == 8u || MASK == 16u || MASK == 32u, "one bit of the lane number");
  if (MASK == 1u) return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0xB1, 0xF, 0xF, true);
  if (MASK == 2u) return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x4E, 0xF, 0xF, true);
  if (MASK == 8u) return (unsigned)__builtin_amdgcn_update_dpp(0, (int)v, 0x128, 0xF, 0xF, true);
  if (MASK == 4u || MASK == 16u) return (unsigned)__builtin_amdgcn_ds_swizzle((int)v, (int)((MASK << 10) | 0x1Fu));
  return (unsigned)__builtin_amdgcn_ds_bpermute((int)(((threadIdx.x & 63u) ^ 32u) << 2), (int)v);
}

/* Called by EVERY lane of a wave that holds one 8x8 tile of the fine grid: (px, py) is the lane's fine pixel inside the launch,
 * W x H the fine size of the launch (multiples of SS), `texel` what the lane's ray saw; lanes with !valid (outside the frame: whole
 * blocks of them, since SS divides 8) add nothing.  Channel sums are at most 64 x 255 < 2^14: red and green share a dword.  The
 * lane of sub-pixel (0, 0) of each block stores out = (sum + SS^2 / 2) >> (2 log2 SS) -- the straight average of the 8-bit values,
 * half rounded up -- at pixel (px / SS, py / SS) of frame `frame` of the W/SS x H/SS frames in fb. */
template <int SS>
__device__ __forceinline__ void resolve_store(unsigned char *fb, unsigned W, unsigned H, unsigned frame, unsigned px, unsigned py,
                                              bool valid, unsigned texel) {
  static_assert(SS == 2 || SS == 4 || SS == 8, "a wave's 64 rays are an 8x8 tile: the factor must divide 8");
  constexpr unsigned LG = SS == 2 ? 1u : SS == 4 ? 2u : 3u;
  unsigned rg = valid ? ((texel & 0xFFu) | ((texel & 0xFF00u) << 8)) : 0u;
  unsigned b = valid ? ((texel >> 16) & 0xFFu) : 0u;
  rg += lane_xor<1>(rg), b += lane_xor<1>(b);
  if (SS >= 4) rg += lane_xor<2>(rg), b += lane_xor<2>(b);
  if (SS >= 8) rg += lane_xor<4>(rg), b += lane_xor<4>(b);
  rg += lane_xor<8>(rg), b += lane_xor<8>(b);
  if (SS >= 4) rg += lane_xor<16>(rg), b += lane_xor<16>(b);
  if (SS >= 8) rg += lane_xor<32>(rg), b += lane_xor<32>(b);
  if (valid && ((px | py) & (unsigned)(SS - 1)) == 0u) {
    constexpr unsigned HALF = (unsigned)(SS * SS) / 2u;
    const unsigned Wo = W >> LG, Ho = H >> LG;
    unsigned char *dst = fb + ((size_t)frame * Wo * Ho + (size_t)(py >> LG) * Wo + (px >> LG)) * 3;
    dst[0] = (unsigned char)(((rg & 0xFFFFu) + HALF) >> (2u * LG));
    dst[1] = (unsigned char)(((rg >> 16) + HALF) >> (2u * LG));
    dst[2] = (unsigned char)((b + HALF) >> (2u * LG));
  }
}

/* ---- option "sky_mipmap" = 1 (the kernels' FILTER = 2): the level tables of the two skies (device memory, levels[k] entries each).
 * They travel in a struct DERIVED from the kernel's argument struct, behind its last member, so that no argument of any other
 * instantiation moves. */
struct SkyMipArgs {
  const cvk::SkyMipLevel *tab[2];
  unsigned levels[2];
};
template <typename Base>
struct WithSkyMip : Base {
  SkyMipArgs mip;
};
/* ---- the accretion disc (include/curvis_hip.h): its texture and bounds, appended to the argument of the DISC kernels the same way */
struct DiscArgs {
  const unsigned *texels; /* w x h RGBA8, w along azimuth, h along l */
  unsigned w, h;
  double l_in, l_out;
};
template <typename Base>
struct WithDisc : Base {
  DiscArgs disc;
};
/* ---- the disc's emission shift (include/curvis_hip.h, curvis_ctx_set_disc_motion): appended behind the disc for the DISC = 2 kernels */
struct DiscMotionArgs {
  double sigma, gain;       /* the motion as +1.0 or -1.0, and G */
  const double *cam_factor; /* device, one per frame of the launch: cv_device.h disc_camera_factor of the frame's camera, from the host */
};
template <typename Base>
struct WithDiscMotion : Base {
  DiscMotionArgs motion;
};
/* Called by EVERY lane of a wave that holds one 8x8 tile of rays whose origin is even in both absolute ray coordinates: `which` is 0
 * (no sky: capped, or outside the frame), 1 (+l sky) or 2 (-l sky), (Xc, Yc) the lane's indices on its own sky.  The lanes exchange the
 * three with the horizontal (lane ^ 1) and vertical (lane ^ 8) partner of their 2 x 2 quad on DPP, form the footprint, the level and
 * its fraction (cv_device.h sky_mip_rho / sky_mip_level) and return the colour; black for which = 0. */
__device__ __forceinline__ unsigned sky_mip_shade(const SkyMipArgs &A, const cvk::SkyParams *sky, unsigned which, unsigned Xc, unsigned Yc) {
  const unsigned Xh = lane_xor<1>(Xc), Yh = lane_xor<1>(Yc), wh = lane_xor<1>(which);
  const unsigned Xv = lane_xor<8>(Xc), Yv = lane_xor<8>(Yc), wv = lane_xor<8>(which);
  unsigned texel = 0xFF000000u;
  if (which != 0u) {
    const bool second = which == 2u;
    const unsigned fine_w = (second ? sky[1].w : sky[0].w) << 8;
    const unsigned rho = cvk::sky_mip_rho(Xc, Yc, fine_w, Xh, Yh, wh == which, Xv, Yv, wv == which);
    texel = cvk::sky_mip_colour(second ? A.tab[1] : A.tab[0], second ? A.levels[1] : A.levels[0], Xc, Yc, rho);
  }
  return texel;
}

/* level k + 1 of a sky's mip chain from level k (cv_device.h sky_mip_down): one thread per output texel, a row of the grid per output
 * row; a thread reads the 2 x 2 texels under its own -- two neighbouring dwords of two rows, so a wave reads two whole runs of 512
 * bytes -- with the last column and row repeated where the source size is odd.  Bandwidth-bound: 5/4 of the source level's bytes. */
__global__ __launch_bounds__(256) void sky_mip_kernel(const unsigned *src, unsigned ws, unsigned hs, unsigned *dst, unsigned wd, unsigned hd) {
  const unsigned x = blockIdx.x * 256u + threadIdx.x;
  for (unsigned y = blockIdx.y; y < hd; y += gridDim.y) {
    if (x < wd) {
      const unsigned x0 = 2u * x, x1 = x0 + 1u < ws ? x0 + 1u : ws - 1u;
      const unsigned y0 = 2u * y, y1 = y0 + 1u < hs ? y0 + 1u : hs - 1u;
      const unsigned *r0 = src + (size_t)y0 * ws, *r1 = src + (size_t)y1 * ws;
      dst[(size_t)y * wd + x] = cvk::sky_mip_down(r0[x0], r0[x1], r1[x0], r1[x1]);
    }
  }
}

/* the per-ray function of option "sky_mipmap" on chosen (Xc, Yc, rho) triples over one sky's level table (tests) */
__global__ void selftest_sky_mip_kernel(const cvk::SkyMipLevel *tab, unsigned L, const unsigned *triples, size_t n, unsigned *out) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const unsigned fine_w = tab[0].w << 8, fine_h = tab[0].h << 8;
  unsigned Xc = triples[3 * i], Yc = triples[3 * i + 1];
  if (Xc >= fine_w) Xc = fine_w - 1u; /* the definition's Xc, Yc lie inside the virtual sky: the gathers below must, too */
  if (Yc >= fine_h) Yc = fine_h - 1u;
  out[i] = cvk::sky_mip_colour(tab, L, Xc, Yc, triples[3 * i + 2]);
}

}  // namespace
