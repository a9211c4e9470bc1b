/* kernels_geodesic.h -- the per-pixel path on the device: launch parameters,
 * geodesic_static / geodesic_persistent / geodesic_relay, the relay seat belt's compare kernel, shade_kernel.
 * Part of the ONE translation unit curvis_hip.hip (included there, nowhere else). */
#pragma once

namespace {

/* Final ray states, structure-of-arrays in HBM, indexed by pixel id = frame*W*H + py*W + px.
 * Written by the integration kernel, read once by the shading kernel (48-56 B per ray against
 * ~2000 Euler steps of arithmetic: the staging costs ~0.2% of a frame). */
struct RayStore {
  double *l, *th, *ph, *p1, *p2, *p3;
  unsigned *steps;
  int *code;
};

struct IntegrateParams {
  cvk::MetricParams metric;
  const cvk::CameraParams *cams; /* device, n_frames entries */
  unsigned n_frames, W, H, tiles_x, tiles_y; /* H = rows rendered by this launch (a band of the frame or all of it) */
  unsigned row0;                 /* first image row of the band: pixel (px, py) of the launch is image row row0 + py */
  unsigned rays_per_frame;       /* tiles_x*tiles_y*64 (padded to whole 8x8 tiles) */
  unsigned long long total_rays; /* n_frames * rays_per_frame */
  unsigned max_iter;
  int projection; /* option "projection" (cv_device.h camera_pixel_vector), read by the PROJ instantiations only; it sits in what was
                     padding, so every other argument of every kernel stays where it was */
  double max_radius, delta;
  RayStore store;
  FrameCounters counters;
  int refill_threshold;
  int fast_ok; /* host-side part of the fast-step guard */
  /* fused shading (static kernel, non-debug): the epilogue looks the sky up and writes RGB8 itself */
  cvk::SkyParams sky[2];
  unsigned char *fb;
  /* diagnostics (CURVIS_TRACE_FILE): per wave of the static kernel {start, end (wall_clock64 ticks), HW_ID,
   * XCC_ID}; null in normal operation */
  unsigned long long *trace;
};
/* The argument of the ADAPT instantiations (options "step_scale" and "integrator", cv_device.h step_delta): IntegrateParams with two members appended.
 * The other kernels keep IntegrateParams itself, so not one of their argument loads moves -- the hidden arguments behind the struct
 * (workgroup size) included.  kappa = RN(delta / L0); t_out: the debug dump's x[0] per pixel, integrated on the device (the host's
 * replay_debug_time assumes one delta). */
struct IntegrateParamsAdapt : IntegrateParams {
  double kappa;
  double *t_out;
};
template <int ADAPT>
using IntegrateArgs = std::conditional_t<ADAPT != 0, IntegrateParamsAdapt, IntegrateParams>;
/* FILTER = 2 (option "sky_mipmap"): either of the two with the skies' level tables appended (kernels_epilogue.h WithSkyMip) */
template <int ADAPT, int FILTER>
using IntegrateArgsF = std::conditional_t<FILTER == 2, WithSkyMip<IntegrateArgs<ADAPT>>, IntegrateArgs<ADAPT>>;
/* DISC = 1 (a disc is set, include/curvis_hip.h): any of the four with the disc appended (kernels_epilogue.h WithDisc);
 * DISC = 2 (the disc has a motion): that with the motion appended (WithDiscMotion) */
template <int ADAPT, int FILTER, int DISC>
using IntegrateArgsD = std::conditional_t<DISC == 2, WithDiscMotion<WithDisc<IntegrateArgsF<ADAPT, FILTER>>>,
                                          std::conditional_t<DISC != 0, WithDisc<IntegrateArgsF<ADAPT, FILTER>>, IntegrateArgsF<ADAPT, FILTER>>>;

struct ShadeParams {
  cvk::MetricParams metric;
  cvk::SkyParams sky[2];
  RayStore store;
  unsigned long long n_pixels; /* n_frames*W*H */
  unsigned char *fb;           /* RGB8 */
  curvis_ray_debug *dbg;       /* or null */
  unsigned long long npix;     /* pixels per frame: frame of pixel o = o / npix */
  FrameCounters counters;
};

/* Per-workgroup LDS copy of the sin/cos table (4 KiB; 8 KiB in its 256-row form): the Euler loop evaluates
 * sincos once per step per lane with a data-dependent index; two ds_read_b128 from LDS instead of divergent
 * __constant__ loads. */
/* the kinds whose step evaluates a logarithm: Interstellar (with an arc tangent) and Schwarzschild (the tortoise solver, cv_math.h
 * cv_tortoise_u: four to five of them per metric evaluation).  They keep the log table in LDS and are compiled for the register
 * budget of five waves per SIMD (four in the direct kernel) */
constexpr bool kind_has_log(int kind) { return kind == cvk::METRIC_INTERSTELLAR || kind == cvk::METRIC_SCHWARZSCHILD; }
template <int KIND>
struct alignas(16) MathTablesLds {
  static constexpr unsigned LOG_ROWS = kind_has_log(KIND) ? (unsigned)CV_LOG_TABLE_N : 2u;
  static constexpr unsigned ATAN_ROWS = (KIND == cvk::METRIC_INTERSTELLAR) ? (unsigned)CV_ATAN_TABLE_N : 1u;
  /* Order and alignment are chosen for the address arithmetic of the lookups: the 24-byte log rows sit at offset
   * 0, so ds_read2_b64 (whose offset field is short) and ds_read_b64 share one address register; the 32- and
   * 64-byte rows of the other two tables are read with ds_read_b128, whose offset field reaches any LDS
   * address, so their base offsets cost no instruction either. */
  /* 256-row form of the sin/cos table (cv_sincos_tw: no index mask) in every kernel.  Footprint of the Interstellar
   * kernels: 12 KiB log (512 rows x 24 B) + 8 KiB sin/cos + 8.06 KiB atan (the 129 reciprocal-branch rows x 64 B; the
   * direct-branch rows are read from __constant__ memory by the few steps next to the throat) = 28.1 KiB per
   * workgroup: five workgroups (= five waves per SIMD, what amdgpu_waves_per_eu(5) asks for) fit the CU's 160 KiB,
   * six would not.  The static_assert below keeps a table change from silently costing that occupancy. */
  static constexpr bool WIDE_SC = true;
  double lg[LOG_ROWS][3]; /* only the Interstellar metric evaluates a logarithm and an arc tangent per step */
  double sc[WIDE_SC ? 256 : 128][4];
  double at[ATAN_ROWS][8];
};

static_assert(sizeof(MathTablesLds<cvk::METRIC_INTERSTELLAR>) * 5 <= 160 * 1024,
              "five workgroups of the Interstellar kernels (5 waves per SIMD) must fit the CU's 160 KiB of LDS");
static_assert(sizeof(MathTablesLds<cvk::METRIC_ELLIS>) * 8 <= 160 * 1024, "the Ellis / flat kernels run at up to 8 workgroups per CU");
static_assert(sizeof(MathTablesLds<cvk::METRIC_SCHWARZSCHILD>) * 5 <= 160 * 1024,
              "five workgroups of the Schwarzschild kernels (12 KiB log + 8 KiB sin/cos: 5 waves per SIMD) must fit the CU's 160 KiB of LDS");

/* copy the elementary-function tables of cv_math.h into LDS and point the metric at them */
template <int KIND>
__device__ __forceinline__ void load_math_tables(MathTablesLds<KIND> &L, cvk::MetricParams &M) {
  const double *src = &cv_sc_table_dev[0][0];
  double *dst = &L.sc[0][0];
  for (unsigned i = threadIdx.x; i < (MathTablesLds<KIND>::WIDE_SC ? 1024u : 512u); i += blockDim.x) dst[i] = src[i & 511u];
  M.T = L.sc;
  if (KIND == cvk::METRIC_SCHWARZSCHILD) { /* the log table alone; the arc tangent is not evaluated */
    const double *lsrc = &cv_log_table_dev[0][0];
    double *ldst = &L.lg[0][0];
    for (unsigned i = threadIdx.x; i < 3u * CV_LOG_TABLE_N; i += blockDim.x) ldst[i] = lsrc[i];
    M.LT = L.lg;
    M.AT = cv_atan_table();
  } else if (KIND == cvk::METRIC_INTERSTELLAR) {
    const double *lsrc = &cv_log_table_dev[0][0];
    double *ldst = &L.lg[0][0];
    for (unsigned i = threadIdx.x; i < 3u * CV_LOG_TABLE_N; i += blockDim.x) ldst[i] = lsrc[i];
    M.LT = L.lg;
    const double *asrc = &cv_atan_table_dev[0][0];
    double *adst = &L.at[0][0];
    for (unsigned i = threadIdx.x; i < 8u * CV_ATAN_TABLE_N; i += blockDim.x) adst[i] = asrc[i];
    M.AT = L.at;
  } else {
    M.LT = cv_log_table();
    M.AT = cv_atan_table();
  }
  __syncthreads();
}

/* ray id -> (frame, pixel).  Rays are numbered by 8x8 pixel tiles so the 64 rays a wave draws
 * together are spatial neighbours (similar step counts, neighbouring texels). */
__device__ __forceinline__ bool decode_ray(const IntegrateParams &P, unsigned long long id, unsigned &frame,
                                           unsigned &px, unsigned &py) {
  frame = (unsigned)(id / P.rays_per_frame);
  const unsigned rem = (unsigned)(id - (unsigned long long)frame * P.rays_per_frame);
  const unsigned tile = rem >> 6, k = rem & 63u;
  const unsigned tyi = tile / P.tiles_x, txi = tile - tyi * P.tiles_x;
  px = txi * 8u + (k & 7u);
  py = tyi * 8u + (k >> 3);
  return px < P.W && py < P.H;
}

/* The moving camera (cv_device.h camera_boost): the CameraBoost of a launch's frames lie behind its cameras, n_frames of them after the
 * n_frames CameraParams, while the launch's `projection` carries PROJ_BOOSTED (render_rays uploads them so); read under that bit only. */
__device__ __forceinline__ const cvk::CameraBoost *frame_boost(const cvk::CameraParams *cams, unsigned n_frames, unsigned frame) {
  return reinterpret_cast<const cvk::CameraBoost *>(cams + n_frames) + frame;
}

template <bool PHI>
__device__ __forceinline__ void store_ray(const RayStore &S, size_t o, const cvk::Ray &q, unsigned steps, int code) {
  S.l[o] = q.l;
  S.th[o] = q.th;
  if (PHI) S.ph[o] = q.ph;
  S.p1[o] = q.p1;
  S.p2[o] = q.p2;
  S.p3[o] = q.p3;
  S.steps[o] = steps;
  S.code[o] = code;
}

/* Escape test of src/systems.rs:129-134: `l > R` -> PositiveSpace, else `l < -R` -> NegativeSpace.
 * One compare per step: |l| > R is true exactly when one of the two is (false for NaN, like both);
 * which one is decided once, after the loop. */
__device__ __forceinline__ bool ray_escaped(double l, double R) { return __builtin_fabs(l) > R; }
__device__ __forceinline__ int escape_code(double l) { return l > 0.0 ? cvk::CODE_POS : cvk::CODE_NEG; }

template <int KIND, bool PHI, bool FAST, bool EQ = false>
__device__ __forceinline__ void one_step(const cvk::MetricParams &M, double delta, cvk::Ray &q, bool lane_ok) {
  if (FAST)
    cvk::ray_step_fast<KIND, PHI, MathTablesLds<KIND>::WIDE_SC, EQ>(M, q, delta, lane_ok);
  else
    cvk::ray_step<KIND, PHI, MathTablesLds<KIND>::WIDE_SC>(M, q, delta);
}

/* option "integrator" = 1: one Heun step (cv_device.h ray_step_heun), two of the above from a saved state and an average */
template <int KIND, bool PHI, bool FAST, bool EQ = false>
__device__ __forceinline__ void heun_step(const cvk::MetricParams &M, double delta, cvk::Ray &q, bool lane_ok) {
  cvk::ray_step_heun<KIND, PHI, FAST, MathTablesLds<KIND>::WIDE_SC, EQ>(M, q, delta, lane_ok);
}

/* The disc test of the DISC kernels (include/curvis_hip.h, the disc's paragraph), as the probe of the step from y_k: it is handed
 * (s_k, c_k) while q is still y_k, so the loop carries l, phi and cos(theta) of y_{k-1} and nothing else.  The hot path pays two sign
 * compares, a ballot and a scalar branch; cv_device.h disc_crossing (three divisions), the gather and the alpha test sit behind the
 * branch, taken in the few iterations in which some lane of the wave changes hemisphere.  A lane that ends here gets its texel (alpha
 * >= 128, so non-zero); the step it is inside of runs to its end and is discarded by the loop. */
struct DiscProbe {
  const DiscArgs &D;
  const cvk::Ray &q;
  double &l_prev, &ph_prev, &c_prev;
  unsigned &texel;
  bool first; /* k = 0 (wave-uniform): there is no previous state */
  __device__ __forceinline__ void rec(int, double, double, double) const {}
  __device__ __forceinline__ void sincos(double s, double c) const {
    const bool crossed = !first & ((c_prev < 0.0) != (c < 0.0));
    if (__builtin_amdgcn_ballot_w64(crossed)) {
      if (crossed) {
        unsigned tx, ty;
        if (cvk::disc_crossing(c_prev, c, s, l_prev, q.l, ph_prev, q.ph, D.l_in, D.l_out, D.w, D.h, &tx, &ty)) {
          const unsigned t = D.texels[(size_t)ty * D.w + tx];
          if ((t >> 24) >= 128u) texel = t;
        }
      }
    }
    l_prev = q.l, ph_prev = q.ph, c_prev = c;
  }
};
/* The probe of the DISC = 2 kernels (the disc has a motion, include/curvis_hip.h): DiscProbe with the emission shift at the moment a lane
 * gets its texel.  What the lane keeps is the SHADED colour, so the loop carries nothing DiscProbe's does not.  Behind the two branches:
 * cv_device.h disc_shift_at (one tortoise solve for u_e, three divisions and a root) with the ray's constant p_phi and the camera factor
 * of the wave's frame -- a tile never straddles frames, so the frame is wave-uniform, found from the block index as the epilogue finds it,
 * and the factor is one load of what the host evaluated per frame. */
struct DiscShiftProbe {
  const DiscArgs &D;
  const DiscMotionArgs &S;
  const cvk::MetricParams &M;
  unsigned rays_per_frame;
  const cvk::Ray &q;
  double &l_prev, &ph_prev, &c_prev;
  unsigned &texel;
  bool first;
  __device__ __forceinline__ void rec(int, double, double, double) const {}
  __device__ __forceinline__ void sincos(double s, double c) const {
    const bool crossed = !first & ((c_prev < 0.0) != (c < 0.0));
    if (__builtin_amdgcn_ballot_w64(crossed)) {
      if (crossed) {
        unsigned tx, ty;
        double l_hit;
        if (cvk::disc_crossing_at(c_prev, c, s, l_prev, q.l, ph_prev, q.ph, D.l_in, D.l_out, D.w, D.h, &tx, &ty, &l_hit)) {
          const unsigned t = D.texels[(size_t)ty * D.w + tx];
          if ((t >> 24) >= 128u) {
            const unsigned frame = frame_of_tile(((unsigned long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6, rays_per_frame);
            texel = cvk::disc_shade(t, cvk::disc_shift_at(M, l_hit, S.cam_factor[frame], S.sigma, S.gain, q.p3));
          }
        }
      }
    }
    l_prev = q.l, ph_prev = q.ph, c_prev = c;
  }
};
}  // namespace
template <>
struct cvk::probe_takes_sincos<DiscProbe> {
  static constexpr bool value = true;
};
template <>
struct cvk::probe_takes_sincos<DiscShiftProbe> {
  static constexpr bool value = true;
};
namespace {
/* a step of a DISC kernel: the call's step flavour with phi integrated, under the probe (with Heun, the first stage's) */
template <int KIND, bool FAST, bool HEUN, class PROBE>
__device__ __forceinline__ void disc_step(const cvk::MetricParams &M, double delta, cvk::Ray &q, bool lane_ok, const PROBE &probe) {
  constexpr bool W = MathTablesLds<KIND>::WIDE_SC;
  if constexpr (HEUN) {
    static_assert(FAST, "the Heun step exists for the fast step only");
    cvk::ray_step_heun<KIND, true, true, W, false, PROBE>(M, q, delta, lane_ok, probe);
  } else if constexpr (FAST) {
    cvk::ray_step_fast<KIND, true, W, false, PROBE>(M, q, delta, lane_ok, probe);
  } else {
    cvk::ray_step_probed<KIND, true, W, PROBE>(M, q, delta, probe);
  }
}

/* final photon -> tangent direction -> nearest sky texel (rows R9-R10 of SURVEY.md 8a); FILTER: the bilinear blend instead */
template <int KIND, int FILTER = 0>
__device__ __forceinline__ unsigned shade_ray(const cvk::MetricParams &M, const cvk::SkyParams *sky, const cvk::Ray &q,
                                              int code, unsigned &tx, unsigned &ty, unsigned &oob) {
  unsigned texel = 0xFF000000u; /* Rgba([0,0,0,255]) */
  tx = ty = 0;
  if (code != cvk::CODE_NONE) {
    double d0, d1, d2;
    cvk::ray_direction<KIND>(M, q, d0, d1, d2);
    sky_lookup<FILTER>(sky[code == cvk::CODE_POS ? 0 : 1], d0, d1, d2, tx, ty, texel, oob);
  }
  return texel;
}

/* K1, persistent form: lanes draw rays from a global queue with one wave-aggregated atomic whenever
 * `refill_threshold` lanes are free; terminated rays are stored together at that point. */
template <int KIND, bool PHI, bool FAST>
__global__ __launch_bounds__(256) void geodesic_persistent(const IntegrateParams P) {
  __shared__ MathTablesLds<KIND> s_tab;
  cvk::MetricParams M = P.metric;
  load_math_tables<KIND>(s_tab, M);
  const unsigned lane = threadIdx.x & 63u;
  cvk::Ray q;
  q.l = q.th = q.ph = q.p1 = q.p2 = q.p3 = q.p3sq = 0.0;
  size_t slot = 0;
  unsigned steps = 0;
  int code = cvk::CODE_NONE;
  bool active = false; /* lane is integrating */
  bool done = false;   /* lane holds a terminated ray that has not been stored yet */
  bool dry = false;    /* queue exhausted (wave-uniform) */
  bool lane_ok = false;

  for (;;) {
    if (done) { /* staged path: shade_kernel reads the store and keeps the per-frame statistics */
      store_ray<PHI>(P.store, slot, q, steps, code);
      done = false;
    }
    if (!dry) {
      const bool need = !active;
      const unsigned long long mask = __ballot(need);
      if (mask) {
        const unsigned n = (unsigned)__popcll(mask);
        const int leader = __ffsll((long long)mask) - 1;
        unsigned long long base = 0;
        if ((int)lane == leader) base = atomicAdd(&P.counters.base[CNT_NEXT], (unsigned long long)n);
        base = __shfl(base, leader);
        const unsigned rank =
            __builtin_amdgcn_mbcnt_hi((unsigned)(mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)mask, 0u));
        const unsigned long long mine = base + rank;
        if (need && mine < P.total_rays) {
          unsigned frame, px, py;
          if (decode_ray(P, mine, frame, px, py)) {
            cvk::ray_init<KIND>(M, P.cams[frame], px, py + P.row0, q);
            slot = (size_t)frame * P.W * P.H + (size_t)py * P.W + px;
            steps = 0;
            lane_ok = FAST && P.fast_ok && cvk::ray_fast_ok(q);
            if (P.max_iter == 0) {
              code = cvk::CODE_NONE;
              done = true;
            } else {
              active = true;
            }
          }
        }
        if (base + n >= P.total_rays) dry = true;
      }
    }
    if (!__ballot(active)) {
      if (__ballot(done)) continue; /* max_iter == 0 corner */
      if (dry) break;
      continue; /* every drawn id was tile padding: draw again */
    }
    const int thr = dry ? 64 : P.refill_threshold;
    for (;;) { /* integrate until `thr` lanes are free */
      if (active) {
        one_step<KIND, PHI, FAST>(M, P.delta, q, lane_ok);
        ++steps;
        const bool esc = ray_escaped(q.l, P.max_radius);
        if (esc | (steps >= P.max_iter)) { /* loop bound of src/systems.rs:126 */
          code = esc ? escape_code(q.l) : cvk::CODE_NONE;
          active = false;
          done = true;
        }
      }
      if (__popcll(__ballot(!active)) >= thr) break;
    }
  }
}

/* K1, static form: one ray per thread, hardware block scheduling does the load balancing.
 * FUSED: the epilogue shades the pixel itself (direction, sky lookup, RGB8 store) instead of staging the
 * final state in HBM for shade_kernel -- the epilogue needs fewer registers than the loop, so the fusion is
 * free in occupancy and removes ~200 MB of HBM traffic and one launch per frame.
 * SS: supersampling factor (1: one ray per output pixel; 2, 4, 8: P is in units of the fine grid and the epilogue averages,
 * kernels_epilogue.h resolve_store; FUSED only). */
/* Waves per SIMD that the DISC form of a kernel gives up against its plain form, from the compiler's resource report (profiles/disc_asm_diff.txt):
 * the loop carries l, phi and cos(theta) of the previous state, phi itself and the texel, nine VGPRs more.  The Ellis Euler forms
 * still fit 7 waves (71-72 VGPRs) -- all but the strict step under the mip-mapped epilogue, which spilled 16 bytes there in a trial build (73 VGPRs at 6) -- and every
 * Schwarzschild form its budget (79-80 of 96, Heun 94 of 128); the Interstellar Euler forms would spill at 5 waves (they take up to 104 at 4), the
 * Ellis Heun forms at 6 (87 at 5) and the flat ones at 7 (up to 73 at 6); the Interstellar Heun forms fit the 4 waves they have (115-117 of 128).
 * With these, no DISC kernel uses scratch.  The DISC = 2 forms (Schwarzschild alone) take their parents' registers, 80 and Heun 94, and need
 * no entry of their own (profiles/disc_motion_asm_diff.txt). */
constexpr int disc_wave_cost(int kind, int adapt, bool fast, int filter) {
  if (kind == cvk::METRIC_SCHWARZSCHILD) return 0;
  if (kind == cvk::METRIC_INTERSTELLAR) return adapt == 2 ? 0 : 1;
  if (kind == cvk::METRIC_ELLIS) return (adapt == 2 || (!fast && filter == 2)) ? 1 : 0; /* the strict step under the mip epilogue spilled 16 bytes at 7 */
  return 1;
}
template <int KIND, bool PHI, bool FAST, bool FUSED, int SS = 1, int FILTER = 0, int PROJ = 0, int ADAPT = 0, int DISC = 0> /* FILTER: option "sky_filter" (FUSED only),
  2 with option "sky_mipmap" on top: the epilogue finds every ray's (Xc, Yc), the wave exchanges them inside its 2 x 2 quads and each lane
  blends two levels of the sky's mip chain (kernels_epilogue.h sky_mip_shade);
  PROJ: 0 the reference's perspective mapping, 1 option "projection" != 0 (P.projection says which; FUSED only);
  ADAPT: 1 option "step_scale" != 0: every step takes cv_device.h step_delta(P.delta, P.kappa, l) instead of P.delta (the fused kernels and
  the debug dump's staged PHI kernel, fast step only); 2 option "integrator" = 1: a step is cv_device.h ray_step_heun with that delta_k
  (kappa = +0 while "step_scale" is off: step_delta then returns P.delta for every l);
  DISC: 1 while the context holds a disc (include/curvis_hip.h; FUSED, and the one fused form that integrates phi): the loop keeps l, phi
  and cos(theta) of the previous state, tests the sign of the cosine each step hands out -- a ballot and a scalar branch -- and, inside the
  branch, calls cv_device.h disc_crossing, gathers the texel and ends the ray where it is opaque; four register pairs and a dword more
  than the parent's loop, which costs some of the DISC kernels a wave (disc_wave_cost); 2 while that disc has a motion
  (curvis_ctx_set_disc_motion; the Schwarzschild kind alone): the texel is scaled by the emission shift inside the same branch
  (DiscShiftProbe), and the loop carries what DISC = 1 carries */
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu((kind_has_log(KIND) ? 5 : 7) - (ADAPT == 2 ? 1 : 0) - (DISC ? disc_wave_cost(KIND, ADAPT, FAST, FILTER) : 0))))
void geodesic_static(const IntegrateArgsD<ADAPT, FILTER, DISC> P) { /* the Heun step holds the saved state across two stages, four register pairs more:
  at 7 (5) waves the loop would spill them, so the ADAPT = 2 kernels ask for one wave less */
  static_assert(DISC == 0 || (FUSED && PHI), "the disc exists in the fused kernels, which then integrate phi");
  static_assert(DISC != 2 || KIND == cvk::METRIC_SCHWARZSCHILD, "a disc's motion is Keplerian: the Schwarzschild kind alone");
  static_assert(SS == 1 || (FUSED && (!PHI || DISC)), "supersampling resolves in the fused epilogue");
  static_assert(FILTER == 0 || (FUSED && (!PHI || DISC)), "the filtered lookup exists in the fused epilogues only");
  static_assert(PROJ == 0 || (FUSED && (!PHI || DISC)), "the projections exist in the fused kernels only");
  static_assert(ADAPT == 0 || (FAST && ((FUSED != PHI) || DISC)), "scaled steps exist for the fast step, in the fused kernels and the debug dump's");
  __shared__ MathTablesLds<KIND> s_tab;
  cvk::MetricParams M = P.metric;
  load_math_tables<KIND>(s_tab, M);
  const unsigned long long id = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
  const unsigned long long t_start = P.trace ? wall_clock64() : 0ull;
  unsigned frame, px, py;
  cvk::Ray q;
  q.l = q.th = q.ph = q.p1 = q.p2 = q.p3 = q.p3sq = 0.0;
  bool valid = false, active = false, lane_ok_w = false;
  unsigned steps = 0;
  int code = cvk::CODE_NONE;
  [[maybe_unused]] double t = 0.0; /* ADAPT debug dump: x[0], the reference's t + (p_t g^tt) delta_k with p_t = 1, g^tt = -1 */
  if (id < P.total_rays && decode_ray(P, id, frame, px, py)) {
    if constexpr (PROJ != 0) cvk::ray_init<KIND, true>(M, P.cams[frame], px, py + P.row0, q, P.projection, frame_boost(P.cams, P.n_frames, frame));
    else cvk::ray_init<KIND>(M, P.cams[frame], px, py + P.row0, q, PROJ ? P.projection : cvk::PROJ_PERSPECTIVE);
    if constexpr (ADAPT != 0 && PHI) t = P.cams[frame].pos[0];
    lane_ok_w = FAST && P.fast_ok && cvk::ray_fast_ok(q);
    valid = true;
    active = P.max_iter != 0;
  }
  /* All lanes of a wave start together, so the step counter is wave-uniform (an SGPR).  The loop is a plain
   * divergent loop: a lane leaves it (drops out of EXEC) when it escapes; the back-edge is "EXEC still
   * non-empty", so activity costs no VALU instruction.  The counter is recorded per lane only in the
   * iterations in which some lane escapes (a scalar branch on the ballot; the per-lane test goes through the
   * ballot mask so that the compiler keeps the block inside the loop instead of sinking it behind the exit,
   * which would cost a counter copy to a VGPR in every iteration).  Lanes still inside when the counter
   * reaches max_iterations are NotEscaped (code stays CODE_NONE). */
  [[maybe_unused]] unsigned on_disc = 0u;    /* DISC: 1 for a ray that ended on the disc, for the frame's n_disc */
  [[maybe_unused]] unsigned disc_texel = 0u; /* DISC: the texel the ray ended on; its alpha is >= 128, so non-zero says "ended on the disc" */
  if constexpr (DISC != 0) {
    /* The disc loop: the parent's, with the plane test inside the step (DiscProbe) at the point where the step from y_k has its
     * (s_k, c_k) and the state is still y_k.  A lane that ended on the disc leaves as an escaping lane does, through the same ballot; its
     * count is k, the steps before the one it was found in, and nothing of that step's result is read again -- its colour is the texel. */
    if (active) {
      const unsigned lane = threadIdx.x & 63u;
      unsigned k = 0;
      steps = P.max_iter;
      double l_prev = 0.0, ph_prev = 0.0, c_prev = 0.0;
      for (;;) {
        double dk = P.delta;
        if constexpr (ADAPT != 0) dk = cvk::step_delta(P.delta, P.kappa, q.l);
        if constexpr (DISC == 2) /* the disc has a motion: the texel is shaded where it is found */
          disc_step<KIND, FAST, ADAPT == 2>(M, dk, q, lane_ok_w, DiscShiftProbe{P.disc, P.motion, M, P.rays_per_frame, q, l_prev, ph_prev, c_prev, disc_texel, k == 0u});
        else
          disc_step<KIND, FAST, ADAPT == 2>(M, dk, q, lane_ok_w, DiscProbe{P.disc, q, l_prev, ph_prev, c_prev, disc_texel, k == 0u});
        ++k;
        const bool hit = disc_texel != 0u;
        const bool esc = hit | ray_escaped(q.l, P.max_radius);
        const unsigned long long em = __builtin_amdgcn_ballot_w64(esc);
        if (em) { /* rare, as in the parent's loop */
          unsigned kv;
          asm volatile("v_mov_b32 %0, %1" : "=v"(kv) : "s"(k));
          if ((em >> lane) & 1ull) steps = kv - (hit ? 1u : 0u);
        }
        if (esc) break;
        if (k >= P.max_iter) break;
      }
      if (disc_texel != 0u) code = cvk::CODE_DISC;
      else if (ray_escaped(q.l, P.max_radius)) code = escape_code(q.l);
    }
  } else if (active) {
    const unsigned lane = threadIdx.x & 63u;
    unsigned k = 0;
    steps = P.max_iter;
    for (;;) {
      ++k;
      if constexpr (ADAPT != 0) {
        const double dk = cvk::step_delta(P.delta, P.kappa, q.l);
        if constexpr (ADAPT == 2) {
          heun_step<KIND, PHI, FAST>(M, dk, q, lane_ok_w);
          if constexpr (PHI) t = cvk::heun_time(t, dk);
        } else {
          one_step<KIND, PHI, FAST>(M, dk, q, lane_ok_w);
          if constexpr (PHI) t = t + (1.0 * -1.0) * dk;
        }
      } else {
        one_step<KIND, PHI, FAST>(M, P.delta, q, lane_ok_w);
      }
      const bool esc = ray_escaped(q.l, P.max_radius);
      const unsigned long long em = __builtin_amdgcn_ballot_w64(esc);
      if (em) { /* rare: at most 64 times per wave.  The volatile asm keeps this a real (scalar) branch. */
        unsigned kv;
        asm volatile("v_mov_b32 %0, %1" : "=v"(kv) : "s"(k));
        if ((em >> lane) & 1ull) steps = kv;
      }
      if (esc) break;
      if (k >= P.max_iter) break;
    }
    if (ray_escaped(q.l, P.max_radius)) code = escape_code(q.l); /* the state is final: same test as in the loop */
  }
  unsigned pos = 0, neg = 0, none = 0, oob = 0;
  /* The pixel position is decoded AGAIN here, from the laundered block index, instead of being kept in registers
   * across the Euler loop (frame, px, py or a 64-bit slot: 3-4 VGPRs the loop is better off without). */
  unsigned bid = blockIdx.x;
  asm volatile("" : "+s"(bid));
  const unsigned long long id2 = (unsigned long long)bid * blockDim.x + threadIdx.x;
  valid = id2 < P.total_rays && decode_ray(P, id2, frame, px, py);
  const size_t slot = valid ? (size_t)frame * P.W * P.H + (size_t)py * P.W + px : 0;
  [[maybe_unused]] unsigned seen = 0u; /* SS > 1: what the lane's ray saw, for the resolve behind the branch */
  if constexpr (FILTER == 2) {
    unsigned which = 0u, Xc = 0u, Yc = 0u; /* the lane's sky (0: none) and its indices on it, for the exchange */
    if (valid) {
      if (code != cvk::CODE_NONE && (DISC == 0 || code != cvk::CODE_DISC)) { /* a disc ray saw no sky: which = 0 in the exchange */
        double d0, d1, d2;
        cvk::ray_direction<KIND>(M, q, d0, d1, d2);
        unsigned tx, ty;
        if (cvk::sky_fine_indices(P.sky[code == cvk::CODE_POS ? 0 : 1], d0, d1, d2, Xc, Yc, tx, ty)) oob = 1;
        which = code == cvk::CODE_POS ? 1u : 2u;
      }
      pos = (code == cvk::CODE_POS);
      neg = (code == cvk::CODE_NEG);
      none = (code == cvk::CODE_NONE);
      if constexpr (DISC != 0) on_disc = (code == cvk::CODE_DISC);
    }
    seen = sky_mip_shade(P.mip, P.sky, which, Xc, Yc); /* the whole wave: lanes outside the frame answer "none" */
    if constexpr (DISC != 0)
      if (on_disc) seen = disc_texel; /* ... then takes its own colour, unfiltered */
    if constexpr (SS == 1)
      if (valid) store_rgb8(P.fb + slot * 3, seen);
  } else if (valid) {
    if (FUSED) {
      unsigned tx, ty;
      if constexpr (DISC != 0) { /* a disc ray's colour is its texel: no direction, no lookup, no filter */
        unsigned colour;
        if (code == cvk::CODE_DISC) colour = disc_texel, on_disc = 1u;
        else colour = shade_ray<KIND, FILTER>(M, P.sky, q, code, tx, ty, oob);
        if constexpr (SS == 1) store_rgb8(P.fb + slot * 3, colour);
        else seen = colour;
      } else {
        const unsigned texel = shade_ray<KIND, FILTER>(M, P.sky, q, code, tx, ty, oob);
        /* the plain store in THIS branch: the compiler does not merge a second test of `valid` behind the shading with the first */
        if constexpr (SS == 1) store_rgb8(P.fb + slot * 3, texel);
        else seen = texel;
      }
      pos = (code == cvk::CODE_POS);
      neg = (code == cvk::CODE_NEG);
      none = (code == cvk::CODE_NONE);
    } else {
      store_ray<PHI>(P.store, slot, q, steps, code);
      if constexpr (ADAPT != 0) P.t_out[slot] = t;
    }
  }
  if constexpr (SS > 1) resolve_store<SS>(P.fb, P.W, P.H, frame, px, py, valid, seen); /* the whole wave: lanes outside the frame add nothing */
  /* statistics of the wave's tile go to the counters of ITS frame (a tile never straddles frames); on the staged
   * path shade_kernel keeps them */
  if (FUSED) flush_frame_counts(P.counters, frame_of_tile(id2 >> 6, P.rays_per_frame), valid, steps, 1u, pos, neg, none, oob);
  if constexpr (DISC != 0) flush_disc_count(P.counters, frame_of_tile(id2 >> 6, P.rays_per_frame), valid, on_disc);
  if (P.trace && (threadIdx.x & 63u) == 0) {
    unsigned hw_id, xcc_id;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw_id));
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc_id));
    unsigned long long *rec = P.trace + 4ull * (id >> 6);
    rec[0] = t_start;
    rec[1] = wall_clock64();
    rec[2] = hw_id;
    rec[3] = xcc_id;
  }
}

/* ------------------------------------------------------------------------------------------------
 * K1, relay form ("variant" = 2, launches of up to "relay_max_frames" = 8 frames): the static kernel plus a hand-over of
 * unfinished tiles in the END-GAME of the launch, with the hardware workgroup dispatcher as load balancer.
 *
 * A single-frame launch ends with ~2 ms in which no fresh workgroup is left and every SIMD finishes the 5-6
 * waves it happens to hold; the SIMDs finish between 10.8 and 12.0 ms (wave trace): ~1 ms of a
 * 12 ms frame is imbalance that cannot be repaired because a wave, once placed, stays where it is.
 *
 * Here the grid is [fresh workgroups | relay workgroups].  A fresh wave runs the static kernel's loop in
 * segments of `seg` steps.  Once every fresh workgroup has started (a counter), a wave that reaches a segment
 * boundary with unfinished rays PARKS its tile -- state of the 64 rays to HBM (56 B per ray), tile id into a
 * ticket ring -- and exits.  Its slot goes to the next relay workgroup, which the dispatcher places on
 * whichever CU has room: a relay wave takes the oldest parked tile, integrates one more segment, and parks
 * it again or shades it.  Tiles therefore drift, `seg` steps at a time, from CUs with a backlog to CUs that
 * ran dry.  There is no persistent loop (inside one it costs 86-155 VGPRs instead of 61): every
 * wave does one piece of work and exits.  Results are bit-identical: same per-ray arithmetic, state
 * round-trips through HBM as doubles.
 *
 * Ring protocol: `tail` / `head` hand out tickets; a parker writes tile+1 into slot ticket%CAP (release), a
 * relay wave waits for its slot to become non-zero (acquire) and clears it.  At most one tile per resident
 * wave is parked, CAP = 32768.  `remaining` counts unfinished tiles; waiting relay waves leave when it
 * reaches zero (their tickets are then never filled).  If the relay workgroups of a launch run out while
 * tiles are still parked, the host launches more (relay-only grid) until every tile is finished; a wave that has
 * waited ~20 s sets `error` and leaves, so a logic error shows up as CURVIS_E_HIP, not as a hang (a relay wave
 * legitimately waits at most for the rest of the launch: the kernel is meant for launches of milliseconds). */
struct RelayQueue { /* all zero before the first launch of a frame (one hipMemsetAsync) */
  unsigned long long started;  /* fresh workgroups that have begun */
  unsigned long long head, tail;
  unsigned long long finished; /* tiles shaded so far */
  unsigned long long error;
  unsigned long long pad[3];
  unsigned ring[1];            /* kRelayRing entries follow */
};
constexpr unsigned kRelayRing = 32768; /* >= resident waves (256 CUs x 32) with margin */
struct RelayArgs {
  RelayQueue *q;
  unsigned long long n_tiles;
  unsigned fresh_blocks; /* workgroups [0, fresh_blocks) start tiles, the rest relay parked ones */
  unsigned seg;          /* steps per segment */
  unsigned max_hops;     /* a tile is handed over at most this many times (0 = no limit) */
  unsigned max_parks;    /* hand-overs per launch at most (0 = no limit) */
  unsigned corrupt_ticket; /* test hook (option "relay_test_corrupt"): non-zero = every relay wave of this launch perturbs the
                              state it reloads, so that the first-launch check below has something to find; 0 = off */
};

/* Hand-over traffic of the relay kernel goes around the caches: system-scope relaxed atomics compile to
 * write-through stores / cache-bypassing loads (sc0 sc1), so publishing a tile needs only "my stores have
 * been acknowledged" (a workgroup-scope release = s_waitcnt) instead of an agent-scope release fence, which on
 * this multi-XCD part writes back the whole L2 (buffer_wbl2) -- measured ~80 us per hand-over. */
template <typename T>
__device__ __forceinline__ void st_sys(T *p, T v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM); }
template <typename T>
__device__ __forceinline__ T ld_sys(const T *p) { return __hip_atomic_load(const_cast<T *>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM); }

/* register budget: the Interstellar instantiation must stay at 5 waves per SIMD (<= 96 VGPRs; its LDS tables allow
 * no more anyway): left alone the allocator takes 97 and drops to four (+6 % time) */
template <int KIND, bool FAST, int SS = 1, int FILTER = 0, int PROJ = 0> /* SS: supersampling factor, FILTER: option "sky_filter", PROJ: option "projection", as in geodesic_static */
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(KIND == cvk::METRIC_INTERSTELLAR ? 5 : 7)))
void geodesic_relay(const IntegrateParams P, const RelayArgs A) {
  __shared__ MathTablesLds<KIND> s_tab;
  RelayQueue *const Q = A.q;
  const unsigned long long t_start = P.trace ? wall_clock64() : 0ull;
  unsigned long long t_work = 0ull; /* diagnostics: when the wave had its tile */
  const bool fresh = blockIdx.x < A.fresh_blocks;
  /* a relay workgroup that starts when every tile is finished leaves at once, before the table load: the grid
   * holds many more relay workgroups than are usually needed.  The decision is made ONCE per workgroup (thread 0
   * reads the counter, LDS + barrier hand it to the other waves): waves reading it on their own could disagree,
   * and a workgroup of which only some waves reach load_math_tables' barrier must not exist. */
  if (!fresh) {
    __shared__ int s_leave;
    if (threadIdx.x == 0)
      s_leave = __hip_atomic_load(&Q->finished, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= A.n_tiles ? 1 : 0;
    __syncthreads();
    if (s_leave) return;
  }
  cvk::MetricParams M = P.metric;
  load_math_tables<KIND>(s_tab, M);
  const unsigned lane = threadIdx.x & 63u;
  unsigned long long tile;
  bool corrupt = false;
  if (fresh) {
    if (threadIdx.x == 0) atomicAdd(&Q->started, 1ull);
    tile = ((unsigned long long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  } else {
    /* relay wave: take the oldest parked tile, or leave when every tile is finished */
    unsigned long long tk = 0;
    if (lane == 0) tk = atomicAdd(&Q->head, 1ull);
    unsigned *slot_p = Q->ring + (__builtin_amdgcn_readfirstlane((unsigned)tk) & (kRelayRing - 1u));
    unsigned v = 0, spins = 0;
    for (;;) {
      v = ld_sys(slot_p);
      if (v) break;
      /* the own ring slot is polled every ~1 us, the shared `remaining` word only every 8th time */
      if ((spins & 7u) == 0u && __hip_atomic_load(&Q->finished, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >= A.n_tiles) break;
      if (++spins > 20000000u) { /* ~20 s of waiting: longer than any launch this kernel is chosen for */
        if (lane == 0) atomicAdd(&Q->error, 1ull);
        break;
      }
      __builtin_amdgcn_s_sleep(32);
    }
    if (!v) return;
    if (lane == 0) st_sys(slot_p, 0u);
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup"); /* order the state loads below after the ticket load */
    tile = (unsigned long long)(v - 1u);
    corrupt = A.corrupt_ticket != 0u; /* test hook: every tile this launch hands over arrives perturbed */
  }
  if (P.trace) t_work = wall_clock64();
  const unsigned long long id = tile * 64ull + lane;
  unsigned frame, px, py;
  cvk::Ray q;
  q.l = q.th = q.ph = q.p1 = q.p2 = q.p3 = q.p3sq = 0.0;
  const bool valid = id < P.total_rays && decode_ray(P, id, frame, px, py);
  bool active = false;
  unsigned steps = 0, k0 = 0, hops = 0; /* hops: how often this tile has been handed over so far */
  int code = cvk::CODE_NONE;
  if (fresh) {
    if (valid) {
      cvk::ray_init<KIND>(M, P.cams[frame], px, py + P.row0, q, PROJ ? P.projection : cvk::PROJ_PERSPECTIVE);
      active = P.max_iter != 0;
      steps = P.max_iter;
    }
  } else {
    /* 40 B per parked ray: l, theta, p_l, p_theta and one packed {steps, code} word.  p_phi is a constant of the motion
     * (dp_phi = 0, src/metrics.rs:262-268; the loop never writes it): ray_init recomputes it -- and p_phi^2 -- from the
     * pixel, bit for bit what the parking wave held. */
    if (valid) cvk::ray_init<KIND>(M, P.cams[frame], px, py + P.row0, q, PROJ ? P.projection : cvk::PROJ_PERSPECTIVE);
    q.l = ld_sys(&P.store.l[id]);
    q.th = ld_sys(&P.store.th[id]);
    q.p1 = ld_sys(&P.store.p1[id]);
    q.p2 = ld_sys(&P.store.p2[id]);
    if (corrupt) { /* what a hand-over that lost stores would look like: the rays of the tile land elsewhere */
      q.th = q.th + 0.25;
      q.p1 = -q.p1;
    }
    const unsigned long long sc = ld_sys((const unsigned long long *)&P.store.ph[id]); /* the phi slot: unused outside the debug dump */
    steps = (unsigned)(sc >> 3);
    hops = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(sc >> 40)) & 0xffu; /* the same in every lane of the tile */
    const int c = (int)(sc & 7ull);
    active = (c & 4) != 0;
    code = (c & 3) == 1 ? cvk::CODE_POS : (c & 3) == 2 ? cvk::CODE_NEG : cvk::CODE_NONE;
    /* the step counter is wave-uniform: every active lane parked it in `steps` (a parked tile has one) */
    const unsigned long long am = __builtin_amdgcn_ballot_w64(active);
    k0 = __builtin_amdgcn_readlane(steps, am ? (int)__builtin_ctzll(am) : 0);
    if (active) steps = P.max_iter;
  }
  const bool lane_ok_w = FAST && P.fast_ok && cvk::ray_fast_ok(q);
  const unsigned SEG = A.seg;
  bool parked = false;
  for (;;) {
    const unsigned seg_end = (P.max_iter - k0 > SEG) ? k0 + SEG : P.max_iter;
    if (active) {
      unsigned k = k0;
      for (;;) {
        ++k;
        one_step<KIND, false, FAST>(M, P.delta, q, lane_ok_w);
        const bool esc = ray_escaped(q.l, P.max_radius);
        const unsigned long long em = __builtin_amdgcn_ballot_w64(esc);
        if (em) { /* rare; the volatile asm keeps this a real (scalar) branch */
          unsigned kv;
          asm volatile("v_mov_b32 %0, %1" : "=v"(kv) : "s"(k));
          if ((em >> lane) & 1ull) steps = kv;
        }
        if (esc) break;
        if (k >= seg_end) break;
      }
      if (ray_escaped(q.l, P.max_radius)) {
        code = escape_code(q.l);
        active = false;
      }
    }
    k0 = seg_end;
    if (!__builtin_amdgcn_ballot_w64(active) || k0 >= P.max_iter) break; /* tile finished */
    /* keep the tile while fresh workgroups are still being started, and afterwards unless a relay wave is
     * waiting for a ticket right now (head > tail): a hand-over then costs the tile ~1 us, whereas a tile parked
     * with nobody waiting would sit idle until the dispatcher has placed another relay workgroup */
    if (fresh && __hip_atomic_load(&Q->started, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < (unsigned long long)A.fresh_blocks)
      continue;
    {
      const unsigned long long tail_now = __hip_atomic_load(&Q->tail, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (__hip_atomic_load(&Q->head, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) <= tail_now) continue;
      if (A.max_parks != 0u && tail_now >= A.max_parks) continue; /* hand-over budget of the launch spent */
    }
    /* a tile that has been handed over `max_hops` times stays where it is: every hop costs 2 x 64 x 40 B of HBM traffic */
    if (!fresh && A.max_hops != 0u && hops >= A.max_hops) continue;
    parked = true;
    break;
  }
  unsigned pos = 0, neg = 0, none = 0, oob = 0;
  if (parked) {
    st_sys(&P.store.l[id], q.l);
    st_sys(&P.store.th[id], q.th);
    st_sys(&P.store.p1[id], q.p1);
    st_sys(&P.store.p2[id], q.p2);
    st_sys((unsigned long long *)&P.store.ph[id],
           ((unsigned long long)(hops < 255u ? hops + 1u : 255u) << 40) | ((unsigned long long)(active ? k0 : steps) << 3) |
               (unsigned long long)((code == cvk::CODE_POS ? 1 : code == cvk::CODE_NEG ? 2 : 0) | (active ? 4 : 0)));
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup"); /* every lane's write-through stores acknowledged */
    if (lane == 0) {
      const unsigned long long tk = atomicAdd(&Q->tail, 1ull);
      st_sys(Q->ring + ((unsigned)tk & (kRelayRing - 1u)), (unsigned)tile + 1u);
    }
  } else {
    /* pixel position decoded again from the laundered tile number rather than kept live across the loop */
    unsigned tile_s = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)tile);
    asm volatile("" : "+s"(tile_s));
    const unsigned long long id2 = (unsigned long long)tile_s * 64ull + lane;
    unsigned frame2 = 0, px2 = 0, py2 = 0, texel = 0u;
    const bool valid2 = id2 < P.total_rays && decode_ray(P, id2, frame2, px2, py2);
    if (valid2) {
      unsigned tx, ty;
      texel = shade_ray<KIND, FILTER>(M, P.sky, q, code, tx, ty, oob);
      if constexpr (SS == 1) store_rgb8(P.fb + ((size_t)frame2 * P.W * P.H + (size_t)py2 * P.W + px2) * 3, texel); /* as in geodesic_static */
      pos = (code == cvk::CODE_POS);
      neg = (code == cvk::CODE_NEG);
      none = (code == cvk::CODE_NONE);
    }
    /* the wave that finishes a tile holds all 64 of its rays, parked on the way or not: supersampled, it averages them */
    if constexpr (SS > 1) resolve_store<SS>(P.fb, P.W, P.H, frame2, px2, py2, valid2, texel);
    if (lane == 0 && tile < A.n_tiles) atomicAdd(&Q->finished, 1ull);
  }
  /* a tile is counted once, by the wave that finishes it, in the counters of its frame */
  flush_frame_counts(P.counters, frame_of_tile(tile, P.rays_per_frame), valid && !parked, steps, 1u, pos, neg, none, oob);
  if (P.trace && lane == 0) { /* CURVIS_TRACE_FILE: {start, end, HW_ID, XCC_ID | flags, got-tile time, tile} per wave */
    unsigned hw_id, xcc_id;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw_id));
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc_id));
    unsigned long long *rec = P.trace + 4ull * ((unsigned long long)blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6));
    rec[0] = t_start;
    rec[1] = wall_clock64();
    rec[2] = (unsigned long long)hw_id | ((unsigned long long)(xcc_id & 0xf) << 32) | ((unsigned long long)(fresh ? 1 : 0) << 40) |
             ((unsigned long long)(parked ? 1 : 0) << 41) | ((unsigned long long)(k0 & 0xffff) << 44);
    rec[3] = t_work;
  }
}

/* seat belt of the relay kernel: number of differing 8-byte words of two framebuffers (one atomic per thread that saw one:
 * none at all in the expected case) */
__global__ __launch_bounds__(256) void compare_kernel(const unsigned long long *a, const unsigned long long *b, size_t n_words,
                                                      unsigned long long *n_diff) {
  size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  unsigned mine = 0;
  for (; i < n_words; i += stride) mine += a[i] != b[i];
  if (mine) atomicAdd(n_diff, (unsigned long long)mine);
}

/* K2: final photon -> tangent direction -> nearest sky texel -> RGB8 (rows R9-R10 of SURVEY.md 8a).
 * One thread per pixel, coalesced reads of the ray store, 3-byte stores of consecutive pixels. */
template <int KIND, bool DEBUG>
__global__ __launch_bounds__(256) void shade_kernel(const ShadeParams P) {
  const unsigned long long o = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x;
  unsigned pos = 0, neg = 0, none = 0, oob = 0, n_steps = 0;
  const bool valid = o < P.n_pixels;
  if (valid) {
    cvk::Ray q;
    q.l = P.store.l[o];
    q.th = P.store.th[o];
    q.ph = DEBUG ? P.store.ph[o] : 0.0;
    q.p1 = P.store.p1[o];
    q.p2 = P.store.p2[o];
    q.p3 = P.store.p3[o];
    q.p3sq = 0.0;
    const int code = P.store.code[o];
    const unsigned steps = P.store.steps[o];
    n_steps = steps;
    unsigned tx, ty;
    cvk::MetricParams M = P.metric;
    M.T = cv_sc_table();
    M.LT = cv_log_table();
    M.AT = cv_atan_table();
    const unsigned texel = shade_ray<KIND>(M, P.sky, q, code, tx, ty, oob);
    store_rgb8(P.fb + o * 3, texel);
    pos = (code == cvk::CODE_POS);
    neg = (code == cvk::CODE_NEG);
    none = (code == cvk::CODE_NONE);
    if (DEBUG) {
      curvis_ray_debug *d = P.dbg + o;
      d->x[0] = 0.0; /* t and p_t: dead lanes of the integrator, filled in by the host */
      d->x[1] = q.l;
      d->x[2] = q.th;
      d->x[3] = q.ph;
      d->p[0] = 1.0;
      d->p[1] = q.p1;
      d->p[2] = q.p2;
      d->p[3] = steps ? q.p3 + 0.0 : q.p3; /* p3 + 0.0*delta of the reference (-0 -> +0) */
      d->steps = steps;
      d->code = code;
      d->tx = tx;
      d->ty = ty;
    }
  }
  flush_frame_counts(P.counters, (unsigned)(o / P.npix), valid, n_steps, 1u, pos, neg, none, oob);
}

}  // namespace
