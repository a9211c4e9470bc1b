/* render_host.h -- host side of the per-pixel path: struct curvis_ctx, the metric / step-flavour dispatcher, the one launch of the
 * kernel family that brute_plan.h names, render_impl and its pieces (the facts of a call, one chunk of frames, the relay seat belt),
 * per-frame statistics.
 * Part of the ONE translation unit curvis_hip.hip (included there, nowhere else). */
#pragma once

namespace {

/* ------------------------------------------------------------------------------------------ host */

thread_local std::string g_create_error;

}  // namespace

/* Every HIP resource below is held by an owning type of hip_owned.h, so `delete ctx` releases them all (curvis_ctx_destroy
 * synchronises the streams first: that, not the order of the members, is what makes the order of destruction immaterial). */
struct curvis_ctx {
  int device = -1;
  Stream stream;
  Event ev0, ev1;
  hipDeviceProp_t prop{};
  std::string err;
  /* skies */
  SkyTexture sky[2];
  double sky_inv_rot[2][9];
  /* the accretion disc (include/curvis_hip.h): at most one, the context's own copy of its texture; the brute renderer's DISC kernels read it */
  DeviceBuffer<unsigned> d_disc;
  bool disc_set = false;
  unsigned disc_w = 0, disc_h = 0;
  double disc_l_in = 0.0, disc_l_out = 0.0;
  /* the disc's emission shift (curvis_ctx_set_disc_motion): the context's, whether a disc is set or not; with a motion the brute
   * renderer launches the DISC = 2 kernels, which read one camera factor per frame (cv_device.h disc_camera_factor, evaluated here) */
  int disc_motion = 0;
  double disc_gain = 1.0;
  DeviceBuffer<double> d_disc_cam;
  PinnedBuffer<double> h_disc_cam;
  std::vector<uint64_t> last_frame_disc; /* rays that ended on the disc, per frame of the last brute render (curvis_ctx_frame_disc_hits) */
  /* frame resources */
  DeviceBuffer<unsigned char> d_fb;
  size_t fb_bytes = 0;
  /* overlapped download (option "async_download", fb_begin_write / fb_download below): a copy stream of its own, the second
   * frame buffer the next render call writes while the copy engine still reads the first, and the one download in flight */
  int async_download = 0;
  Stream copy_stream;
  Event ev_fb, ev_dl; /* frames complete on `stream` / download complete on `copy_stream` */
  DeviceBuffer<unsigned char> d_fb_alt;
  bool dl_pending = false;
  const unsigned char *dl_src = nullptr;       /* the device buffer the pending download reads */
  uint64_t downloads_overlapped = 0;           /* downloads queued behind the caller's back so far (option, read-only) */
  /* option "async_streams": curvis_ctx_deflate_frames returns while its streams are still on their way to the caller's buffer (copy
   * stream); they are there after curvis_ctx_download_wait, and before the next deflate call touches the scratch they are read from */
  int async_streams = 0;
  bool streams_pending = false;
  Event ev_streams;
  DeviceBuffer<curvis_ray_debug> d_dbg;
  DeviceBuffer<double> d_dbg_t;         /* option "step_scale": x[0] of every ray of a debug dump, integrated on the device */
  DeviceBuffer<unsigned char> d_store;  /* RayStore arrays, carved from one allocation */
  DeviceBuffer<unsigned char> d_rq;     /* RelayQueue + ticket ring of the relay kernel */
  DeviceBuffer<unsigned char> d_verify; /* copy of the relay kernel's frame while the static kernel re-renders it (seat belt) */
  DeviceBuffer<unsigned char> d_png;    /* scratch of the device PNG front end (kernels_png.h): histograms, codes, offsets, streams */
  double last_png_ms = 0.0;          /* HIP-event time of the last curvis_ctx_deflate_frames */
  size_t last_png_stream_bytes = 0;  /* bytes the streams of the last curvis_ctx_deflate_frames take (also when it failed for want of room) */
  int relay_segment = 0;            /* steps between two hand-over points; 0 = automatic */
  int relay_max_hops = 0;           /* hand-overs per tile at most; 0 = no limit */
  int relay_max_parks = 0;          /* hand-overs per launch at most; 0 = no limit */
  int relay_max_frames = 8;         /* largest launch (frames) the relay kernel is used for: the end-game it repairs is
                                       ~5 % of a one-frame launch and 1-2 % of a launch of three to six frames;
                                       beyond that its staging area (56 B per ray) buys nothing */
  int relay_disabled = 0;           /* set when a relay launch reported waves that gave up waiting: the context falls back
                                       to the static kernel for good (the relay kernel leans on the dispatcher starting
                                       workgroups in blockIdx order, which HIP does not promise) */
  int relay_verify = 0;             /* debug option: every relay render is repeated with the static kernel and the two
                                       frames and statistics compared (CURVIS_E_HIP on a difference) */
  int relay_test_fault = 0;         /* test hook: pretend the next relay launch reported a wave that gave up */
  int relay_test_corrupt = 0;       /* test hook: the next relay launch perturbs the first tile it hands over */
  int relay_auto_verify = 1;        /* seat belt (default on): the FIRST relay launch of every launch shape (W, H, frames, metric,
                                       step flavour) of this context is repeated by the static kernel and compared; on a
                                       difference the context drops to the static kernel for good (relay_mismatches counts) */
  uint32_t relay_mismatches = 0;
  /* launch shapes of the relay kernel -> relay launches of that shape so far; the first and then every
   * relay_recheck_every-th is repeated by the static kernel and compared */
  std::map<std::array<uint32_t, 9>, uint64_t> relay_verified;
  int relay_recheck_every = 1024;
  uint64_t relay_checks = 0;        /* launches checked so far */
  uint32_t relay_fallbacks = 0;     /* renders that fell back from the relay to the static kernel */
  long long relay_min_blocks = -1;  /* smallest grid (fresh workgroups) the relay kernel is used for; -1 = automatic
                                       (4 per CU: with fewer workgroups than that nearly the whole grid is resident at
                                       once, there is no dispatch phase, and the static kernel is as good) */
  uint32_t last_relay_launches = 0;
  uint64_t last_relay_parks = 0, last_relay_waiters = 0;
  unsigned relay_resident_blocks[2][2][4][3][2] = {}; /* cached occupancy query per kernel instantiation: [projection != 0][sky_filter][log2 supersample][kind][fast]; the kind is Ellis, Interstellar or flat: the relay kernel is not instantiated for Schwarzschild */
  int relay_resident_threads = 0;                                  /* ... valid for this workgroup size */
  int block_threads = 0; /* workgroup size of the static / relay kernels: 64, 128 or 256; 0 = automatic */
  Event ev2;
  /* efficient mode scratch (device) */
  DeviceBuffer<unsigned char> d_eff;
  PinnedBuffer<unsigned char> h_eff; /* staging mirror of d_eff for the sampling launches */
  /* sample tables of the last efficient render, per frame (for tests / statistics) */
  std::vector<std::vector<cvs::BiPoint>> last_samples;
  std::vector<curvis_sampling_info> last_sampling_info;
  DeviceBuffer<cvk::CameraParams> d_cams;
  PinnedBuffer<cvk::CameraParams> h_cams;
  DeviceBuffer<unsigned long long> d_counters; /* FrameCounters block, sized for the largest launch so far */
  PinnedBuffer<unsigned long long> h_counters; /* mirror (+ 8 words for the relay queue header) */
  /* statistics of the last render, per frame (curvis_ctx_frame_stats) */
  std::vector<curvis_stats> last_frame_stats;
  /* options */
  int variant = -1;         /* -1 automatic (default): relay kernel for launches of up to relay_max_frames frames and at least
                               relay_min_blocks workgroups, static kernel otherwise;
                               1 static one-ray-per-thread, 2 relay (subject to relay_min_blocks), 0 persistent lane-refill */
  int refill_threshold = 16;
  int blocks_per_cu = 0;    /* 0 = occupancy query */
  int fast_math = 1;        /* 1 shared-reciprocal step (ray_step_fast), 0 compiler IEEE div/sqrt */
  int fuse_shade = 1;       /* static kernel shades in its epilogue (no ray store, no shade launch) */
  int supersample = 1;      /* N in {1, 2, 4, 8}: every render call traces N x N rays per pixel of the cameras' resolution and the
                               kernels' epilogues average them (kernels_epilogue.h resolve_store); frames stay res_x x res_y */
  int sky_filter = 0;       /* 0: a ray takes the nearest sky texel (the reference); 1: the bilinear blend of the four around its
                               direction, defined in include/curvis_hip.h (cv_device.h sky_bilinear_taps / sky_bilinear_blend) */
  int sky_mipmap = 0;       /* 1 (on top of sky_filter = 1): the bilinear blend on a mip pyramid of the sky, the level chosen per ray from
                               its quad neighbours -- defined in include/curvis_hip.h (cv_device.h sky_mip_*; the kernels' FILTER = 2) */
  int pixel_tiled = 0;      /* measurement switch (tools/gpu_sky_mipmap_cost.py): 1 = the efficient renderer's per-pixel launch enumerates
                               pixels by 8x8 tiles even where the linear kernel would do, so that the enumeration is timed on its own */
  int64_t last_sky_mip_build_us = 0; /* HIP-event time of the last mip chain build (its launches alone), microseconds */
  int64_t last_sky_copy_us = 0;      /* HIP-event time of the last device-to-device sky copy (curvis_ctx_set_sky_device, copy = 1) */
  int last_pixel_tiled = 0; /* the efficient renderer's last per-pixel launch: 0 efficient_pixel_kernel (linear), 1 the tile-enumerating one */
  int projection = 0;       /* 0: the reference's perspective camera; 1: equirectangular; 2: equidistant fisheye -- pixel -> camera-space
                               vector, defined in include/curvis_hip.h (cv_device.h camera_pixel_vector) */
  std::vector<double> cam_beta; /* curvis_ctx_set_camera_velocities: (b_l, b_theta, b_phi) per triple, validated when set; empty: every
                                   camera is static.  One triple serves every frame of a call, n triples a call of n frames
                                   (prepare_camera_boost) */
  int integrator = 0;       /* 0: forward Euler, the reference's loop; 1: Heun's method composed of two Euler steps -- defined in
                               include/curvis_hip.h (cv_device.h ray_step_heun) */
  int64_t step_scale = 0;   /* S in [0, 2^20]; 0: every Euler step takes the call's delta (the reference).  S != 0: L0 = S / 256, and a step
                               from radial coordinate l takes max(delta, |l| delta / L0) -- defined in include/curvis_hip.h (cv_device.h
                               step_delta) */
  int sampling_speculation = -1; /* efficient renderer: depth of the speculative subtree evaluated below every
                                    refined interval (0 = one launch per refinement round, no speculation;
                                    -1 = automatic: 10 for one or two frames, 6 for three to five, 4 for larger batches;
                                    at most 11) */
  int sampling_speculation_first = -1; /* the same for the first launch (below the uniform grid); -1 = automatic: 8 / 4 / 3 */
  int device_sampler = -1;           /* efficient renderer: 1 = sampler_kernel (device-resident refinement loop), 0 = host-paced sampler with
                                        speculation, -1 = automatic: the device for calls of device_sampler_min_frames frames and more */
  int device_sampler_min_frames = 48; /* measured cross-over against the host-paced sampler: between 32 and 64 frames per call (profiles/round6_eff_device_sampler.txt) */
  int last_sampler_path = 0;         /* of the last render_efficient call: 0 host-paced, 1 device, 2 device -> fell back to the host (overflow) */
  /* device-resident sampler: two slots (device buffer + page-locked mirror each) that take turns -- a call samples into one on its own
   * stream, or finds one filled ahead of time by curvis_ctx_prefetch_efficient on `sampler_stream`; the tables of the last render
   * stay readable in their slot (curvis_ctx_samples) until that slot is submitted to again, i.e. for one more submission */
  struct SamplerKey { /* what the tables of a sampler launch depend on (efficient_host.h sampler_key_equal) */
    curvis_metric metric{};
    uint32_t n_frames = 0, max_iter = 0, alpha_nums = 0, max_iterations_sampling = 0;
    double max_radius = 0, delta = 0, thr1 = 0, thr2 = 0;
    int fast = 0, speculate = 0;
    int64_t step_scale = 0; /* option "step_scale": other steps, other tables */
    int integrator = 0;     /* option "integrator": likewise */
    std::vector<double> l_frame; /* radial coordinate of every frame's camera */
  };
  struct SamplerSlot {
    bool valid = false, prefetched = false;
    DeviceBuffer<unsigned char> d;
    PinnedBuffer<unsigned char> h;
    size_t res_bytes = 0, h_res_off = 0;
    size_t o_tab_off = 0, o_tab_n = 0, o_grid_off = 0, o_grid = 0, o_res = 0, o_tab[7] = {0, 0, 0, 0, 0, 0, 0};
    Event done, t0, t1;
    std::vector<unsigned> job_of_frame;
    std::vector<double> l_job;
    SamplerKey key;
    uint64_t seq = 0; /* order of submission */
  } samp[2];
  unsigned samp_next = 0;
  uint64_t samp_seq = 0;
  Stream sampler_stream;
  uint64_t prefetches = 0, prefetch_hits = 0;
  int last_sampling_prefetched = 0;
  struct DevSamples {                /* which slot holds the tables of the last device-sampled call (curvis_ctx_samples fetches on demand) */
    bool valid = false, overwritten = false;
    unsigned slot = 0;
  } dev_samples;
  struct PixRecips {                 /* efficient pixel kernel: reciprocals of the call's constant denominators, formed on the device once
                                        per resolution (efficient_host.h ensure_pixel_recips) */
    bool valid = false;
    double res_x = 0.0, res_y = 0.0;
    cvk::PixelRecips y{};
  } pix_recips;
  uint32_t last_sampling_chains = 0; /* device sampler: Euler chains (rounds that had to integrate) of the slowest job of the last call */
  uint32_t last_sampling_launches = 0;
  uint64_t last_sampling_evaluated = 0;
  size_t max_store_bytes = (size_t)8 << 30; /* frames of a batch are rendered in chunks below this */
  double last_integrate_ms = 0.0, last_shade_ms = 0.0;
};

namespace {

int fail(curvis_ctx *ctx, int code, const std::string &msg) {
  if (ctx)
    ctx->err = msg;
  else
    g_create_error = msg;
  return code;
}

/* ---- the metric kind and the step flavour, from run-time values to template arguments -----------------------------------
 * with_kind(kind, [&](auto K) { ... decltype(K)::value ... }) calls the lambda with the kind as a type; an unknown kind is FLAT
 * (curvis_metric_validate is what refuses it).  with_flag does the same for a bool.  The lambda's result is the call's result:
 * HIP_TRY inside it returns from the LAMBDA, so a caller hands that int on. */
template <typename F>
auto with_kind(int kind, F &&f) {
  switch (kind) {
    case CURVIS_METRIC_ELLIS: return f(std::integral_constant<int, cvk::METRIC_ELLIS>{});
    case CURVIS_METRIC_INTERSTELLAR: return f(std::integral_constant<int, cvk::METRIC_INTERSTELLAR>{});
    case CURVIS_METRIC_SCHWARZSCHILD: return f(std::integral_constant<int, cvk::METRIC_SCHWARZSCHILD>{});
    default: return f(std::integral_constant<int, cvk::METRIC_FLAT>{});
  }
}
template <typename F>
auto with_flag(bool flag, F &&f) {
  return flag ? f(std::true_type{}) : f(std::false_type{});
}
/* The whole shape of a render launch -- metric kind, step flavour, supersampling factor, sky filter, projection -- as ONE type:
 * with_launch_shape(kind, fast, ss, filter, projection, [&](auto S) { using T = decltype(S); ... T::KIND, T::FAST, T::SS, T::FILTER,
 * T::PROJ ... }) calls the lambda once.  ss is 1, 2, 4 or 8 and filter 0 or 1: the writers of the options "supersample" and
 * "sky_filter" admit nothing else; filter = 2 is "sky_filter" = 1 with "sky_mipmap" = 1 on top (prepare_call_shape).  PROJ is 1 for every projection but the perspective one: which of them is a kernel argument. */
template <int KIND_, bool FAST_, int SS_, int FILTER_, int PROJ_, int ADAPT_ = 0>
struct LaunchShape {
  static constexpr int KIND = KIND_, SS = SS_, FILTER = FILTER_, PROJ = PROJ_, ADAPT = ADAPT_;
  static constexpr bool FAST = FAST_;
};
/* adapt: 0, 1 option "step_scale" != 0 under the Euler step, 2 option "integrator" = 1 (ADAPT != 0 exists for the fast step only:
 * prepare_call_shape refuses both options with fast_math = 0) */
template <typename F>
auto with_launch_shape(int kind, bool fast, uint32_t ss, uint32_t filter, uint32_t projection, int adapt, F &&f) {
  return with_kind(kind, [&](auto K) {
    return with_flag(fast, [&](auto A) {
      auto with_ss = [&](auto N) {
        constexpr int KIND = decltype(K)::value, SS = decltype(N)::value;
        constexpr bool FAST = decltype(A)::value;
        if constexpr (FAST)
          if (adapt) {
            auto with_adapt = [&](auto D) {
              constexpr int ADAPT = decltype(D)::value;
              if (filter == 2u) return projection ? f(LaunchShape<KIND, FAST, SS, 2, 1, ADAPT>{}) : f(LaunchShape<KIND, FAST, SS, 2, 0, ADAPT>{});
              if (projection) return filter ? f(LaunchShape<KIND, FAST, SS, 1, 1, ADAPT>{}) : f(LaunchShape<KIND, FAST, SS, 0, 1, ADAPT>{});
              return filter ? f(LaunchShape<KIND, FAST, SS, 1, 0, ADAPT>{}) : f(LaunchShape<KIND, FAST, SS, 0, 0, ADAPT>{});
            };
            return adapt == 2 ? with_adapt(std::integral_constant<int, 2>{}) : with_adapt(std::integral_constant<int, 1>{});
          }
        if (filter == 2u) return projection ? f(LaunchShape<KIND, FAST, SS, 2, 1>{}) : f(LaunchShape<KIND, FAST, SS, 2, 0>{});
        if (projection) return filter ? f(LaunchShape<KIND, FAST, SS, 1, 1>{}) : f(LaunchShape<KIND, FAST, SS, 0, 1>{});
        return filter ? f(LaunchShape<KIND, FAST, SS, 1, 0>{}) : f(LaunchShape<KIND, FAST, SS, 0, 0>{});
      };
      switch (ss) {
        case 2: return with_ss(std::integral_constant<int, 2>{});
        case 4: return with_ss(std::integral_constant<int, 4>{});
        case 8: return with_ss(std::integral_constant<int, 8>{});
        default: return with_ss(std::integral_constant<int, 1>{});
      }
    });
  });
}
inline unsigned supersample_log2(uint32_t ss) { return ss == 8 ? 3u : ss == 4 ? 2u : ss == 2 ? 1u : 0u; }

/* the filter indexes the virtual sky of 256 w x 256 h texels with 32-bit numbers */
constexpr uint32_t kSkyFilterMaxSide = 1u << 23;
/* What the options "supersample", "sky_filter" and "projection" make of a render call, for all three renderers: the factor, the
 * filter, the projection, and
 * -- ss > 1 -- the cameras of the call over the ss times finer grid: the same sensor at ss times the resolution (pixel (ss x, ss y)
 * of it is pixel (x, y) of the original, cv_device.h ray_init). */
struct CallShape {
  uint32_t ss = 1, filter = 0, projection = 0; /* projection: the option's value, with cvk::PROJ_BOOSTED on top while a frame of the call moves */
  std::vector<cvk::CameraBoost> boost;         /* then: one per frame (a frame at rest has B = 0), else empty */
  double kappa = 0.0; /* option "step_scale" != 0: RN(delta / L0), else +0 (read under "integrator" = 1 only: step_delta then gives delta) */
  int adapt = 0;      /* the kernels' ADAPT: 2 option "integrator" = 1, else 1 option "step_scale" != 0, else 0 */
  std::vector<curvis_camera> fine;
};
/* Option "step_scale" for a call with step delta: off (adapt = false), or kappa = RN(delta / L0) with L0 = S / 256 (exact), one IEEE
 * division, here and nowhere else.  The option needs a positive delta and the fast step (the strict step exists for the theorem about
 * the reference's own frames, and has no ADAPT kernels). */
int step_scale_kappa(curvis_ctx *ctx, double delta, double &kappa, int &adapt) {
  kappa = 0.0;
  adapt = ctx->integrator != 0 ? 2 : ctx->step_scale != 0 ? 1 : 0;
  if (!adapt) return CURVIS_OK;
  /* Option "integrator" = 1 (Heun) has the same two needs, for the same reasons, and is refused under its own name while "step_scale"
   * is off.  Its kernels are the ADAPT = 2 ones, which take delta_k from step_delta whether or not the steps are scaled: with kappa = +0,
   * |l| kappa is 0 or NaN and the maximum with delta > 0 is delta, for every l. */
  if (!(delta > 0.0))
    return fail(ctx, CURVIS_E_INVALID, ctx->step_scale != 0 ? "step_scale != 0: the step delta must be greater than 0"
                                                            : "integrator = 1: the step delta must be greater than 0");
  if (ctx->fast_math == 0)
    return fail(ctx, CURVIS_E_INVALID,
                ctx->step_scale != 0 ? "step_scale != 0: fast_math = 0 (the strict step) takes the reference's fixed step only (set step_scale = 0)"
                                     : "integrator = 1: fast_math = 0 (the strict step) takes the reference's Euler step only (set integrator = 0)");
  if (ctx->step_scale != 0) kappa = cvk::step_kappa(delta, ctx->step_scale);
  return CURVIS_OK;
}
/* The moving camera (curvis_ctx_set_camera_velocities) for a call of n_frames frames: which triple serves which frame, and the five
 * doubles of every frame from its own rot (cv_device.h camera_boost_prepare).  A call none of whose frames moves keeps an empty
 * s.boost and is the call it would be with the velocities cleared. */
int prepare_camera_boost(curvis_ctx *ctx, const curvis_camera *cams, uint32_t n_frames, CallShape &s) {
  s.boost.clear();
  const size_t n = ctx->cam_beta.size() / 3;
  if (n == 0) return CURVIS_OK;
  if (n != 1 && n != n_frames)
    return fail(ctx, CURVIS_E_INVALID, "camera velocity: " + std::to_string(n) + " velocities are set for a call of " + std::to_string(n_frames) +
                                           " frame(s) (set one for all frames, one per frame, or none)");
  std::vector<cvk::CameraBoost> K(n_frames);
  bool moving = false;
  for (uint32_t f = 0; f < n_frames; ++f) {
    const int rc = cvk::camera_boost_prepare(cams[f].rot, &ctx->cam_beta[n == 1 ? 0 : 3 * (size_t)f], K[f]);
    if (rc < 0) return fail(ctx, CURVIS_E_INVALID, "camera velocity: the speed of frame " + std::to_string(f) + " in its camera's frame is not below 1 (the speed of light)");
    moving = moving || rc > 0;
  }
  if (moving) s.boost.swap(K);
  return CURVIS_OK;
}
/* the cameras of a call as the kernels read them: n CameraParams and, while a frame moves, the n CameraBoost behind them
 * (kernels_geodesic.h frame_boost) */
size_t staged_cameras_bytes(uint32_t n, const cvk::CameraBoost *boost) { return (sizeof(cvk::CameraParams) + (boost ? sizeof(cvk::CameraBoost) : 0)) * (size_t)n; }
void stage_cameras(unsigned char *dst, const curvis_camera *cams, uint32_t n, const cvk::CameraBoost *boost);

/* cams: the caller's n_frames cameras on entry, those the kernels run over on return (s.fine with ss > 1).  With the filter on, both
 * skies must be small enough for it; a fisheye whose image corner lies beyond the angle pi from the axis is refused; too_large is the renderer's message for a fine resolution that no longer fits 32 bits.
 * boost_prepared: s.boost is the call's already (render_impl, whose plan reads it before it comes here). */
int prepare_call_shape(curvis_ctx *ctx, const curvis_camera *&cams, uint32_t n_frames, double delta, const char *too_large, CallShape &s,
                       bool boost_prepared = false) {
  if (int rc = step_scale_kappa(ctx, delta, s.kappa, s.adapt)) return rc;
  s.ss = (uint32_t)ctx->supersample;
  s.filter = (uint32_t)ctx->sky_filter;
  if (ctx->sky_mipmap) { /* the kernels' FILTER = 2: the mip-mapped lookup acts on top of the bilinear one */
    if (!s.filter) return fail(ctx, CURVIS_E_INVALID, "sky_mipmap = 1: the mip-mapped lookup acts on top of the bilinear filter (set sky_filter = 1)");
    s.filter = 2u;
  }
  if (s.filter)
    for (const auto &sky : ctx->sky)
      if (sky.texels && (sky.w > kSkyFilterMaxSide || sky.h > kSkyFilterMaxSide))
        return fail(ctx, CURVIS_E_INVALID, "sky_filter = 1: a sky of more than 2^23 texels per side (256 times its size must fit 32 bits)");
  s.projection = (uint32_t)ctx->projection;
  if (!boost_prepared)
    if (int rc = prepare_camera_boost(ctx, cams, n_frames, s)) return rc;
  if (s.projection == (uint32_t)cvk::PROJ_FISHEYE)
    for (uint32_t f = 0; f < n_frames; ++f) {
      const curvis_camera &c = cams[f];
      if (!(0.5 * std::sqrt(c.sensor_w * c.sensor_w + c.sensor_h * c.sensor_h) / c.focal <= CV_PI))
        return fail(ctx, CURVIS_E_INVALID, "projection = 2 (fisheye): half the sensor's diagonal over the focal length exceeds pi");
    }
  if (!s.boost.empty()) s.projection |= (uint32_t)cvk::PROJ_BOOSTED;
  if (s.ss <= 1u) return CURVIS_OK;
  s.fine.assign(cams, cams + n_frames);
  for (curvis_camera &c : s.fine) {
    if ((uint64_t)c.res_x * s.ss > 0xFFFFFFFFull || (uint64_t)c.res_y * s.ss > 0xFFFFFFFFull) return fail(ctx, CURVIS_E_INVALID, too_large);
    c.res_x *= s.ss;
    c.res_y *= s.ss;
  }
  cams = s.fine.data();
  return CURVIS_OK;
}

/* The Schwarzschild kind in a render call (all three renderers): the coordinate l > 0 is the whole exterior, l <= 0 is the funnel that
 * swallows captured rays (include/curvis_hip.h) -- no place for a camera. */
int schwarzschild_camera_check(curvis_ctx *ctx, const curvis_metric *metric, const curvis_camera *cams, uint32_t n_frames) {
  if (metric->kind != CURVIS_METRIC_SCHWARZSCHILD) return CURVIS_OK;
  for (uint32_t f = 0; f < n_frames; ++f)
    if (!(cams[f].pos[1] > 0.0)) return fail(ctx, CURVIS_E_INVALID, "Schwarzschild metric: the camera's radial coordinate l must be greater than 0 (l <= 0 is the capture funnel)");
  return CURVIS_OK;
}

/* ---- overlapped download of the frames (option "async_download" = 1) -------------------------------------------------
 * The reference's render_image returns an owned host image (src/systems.rs:314-329), so a host that calls one render per
 * frame pays the PCIe copy after every kernel: +0.25 ms on a 10.2 ms 1080p frame (bench.py: value_with_download, -2.4 %).
 * With the option set a render call given `rgb_out` returns when its kernels are done and the copy is QUEUED on the
 * context's copy stream; the next call renders into the OTHER frame buffer while the copy engine drains the first, and,
 * before it queues its own download, waits for the previous one (long finished: it ran under this call's kernels).  So the
 * contract is a pipeline one frame deep: `rgb_out` of call k is complete when call k + 1 on the same context returns, or
 * after curvis_ctx_download_wait.  ctx->d_fb is always the buffer of the LAST render (what curvis_ctx_deflate_frames,
 * curvis_ctx_download and the seat belt read); only a call that is about to WRITE frames steps aside. */
int download_wait(curvis_ctx *ctx) {
  if (ctx->streams_pending) { /* option "async_streams": the zlib streams of the last deflate call */
    ctx->streams_pending = false;
    HIP_TRY(ctx, hipEventSynchronize(ctx->ev_streams));
  }
  if (!ctx->dl_pending) return CURVIS_OK;
  ctx->dl_pending = false;
  ctx->dl_src = nullptr;
  HIP_TRY(ctx, hipEventSynchronize(ctx->ev_dl));
  return CURVIS_OK;
}
int ensure_copy_stream(curvis_ctx *ctx) {
  if (int rc = ctx->copy_stream.ensure(ctx, hipStreamNonBlocking)) return rc;
  if (int rc = ctx->ev_fb.ensure(ctx, hipEventDisableTiming)) return rc;
  if (int rc = ctx->ev_dl.ensure(ctx, hipEventDisableTiming)) return rc;
  return ctx->ev_streams.ensure(ctx, hipEventDisableTiming);
}
/* call before anything writes `bytes` of frames into ctx->d_fb */
int fb_begin_write(curvis_ctx *ctx, size_t bytes) {
  if (ctx->dl_pending && ctx->dl_src == ctx->d_fb.p) /* the copy engine is still reading it: write the other one */
    std::swap(ctx->d_fb, ctx->d_fb_alt);
  return ctx->d_fb.reserve(ctx, bytes);
}
/* frames [0, bytes) of ctx->d_fb -> rgb_out, after everything queued on ctx->stream so far.  Synchronous unless the
 * option is set; either way ctx->stream is idle on return. */
int fb_download(curvis_ctx *ctx, unsigned char *rgb_out, size_t bytes) {
  if (!ctx->async_download) {
    HIP_TRY(ctx, hipMemcpyAsync(rgb_out, ctx->d_fb, bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return CURVIS_OK;
  }
  {
    const int rcs = ensure_copy_stream(ctx);
    if (rcs) return rcs;
  }
  const int rc = download_wait(ctx); /* the previous call's: it had this call's kernels to hide under */
  if (rc) return rc;
  HIP_TRY(ctx, hipEventRecord(ctx->ev_fb, ctx->stream));
  HIP_TRY(ctx, hipStreamWaitEvent(ctx->copy_stream, ctx->ev_fb, 0));
  HIP_TRY(ctx, hipMemcpyAsync(rgb_out, ctx->d_fb, bytes, hipMemcpyDeviceToHost, ctx->copy_stream));
  /* from here on a copy into the caller's buffer is in flight: it is tracked BEFORE anything else can fail, and a failure of
   * one of the remaining calls drains the copy stream before it is reported -- no error return with rgb_out still being written */
  ctx->dl_pending = true;
  ctx->dl_src = ctx->d_fb;
  ctx->downloads_overlapped++;
  hipError_t e = hipEventRecord(ctx->ev_dl, ctx->copy_stream);
  if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream); /* kernels, counters, debug dump: done (the frames are still on their way) */
  if (e != hipSuccess) {
    (void)hipStreamSynchronize(ctx->copy_stream);
    ctx->dl_pending = false;
    ctx->dl_src = nullptr;
    return fail(ctx, CURVIS_E_HIP, std::string("asynchronous frame download: ") + hipGetErrorString(e));
  }
  return CURVIS_OK;
}

/* counter block for a launch of n_frames frames: device block + pinned mirror, zeroed on the stream */
int prepare_counters(curvis_ctx *ctx, unsigned n_frames, FrameCounters &C, unsigned slots = 0u) {
  C.slots = slots ? slots : counter_slots_for(n_frames); /* a power of two */
  const size_t words = counter_words(n_frames, C.slots);
  if (int rc = ctx->d_counters.reserve(ctx, words)) return rc;
  if (int rc = ctx->h_counters.reserve(ctx, words + 8)) return rc;
  C.base = ctx->d_counters;
  HIP_TRY(ctx, hipMemsetAsync(ctx->d_counters, 0, sizeof(unsigned long long) * words, ctx->stream));
  return CURVIS_OK;
}
/* sum the replicas of frame f of the mirrored block into out[FC_N] */
void sum_frame_counters(const unsigned long long *h, unsigned slots, unsigned f, uint64_t out[FC_N]) {
  for (int k = 0; k < FC_N; ++k) out[k] = 0;
  for (unsigned r = 0; r < slots; ++r) {
    const unsigned long long *line = h + (size_t)CNT_STRIDE * (1u + (size_t)f * slots + r);
    for (int k = 0; k < FC_N; ++k) out[k] += line[k];
  }
}
/* the count fields of a statistics record from one summed counter line */
void counts_to_stats(const uint64_t fc[FC_N], curvis_stats &s) {
  s.rays = fc[FC_RAYS];
  s.steps = fc[FC_STEPS];
  s.n_pos = fc[FC_POS];
  s.n_neg = fc[FC_NEG];
  s.n_none = fc[FC_NONE];
  s.n_oob = fc[FC_OOB];
}

cvk::MetricParams make_metric(const curvis_metric &m) {
  cvk::MetricParams M;
  M.rho = m.rho;
  M.rho2 = m.rho * m.rho;
  M.m = m.m;
  M.a = m.a;
  M.pim = CV_PI * m.m;
  M.inv_pim = 1.0 / M.pim;
  M.two_o_pi = 2.0 / CV_PI;
  if (m.kind == CURVIS_METRIC_SCHWARZSCHILD) { /* the kind's own constants in the same slots (cv_device.h MetricParams) */
    M.pim = 2.0 * m.m;
    M.inv_pim = 1.0 / M.pim;
  }
  M.T = cv_sc_table(); /* host tables; kernels substitute their own copies (LDS or __constant__) */
  M.LT = cv_log_table();
  M.AT = cv_atan_table();
  return M;
}

/* one Euler step on the host, all eight components: the body of trajectory_kernel's loop */
template <int KIND>
void host_euler_step(const cvk::MetricParams &MP, double x[4], double p[4], double delta) {
  cvk::Ray q;
  q.l = x[1];
  q.th = x[2];
  q.ph = x[3];
  q.p1 = p[1];
  q.p2 = p[2];
  q.p3 = p[3];
  q.p3sq = q.p3 * q.p3;
  cvk::ray_step<KIND, true>(MP, q, delta);
  x[0] = x[0] + (p[0] * (1.0 / -1.0)) * delta; /* dx0 = p0 * g00.powi(-1), as in trajectory_kernel */
  x[1] = q.l;
  x[2] = q.th;
  x[3] = q.ph;
  p[0] = p[0] + 0.0 * delta;
  p[1] = q.p1;
  p[2] = q.p2;
  p[3] = p[3] + 0.0 * delta;
}

cvk::CameraParams make_camera(const curvis_camera &c) {
  cvk::CameraParams C;
  for (int i = 0; i < 4; ++i) C.pos[i] = c.pos[i];
  for (int i = 0; i < 9; ++i) C.rot[i] = c.rot[i];
  C.focal = c.focal;
  C.sensor_w = c.sensor_w;
  C.sensor_h = c.sensor_h;
  C.res_x = (double)c.res_x;
  C.res_y = (double)c.res_y;
  return C;
}

void stage_cameras(unsigned char *dst, const curvis_camera *cams, uint32_t n, const cvk::CameraBoost *boost) {
  for (uint32_t f = 0; f < n; ++f) {
    const cvk::CameraParams C = make_camera(cams[f]);
    std::memcpy(dst + sizeof C * f, &C, sizeof C);
  }
  if (boost) std::memcpy(dst + sizeof(cvk::CameraParams) * n, boost, sizeof(cvk::CameraBoost) * n);
}

cvk::SkyParams make_sky_params(const curvis_ctx *ctx, int k) {
  cvk::SkyParams S;
  S.texels = (const unsigned *)ctx->sky[k].texels;
  S.w = ctx->sky[k].w;
  S.h = ctx->sky[k].h;
  for (int i = 0; i < 9; ++i) S.inv_rot[i] = ctx->sky_inv_rot[k][i];
  return S;
}

/* ---- option "sky_mipmap": the mip chain of a sky.  Level k + 1 has (w_k + 1) >> 1 x (h_k + 1) >> 1 texels, down to 1 x 1; levels >= 1
 * share one allocation (a third of the sky), level 0 is the sky's own texels -- the caller's buffer for a borrowed sky.  One launch of
 * sky_mip_kernel per level on the context's stream; the table of {pointer, w, h} per level is what the FILTER = 2 kernels index. */
int build_sky_mips(curvis_ctx *ctx, const unsigned *level0, unsigned w, unsigned h, DeviceBuffer<unsigned> &texels,
                   DeviceBuffer<cvk::SkyMipLevel> &table, std::vector<cvk::SkyMipLevel> &host, unsigned &levels) {
  const unsigned L = cvk::sky_mip_levels(w, h);
  size_t total = 0;
  {
    unsigned wk = w, hk = h;
    for (unsigned k = 1; k < L; ++k) {
      wk = (wk + 1u) >> 1, hk = (hk + 1u) >> 1;
      total += (size_t)wk * hk;
    }
  }
  if (int rc = texels.reserve(ctx, total ? total : 1)) return rc;
  if (int rc = table.reserve(ctx, L)) return rc;
  host.assign(L, cvk::SkyMipLevel{level0, w, h});
  if (int rc = ctx->ev0.ensure(ctx)) return rc;
  if (int rc = ctx->ev1.ensure(ctx)) return rc;
  HIP_TRY(ctx, hipEventRecord(ctx->ev0, ctx->stream)); /* the launches alone, by HIP events: option "last_sky_mip_build_us" */
  size_t off = 0;
  for (unsigned k = 1; k < L; ++k) {
    const cvk::SkyMipLevel &s = host[k - 1];
    cvk::SkyMipLevel &d = host[k];
    d.w = (s.w + 1u) >> 1, d.h = (s.h + 1u) >> 1;
    d.texels = texels.p + off;
    off += (size_t)d.w * d.h;
    const dim3 grid((d.w + 255u) / 256u, d.h < 65535u ? d.h : 65535u);
    hipLaunchKernelGGL(sky_mip_kernel, grid, dim3(256), 0, ctx->stream, s.texels, s.w, s.h, const_cast<unsigned *>(d.texels), d.w, d.h);
    HIP_TRY(ctx, hipGetLastError());
  }
  HIP_TRY(ctx, hipEventRecord(ctx->ev1, ctx->stream));
  HIP_TRY(ctx, hipMemcpyAsync(table, host.data(), sizeof(cvk::SkyMipLevel) * L, hipMemcpyHostToDevice, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream)); /* `host` is pageable memory: the copy has left it */
  float build_ms = 0.f;
  HIP_TRY(ctx, hipEventElapsedTime(&build_ms, ctx->ev0, ctx->ev1));
  ctx->last_sky_mip_build_us = (int64_t)(build_ms * 1000.0f + 0.5f);
  levels = L;
  return CURVIS_OK;
}
/* the chains of both skies, built on first use (a render call with the option on, curvis_ctx_sky_mip_level) */
int ensure_sky_mips(curvis_ctx *ctx, int which) {
  SkyTexture &S = ctx->sky[which];
  if (!S.texels) return fail(ctx, CURVIS_E_NO_SKY, "sky not set");
  if (S.mip_levels) return CURVIS_OK;
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  const int rc = build_sky_mips(ctx, (const unsigned *)S.texels, S.w, S.h, S.mip_texels, S.mip_table, S.mip_host, S.mip_levels);
  if (rc) S.drop_mips();
  return rc;
}
SkyMipArgs sky_mip_args(const curvis_ctx *ctx) {
  SkyMipArgs A;
  for (int k = 0; k < 2; ++k) A.tab[k] = ctx->sky[k].mip_table.p, A.levels[k] = ctx->sky[k].mip_levels;
  return A;
}

/* workgroup size of the static and relay kernels ("block_threads"; total_rays is a multiple of 64) */
unsigned integrate_block_threads(const curvis_ctx *ctx) {
  const int bt = ctx->block_threads;
  return (bt == 64 || bt == 128 || bt == 256) ? (unsigned)bt : 256u;
}

/* grid = fresh workgroups + relay workgroups; see geodesic_relay */
template <int KIND, bool FAST, int SS, int FILTER, int PROJ>
int launch_relay(curvis_ctx *ctx, const IntegrateParams &P, bool relay_only) {
  static_assert(KIND != cvk::METRIC_SCHWARZSCHILD, "no relay kernel of the Schwarzschild kind: relay_resident_blocks has three kinds");
  void (*const kernel)(const IntegrateParams, const RelayArgs) = geodesic_relay<KIND, FAST, SS, FILTER, PROJ>;
  const size_t bytes = sizeof(RelayQueue) + sizeof(unsigned) * kRelayRing;
  if (int rc = ctx->d_rq.reserve(ctx, bytes)) return rc;
  RelayArgs A;
  A.q = (RelayQueue *)ctx->d_rq.p;
  A.n_tiles = P.total_rays / 64ull;
  const unsigned bt = integrate_block_threads(ctx);
  const unsigned long long fresh_blocks = relay_only ? 0ull : (P.total_rays + bt - 1ull) / bt;
  A.fresh_blocks = (unsigned)fresh_blocks;
  /* segment = 0.6 R / delta steps: an ordinary ray (about R / delta steps from a camera near the throat, +-10 %)
   * then crosses ONE hand-over point and ends well inside its second segment.  With 0.5 R / delta the second
   * boundary falls inside the spread of ray lengths and a third of the tiles is handed over a second time for their
   * last few dozen steps (1080p: 10.8 ms against 10.6 with 0.4 or 0.6; tools/gpu_seg_sweep.py); segments below
   * ~0.3 R / delta cost more in boundary checks and workgroup launches than the finer balance returns. */
  {
    const double half = 0.6 * P.max_radius / P.delta;
    unsigned seg = (half >= 256.0 && half <= 65536.0) ? (unsigned)half : 1024u;
    A.seg = ctx->relay_segment > 0 ? (unsigned)ctx->relay_segment : seg;
  }
  A.max_hops = (unsigned)std::max(0, ctx->relay_max_hops);
  A.max_parks = (unsigned)std::max(0, ctx->relay_max_parks);
  A.corrupt_ticket = ctx->relay_test_corrupt ? 1u : 0u;
  ctx->relay_test_corrupt = 0;
  if (ctx->relay_resident_threads != (int)bt) {
    std::memset(ctx->relay_resident_blocks, 0, sizeof ctx->relay_resident_blocks);
    ctx->relay_resident_threads = (int)bt;
  }
  unsigned &cached = ctx->relay_resident_blocks[PROJ][FILTER][supersample_log2(SS)][KIND][FAST ? 1 : 0];
  if (cached == 0) {
    int per_cu = 0;
    HIP_TRY(ctx, hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, (int)bt, 0));
    if (per_cu <= 0) per_cu = 1;
    cached = (unsigned)per_cu * (unsigned)ctx->prop.multiProcessorCount;
  }
  const unsigned long long resident_blocks = cached;
  if (!relay_only) HIP_TRY(ctx, hipMemsetAsync(ctx->d_rq, 0, bytes, ctx->stream));
  /* every tile in flight when the fresh workgroups run out (at most the resident waves) is passed on once per
   * segment of its remaining steps: (max_iter / seg) <= 16 hand-overs each, usually ~2; surplus relay
   * workgroups leave at once */
  unsigned long long relay_blocks = resident_blocks * 24ull;
  if (relay_blocks > fresh_blocks * 2ull + resident_blocks) relay_blocks = fresh_blocks * 2ull + resident_blocks;
  hipLaunchKernelGGL(kernel, dim3((unsigned)(fresh_blocks + relay_blocks)), dim3(bt), 0, ctx->stream, P, A);
  HIP_TRY(ctx, hipGetLastError());
  return CURVIS_OK;
}

int launch_shade(curvis_ctx *ctx, int kind, bool debug, const ShadeParams &P) {
  const unsigned long long blocks = (P.n_pixels + 255ull) / 256ull;
  with_kind(kind, [&](auto K) {
    with_flag(debug, [&](auto D) {
      hipLaunchKernelGGL((shade_kernel<decltype(K)::value, decltype(D)::value>), dim3((unsigned)blocks), dim3(256), 0, ctx->stream, P);
    });
  });
  HIP_TRY(ctx, hipGetLastError());
  return CURVIS_OK;
}

RayStore carve_store(unsigned char *base, size_t npix) {
  RayStore S;
  double *d = (double *)base;
  S.l = d;
  S.th = d + npix;
  S.ph = d + 2 * npix;
  S.p1 = d + 3 * npix;
  S.p2 = d + 4 * npix;
  S.p3 = d + 5 * npix;
  S.steps = (unsigned *)(d + 6 * npix);
  S.code = (int *)(S.steps + npix);
  return S;
}
constexpr size_t kStoreBytesPerPixel = 6 * sizeof(double) + sizeof(unsigned) + sizeof(int);

/* ---- render_impl and its pieces ------------------------------------------------------------------------------------------ */

/* one call: its arguments, and the sizes the argument checks derive from them */
struct BruteCall {
  const curvis_metric *metric;
  const curvis_camera *cams;
  uint32_t n_frames, max_iter;
  double max_radius, delta;
  uint8_t *rgb_out;
  curvis_ray_debug *dbg_out;
  curvis_stats *stats;
  uint32_t row_begin, row_count; /* row band (curvis_render_brute_rows); row_count = 0: the whole frame */
  uint32_t ss;                   /* supersampling factor.  With ss > 1 the cameras, the band, W and H are those of the ss times finer
                                    RAY grid (what the kernels run over); npix and fb_bytes are always those of the frames written */
  uint32_t filter;               /* option "sky_filter" for this call */
  uint32_t projection;           /* option "projection" for this call (CallShape: with PROJ_BOOSTED while a frame moves) */
  const cvk::CameraBoost *boost = nullptr; /* ... and then the frames' boosts, n_frames of them */
  double kappa = 0.0;            /* option "step_scale" for this call: RN(delta / L0) ... */
  int adapt = 0;                 /* ... and the kernels' ADAPT (CallShape) */
  brute::Facts facts;            /* what the plan reads (brute_plan.h), but for relay_size_ok: choose_render_path's */
  uint32_t W = 0, H = 0;         /* H: the rows this call renders */
  size_t npix = 0, fb_bytes = 0;
};
static_assert(brute::KIND_SCHWARZSCHILD == CURVIS_METRIC_SCHWARZSCHILD && brute::KIND_SCHWARZSCHILD == cvk::METRIC_SCHWARZSCHILD, "brute_plan.h spells the kind out");
/* the facts of a call as the context's options, its disc and the call's arguments give them; `moving` is known after prepare_camera_boost.
 * Without a metric the disc's motion refuses nothing: the call is on its way to the null-argument refusal. */
brute::Facts brute_facts(const curvis_ctx *ctx, const curvis_metric *metric, bool dump) {
  brute::Facts f;
  f.dump = dump;
  f.variant = ctx->variant;
  f.fuse_shade = ctx->fuse_shade != 0;
  f.fast_math = ctx->fast_math != 0;
  f.supersample = ctx->supersample > 1;
  f.sky_filter = ctx->sky_filter != 0;
  f.sky_mipmap = ctx->sky_mipmap != 0;
  f.projection = ctx->projection != 0;
  f.step_scale = ctx->step_scale != 0;
  f.integrator = ctx->integrator != 0;
  f.disc = !ctx->disc_set ? brute::DISC_NONE : ctx->disc_motion != 0 && metric ? brute::DISC_MOVING : brute::DISC_STATIC;
  f.kind = metric ? metric->kind : CURVIS_METRIC_FLAT;
  return f;
}
/* the plan's refusal, at the point of the call where it is due (brute::At) */
int plan_refusal(curvis_ctx *ctx, const brute::Facts &facts, brute::At now) {
  const brute::Plan plan = brute::plan(facts);
  return plan.refusal && plan.at <= now ? fail(ctx, CURVIS_E_INVALID, plan.refusal) : CURVIS_OK;
}
int render_rays(curvis_ctx *ctx, BruteCall c);
/* the same frames once more (the relay kernel's fall-backs and its checker): with the caller's outputs, or into d_fb only; the
 * checker asks for the static kernel */
int render_again(curvis_ctx *ctx, BruteCall c, bool deliver, bool static_only = false) {
  if (!deliver) c.rgb_out = nullptr, c.dbg_out = nullptr, c.stats = nullptr;
  if (static_only) c.facts.variant = brute::STATIC_ONLY;
  return render_rays(ctx, c);
}
/* a piece's answer when the relay kernel has just been switched off for this context (waves that gave up, a checked launch that
 * differs): render_impl renders the call again -- the static kernel takes it */
constexpr int kRenderAgain = 1;

/* which kernels render the call, and how many frames at a time */
struct RenderPath {
  bool fused, relay;    /* the plan's (brute_plan.h) */
  brute::Family family; /* of the kernel that integrates */
  uint32_t chunk;       /* frames per launch */
  size_t store_bytes;   /* of the ray store: the relay kernel's staging area, or the unfused path's final states; 0 = none */
};
RenderPath choose_render_path(const curvis_ctx *ctx, const BruteCall &c) {
  /* Fused shading (static kernel, no debug dump; option "fuse_shade", default on) has no ray store at all.  Otherwise frames are
   * rendered in chunks whose ray store stays below max_store_bytes.  Which calls are fused, and which options keep a call from the
   * relay kernel whatever its size: brute_plan.h (plan, kNoRelay).  Here are its size conditions.
   * Relay kernel ("variant" = 2, and the automatic choice for big enough single images): end-game hand-over of
   * tiles; only launches of a few frames have a tail worth its staging area (56 B per ray) -- larger batches
   * use the static kernel, and so do frames too small to have a dispatch phase (measured against the static
   * kernel: 640x360 +2 %, 720x405 -9 %, 800x450 -9 %, 960x540 -15 %, 1280x720 -6 %, 1920x1080 -3..-5 %,
   * 2560x1440 -1 %; tools/gpu_relay_sizes.py, tools/gpu_relay_threshold.py) */
  const unsigned long long tiles = (unsigned long long)((c.W + 7) / 8) * ((c.H + 7) / 8) * c.n_frames;
  const unsigned long long relay_fresh_blocks = (tiles + 3ull) / 4ull;
  const unsigned long long relay_min = ctx->relay_min_blocks >= 0 ? (unsigned long long)ctx->relay_min_blocks
                                                                   : 4ull * (unsigned long long)ctx->prop.multiProcessorCount;
  const size_t relay_staging = (size_t)tiles * 64u * kStoreBytesPerPixel;
  brute::Facts facts = c.facts;
  facts.relay_size_ok = !ctx->relay_disabled && c.n_frames <= (uint32_t)ctx->relay_max_frames && relay_fresh_blocks >= relay_min && relay_staging <= ctx->max_store_bytes;
  const brute::Plan plan = brute::plan(facts);
  RenderPath p;
  p.fused = plan.fused;
  p.relay = plan.relay;
  p.family = plan.family;
  p.chunk = c.n_frames;
  p.store_bytes = p.relay ? relay_staging : 0;
  if (!p.fused) {
    p.chunk = (uint32_t)std::max<size_t>(1, ctx->max_store_bytes / (c.npix * kStoreBytesPerPixel));
    if (p.chunk > c.n_frames) p.chunk = c.n_frames;
    p.store_bytes = (size_t)p.chunk * c.npix * kStoreBytesPerPixel;
  }
  return p;
}

struct RenderTotals { /* over the chunks of a call */
  uint64_t counts[FC_N] = {0};
  double integrate_ms = 0.0, shade_ms = 0.0;
};

template <typename Arg>
int launch_kernel(curvis_ctx *ctx, void (*kernel)(Arg), dim3 grid, dim3 block, const Arg &arg) {
  hipLaunchKernelGGL(kernel, grid, block, 0, ctx->stream, arg);
  HIP_TRY(ctx, hipGetLastError());
  return CURVIS_OK;
}
/* the argument of a static kernel: the plain form's (PA, cut down to IntegrateParams where ADAPT = 0) with what FILTER = 2 and the
 * DISC forms append */
template <int ADAPT, int FILTER, int DISC = 0>
IntegrateArgsD<ADAPT, FILTER, DISC> integrate_args(const curvis_ctx *ctx, const IntegrateParamsAdapt &PA) {
  IntegrateArgsD<ADAPT, FILTER, DISC> A;
  static_cast<IntegrateArgs<ADAPT> &>(A) = PA;
  if constexpr (FILTER == 2) A.mip = sky_mip_args(ctx); /* option "sky_mipmap": the level tables */
  if constexpr (DISC != 0) {
    A.disc.texels = ctx->d_disc;
    A.disc.w = ctx->disc_w;
    A.disc.h = ctx->disc_h;
    A.disc.l_in = ctx->disc_l_in;
    A.disc.l_out = ctx->disc_l_out;
  }
  if constexpr (DISC == 2) { /* the disc has a motion: sigma, G and the camera factors of the launch's frames (render_rays filled them) */
    A.motion.sigma = (double)ctx->disc_motion;
    A.motion.gain = ctx->disc_gain;
    const cvk::CameraParams *cams0 = ctx->d_cams;
    A.motion.cam_factor = ctx->d_disc_cam + (PA.cams - cams0); /* the chunk's first frame, as PA.cams is */
  }
  return A;
}

/* One launch of the integrator: the kernel of the plan's family, in the call's launch shape.  Each family is instantiated for the
 * shapes brute::family_exists names and for no other (the kernels' own static_asserts admit no more); the plan names no family that is
 * absent for the call's shape (tests/test_brute_plan_host.py walks every call), so the refusal at the end is not reached.  phi is
 * integrated for the debug dump and by the DISC kernels.  relay_only: the relay kernel's re-launch. */
int launch_integrate(curvis_ctx *ctx, const BruteCall &c, brute::Family family, const IntegrateParamsAdapt &PA, bool relay_only = false) {
  const unsigned bt = integrate_block_threads(ctx);
  const dim3 grid((unsigned)((PA.total_rays + bt - 1ull) / bt)), block(bt);
  return with_launch_shape(c.metric->kind, ctx->fast_math != 0, c.ss, c.filter, c.projection, c.adapt, [&](auto S) -> int {
    using T = decltype(S);
    using brute::Family;
    constexpr int KIND = T::KIND, SS = T::SS, FILTER = T::FILTER, PROJ = T::PROJ, ADAPT = T::ADAPT;
    constexpr bool FAST = T::FAST;
    switch (family) {
      case Family::Persistent:
        if constexpr (brute::family_exists<T>(Family::Persistent))
          return with_flag(c.dbg_out != nullptr, [&](auto PHI) -> int {
            void (*const kernel)(const IntegrateParams) = geodesic_persistent<KIND, decltype(PHI)::value, FAST>;
            int per_cu = ctx->blocks_per_cu;
            if (per_cu <= 0) {
              HIP_TRY(ctx, hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, 256, 0));
              if (per_cu <= 0) per_cu = 1;
            }
            unsigned long long blocks = (unsigned long long)per_cu * (unsigned long long)ctx->prop.multiProcessorCount;
            const unsigned long long max_useful = (PA.total_rays + 255ull) / 256ull;
            if (blocks > max_useful) blocks = max_useful;
            if (blocks == 0) blocks = 1;
            return launch_kernel(ctx, kernel, dim3((unsigned)blocks), dim3(256), integrate_args<0, 0>(ctx, PA));
          });
        break;
      case Family::Unfused:
        if constexpr (brute::family_exists<T>(Family::Unfused))
          return with_flag(c.dbg_out != nullptr, [&](auto PHI) -> int {
            return launch_kernel(ctx, geodesic_static<KIND, decltype(PHI)::value, FAST, false>, grid, block, integrate_args<0, 0>(ctx, PA));
          });
        break;
      case Family::StagedAdapt:
        if constexpr (brute::family_exists<T>(Family::StagedAdapt))
          return launch_kernel(ctx, geodesic_static<KIND, true, FAST, false, 1, 0, 0, ADAPT>, grid, block, integrate_args<ADAPT, 0>(ctx, PA));
        break;
      case Family::Fused:
        if constexpr (brute::family_exists<T>(Family::Fused))
          return launch_kernel(ctx, geodesic_static<KIND, false, FAST, true, SS, FILTER, PROJ, ADAPT>, grid, block, integrate_args<ADAPT, FILTER>(ctx, PA));
        break;
      case Family::Relay: /* a grid of its own */
        if constexpr (brute::family_exists<T>(Family::Relay)) return launch_relay<KIND, FAST, SS, FILTER, PROJ>(ctx, PA, relay_only);
        break;
      case Family::Disc:
        if constexpr (brute::family_exists<T>(Family::Disc))
          return launch_kernel(ctx, geodesic_static<KIND, true, FAST, true, SS, FILTER, PROJ, ADAPT, 1>, grid, block, integrate_args<ADAPT, FILTER, 1>(ctx, PA));
        break;
      case Family::DiscMotion:
        if constexpr (brute::family_exists<T>(Family::DiscMotion))
          return launch_kernel(ctx, geodesic_static<KIND, true, FAST, true, SS, FILTER, PROJ, ADAPT, 2>, grid, block, integrate_args<ADAPT, FILTER, 2>(ctx, PA));
        break;
    }
    return fail(ctx, CURVIS_E_INVALID, "no kernel of the plan's family exists for this call's launch shape");
  });
}

/* frames [f0, f0 + nf) of the call: parameters, the launch(es), the relay kernel's re-launch loop, counters -> statistics */
int render_chunk(curvis_ctx *ctx, const BruteCall &c, const RenderPath &path, const cvk::MetricParams &MP, uint32_t f0, uint32_t nf,
                 RenderTotals &tot) {
  const bool relay = path.relay, fused = path.fused;
  FrameCounters FC;
  int rc = prepare_counters(ctx, nf, FC);
  if (rc) return rc;
  const size_t cnt_words = counter_words(nf, FC.slots);
  IntegrateParamsAdapt P;
  P.metric = MP;
  P.cams = ctx->d_cams + f0;
  P.n_frames = nf;
  P.W = c.W;
  P.H = c.H;
  P.row0 = c.row_count ? c.row_begin : 0u;
  P.tiles_x = (c.W + 7) / 8;
  P.tiles_y = (c.H + 7) / 8;
  const unsigned long long rpf = (unsigned long long)P.tiles_x * P.tiles_y * 64ull;
  if (rpf > 0xFFFFFFFFull || rpf * nf / 64ull > 0xFFFFFFFFull) return fail(ctx, CURVIS_E_INVALID, "frame or batch too large");
  P.rays_per_frame = (unsigned)rpf;
  P.total_rays = rpf * nf;
  P.max_iter = c.max_iter;
  P.max_radius = c.max_radius;
  P.delta = c.delta;
  P.store = relay ? carve_store(ctx->d_store, (size_t)P.total_rays) : fused ? RayStore{} : carve_store(ctx->d_store, (size_t)nf * c.npix);
  P.counters = FC;
  for (int k = 0; k < 2; ++k) P.sky[k] = make_sky_params(ctx, k);
  P.fb = ctx->d_fb + (size_t)f0 * c.npix * 3;
  P.refill_threshold = ctx->refill_threshold < 1 ? 1 : (ctx->refill_threshold > 64 ? 64 : ctx->refill_threshold);
  P.fast_ok = cvk::metric_fast_ok(c.metric->kind, MP, c.max_radius) ? 1 : 0;
  P.projection = (int)c.projection;
  if (c.boost && (f0 != 0 || nf != c.n_frames)) return fail(ctx, CURVIS_E_INVALID, "camera velocity: the frames' boosts lie behind the cameras of the whole call, which one fused launch renders");
  P.kappa = c.kappa;
  P.t_out = (c.adapt && c.dbg_out) ? ctx->d_dbg_t + (size_t)f0 * c.npix : nullptr;
  /* diagnostics only (CURVIS_TRACE_FILE): per-wave records of this launch, binary u64 x 4 per wave */
  DeviceBuffer<unsigned long long> trace;
  const char *trace_file = getenv("CURVIS_TRACE_FILE");
  size_t trace_words = (size_t)(P.total_rays / 64ull) * 4u;
  if (relay) trace_words = (size_t)(P.total_rays / 64ull) * 3u * 4u + 65536u * 16u; /* every wave of the grid */
  if (trace_file && *trace_file && path.family != brute::Family::Persistent) {
    if ((rc = trace.reserve(ctx, trace_words))) return rc;
    HIP_TRY(ctx, hipMemsetAsync(trace, 0, trace_words * sizeof(unsigned long long), ctx->stream));
  }
  P.trace = trace;

  ShadeParams Q;
  Q.metric = MP;
  for (int k = 0; k < 2; ++k) Q.sky[k] = P.sky[k];
  Q.store = P.store;
  Q.n_pixels = (unsigned long long)nf * c.npix;
  Q.fb = P.fb;
  Q.dbg = c.dbg_out ? ctx->d_dbg + (size_t)f0 * c.npix : nullptr;
  Q.npix = c.npix;
  Q.counters = FC;

  HIP_TRY(ctx, hipEventRecord(ctx->ev0, ctx->stream));
  rc = launch_integrate(ctx, c, path.family, P);
  if (rc) return rc;
  HIP_TRY(ctx, hipEventRecord(ctx->ev1, ctx->stream));
  if (trace) {
    std::vector<unsigned long long> tr(trace_words);
    HIP_TRY(ctx, hipMemcpyAsync(tr.data(), trace, trace_words * sizeof(unsigned long long), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (FILE *fp = fopen(trace_file, "wb")) {
      fwrite(tr.data(), sizeof(unsigned long long), tr.size(), fp);
      fclose(fp);
    }
  }
  if (!fused) {
    rc = launch_shade(ctx, c.metric->kind, c.dbg_out != nullptr, Q);
    if (rc) return rc;
  }
  HIP_TRY(ctx, hipEventRecord(ctx->ev2, ctx->stream));
  ctx->last_relay_launches = relay ? 1 : 0;
  for (;;) {
    HIP_TRY(ctx, hipMemcpyAsync(ctx->h_counters, ctx->d_counters, sizeof(unsigned long long) * cnt_words, hipMemcpyDeviceToHost,
                                ctx->stream));
    if (relay) /* queue header rides along with the counters: finished / error */
      HIP_TRY(ctx, hipMemcpyAsync(ctx->h_counters + cnt_words, ctx->d_rq, sizeof(unsigned long long) * 8, hipMemcpyDeviceToHost,
                                  ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (!relay) break;
    /* normally the one launch finished every tile; more relay workgroups only if the grid ran out of them
     * with tiles still parked */
    const RelayQueue *hq = (const RelayQueue *)(ctx->h_counters + cnt_words);
    const unsigned long long n_tiles = P.total_rays / 64ull;
    if (hq->error != 0 || ctx->relay_test_fault) {
      /* waves gave up waiting for a tile (a logic error, or a dispatcher that did not start the workgroups in
       * order): not a hang and not a wrong frame -- the frame is rendered again by the static kernel, which has no
       * inter-workgroup dependency, and this context stops using the relay kernel */
      ctx->relay_test_fault = 0;
      ctx->relay_disabled = 1;
      ctx->relay_fallbacks++;
      fprintf(stderr, "[curvis] relay kernel: %llu waves gave up waiting (%llu tiles unfinished); falling back to the static kernel for this context\n",
              (unsigned long long)hq->error, (unsigned long long)(n_tiles - hq->finished));
      return kRenderAgain;
    }
    ctx->last_relay_parks = hq->tail;
    ctx->last_relay_waiters = hq->head;
    if (hq->finished >= n_tiles) break;
    if (ctx->last_relay_launches++ > 64)
      return fail(ctx, CURVIS_E_HIP, "relay kernel: tiles still unfinished after 64 relay launches");
    rc = launch_integrate(ctx, c, path.family, P, true);
    if (rc) return rc;
    HIP_TRY(ctx, hipEventRecord(ctx->ev1, ctx->stream));
    HIP_TRY(ctx, hipEventRecord(ctx->ev2, ctx->stream));
  }
  float ms_i = 0.f, ms_s = 0.f;
  HIP_TRY(ctx, hipEventElapsedTime(&ms_i, ctx->ev0, ctx->ev1));
  tot.integrate_ms += ms_i;
  HIP_TRY(ctx, hipEventElapsedTime(&ms_s, ctx->ev1, ctx->ev2));
  tot.shade_ms += ms_s;
  uint64_t launch_steps = 0;
  for (uint32_t f = 0; f < nf; ++f) {
    uint64_t fc[FC_N];
    sum_frame_counters(ctx->h_counters, FC.slots, f, fc);
    for (int k = 0; k < FC_N; ++k) tot.counts[k] += fc[k];
    counts_to_stats(fc, ctx->last_frame_stats[f0 + f]);
    ctx->last_frame_disc[f0 + f] = fc[FC_DISC];
    launch_steps += fc[FC_STEPS];
  }
  /* the frames of a launch run interleaved on the GPU: times are the launch's, shared out by executed Euler steps */
  for (uint32_t f = 0; f < nf; ++f) {
    curvis_stats &fs = ctx->last_frame_stats[f0 + f];
    const double share = launch_steps ? (double)fs.steps / (double)launch_steps : 1.0 / nf;
    fs.integrate_ms = ms_i * share;
    fs.shade_ms = ms_s * share;
    fs.kernel_ms = fs.integrate_ms + fs.shade_ms;
    fs.total_ms = fs.kernel_ms;
  }
  return CURVIS_OK;
}

/* what a render leaves in the context for the statistics calls and options: the seat belt's re-render overwrites it, and the relay
 * launch's values are put back */
struct LastRenderStats {
  std::vector<curvis_stats> frames;
  uint32_t relay_launches;
  uint64_t relay_parks, relay_waiters;
  double integrate_ms, shade_ms;
  explicit LastRenderStats(const curvis_ctx *c)
      : frames(c->last_frame_stats), relay_launches(c->last_relay_launches), relay_parks(c->last_relay_parks),
        relay_waiters(c->last_relay_waiters), integrate_ms(c->last_integrate_ms), shade_ms(c->last_shade_ms) {}
  void restore(curvis_ctx *c) const {
    c->last_frame_stats = frames;
    c->last_relay_launches = relay_launches;
    c->last_relay_parks = relay_parks;
    c->last_relay_waiters = relay_waiters;
    c->last_integrate_ms = integrate_ms;
    c->last_shade_ms = shade_ms;
  }
};

/* The relay kernel's hand-over rests on gfx950 facts (write-through sc0 sc1 stores, s_waitcnt vmcnt(0) before
 * the ticket store) rather than on the HIP memory model, so it wears a seat belt: the first relay launch of every
 * launch shape is repeated by the static kernel -- no inter-workgroup traffic at all -- and frames and counters are
 * compared.  Option "relay_verify" = 1 checks EVERY launch and makes a difference an error (debugging); the automatic
 * check (option "relay_auto_verify", default 1) costs one static launch per shape and context and, on a difference,
 * reports it on stderr, counts it ("relay_mismatches"), switches the context to the static kernel and asks for the call to be
 * rendered again (kRenderAgain): the caller gets the static kernel's frame.  Called after a relay render, d_fb holding its frames. */
int relay_seat_belt(curvis_ctx *ctx, const BruteCall &c) {
  /* everything that shapes the hand-over pattern: size of the ray grid and frame count, metric, step flavour, supersampling
   * factor and sky filter (other epilogues), the projection (other rays), the band, the step cap, the segment length and hop limit in force */
  const std::array<uint32_t, 9> shape = {c.W, c.H, c.n_frames, (uint32_t)c.metric->kind,
                                         (uint32_t)(ctx->fast_math != 0 ? 1 : 0) | (c.ss << 8) | (c.filter << 16) | (c.projection << 24),
                                         c.row_begin, c.row_count, c.max_iter,
                                         (uint32_t)ctx->relay_segment * 256u + (uint32_t)std::max(0, ctx->relay_max_hops)};
  bool auto_check = false;
  if (!ctx->relay_verify && ctx->relay_auto_verify) {
    const uint64_t seen = ctx->relay_verified[shape]++; /* relay launches of this shape before this one */
    auto_check = seen == 0 || (ctx->relay_recheck_every > 0 && seen % (uint64_t)ctx->relay_recheck_every == 0);
  }
  if (!ctx->relay_verify && !auto_check) return CURVIS_OK;
  /* the relay frame is kept in a second device buffer and compared there: no host copies (two pageable D2H copies of a
   * batch cost more than the static re-render and left the NEXT render call 20 ms slower) */
  const size_t fb_bytes = c.fb_bytes, padded = (fb_bytes + 7) & ~(size_t)7;
  int rc = ctx->d_verify.reserve(ctx, padded + 8);
  if (rc) return rc;
  HIP_TRY(ctx, hipMemsetAsync(ctx->d_verify + (padded - 8), 0, 16, ctx->stream)); /* tail padding + the counter */
  HIP_TRY(ctx, hipMemcpyAsync(ctx->d_verify, ctx->d_fb, fb_bytes, hipMemcpyDeviceToDevice, ctx->stream));
  if (ctx->d_fb.cap < padded) { /* room for the zeroed tail the word-wise compare reads (the frame is re-rendered below anyway) */
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if ((rc = ctx->d_fb.reserve(ctx, padded))) return rc;
  }
  const LastRenderStats relay_run(ctx);
  rc = render_again(ctx, c, false, true); /* the static kernel */
  if (rc) return rc;
  /* d_fb holds the static kernel's frame now */
  if (padded != fb_bytes) HIP_TRY(ctx, hipMemsetAsync(ctx->d_fb + fb_bytes, 0, padded - fb_bytes, ctx->stream));
  unsigned long long *d_cnt = (unsigned long long *)(ctx->d_verify + padded);
  const size_t n_words = padded / 8;
  hipLaunchKernelGGL(compare_kernel, dim3((unsigned)std::min<size_t>((n_words + 255) / 256, 4096)), dim3(256), 0, ctx->stream,
                     (const unsigned long long *)ctx->d_verify.p, (const unsigned long long *)ctx->d_fb.p, n_words, d_cnt);
  HIP_TRY(ctx, hipGetLastError());
  unsigned long long n_diff_words = 0;
  HIP_TRY(ctx, hipMemcpyAsync(&n_diff_words, d_cnt, sizeof n_diff_words, hipMemcpyDeviceToHost, ctx->stream));
  HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  const std::vector<curvis_stats> &fs = relay_run.frames;
  bool same = n_diff_words == 0 && fs.size() == ctx->last_frame_stats.size();
  for (size_t f = 0; same && f < fs.size(); ++f) {
    const curvis_stats &x = fs[f], &y = ctx->last_frame_stats[f];
    same = x.rays == y.rays && x.steps == y.steps && x.n_pos == y.n_pos && x.n_neg == y.n_neg && x.n_none == y.n_none && x.n_oob == y.n_oob;
  }
  if (!same) {
    ctx->relay_mismatches++;
    if (ctx->relay_verify) return fail(ctx, CURVIS_E_HIP, "relay_verify: the relay kernel and the static kernel disagree on this launch");
    fprintf(stderr, "[curvis] relay kernel: a checked launch of shape %ux%u x %u frame(s) differs from the static kernel (%llu of %zu 8-byte words%s); "
                    "this context uses the static kernel from now on\n", c.W, c.H, c.n_frames, n_diff_words, n_words, n_diff_words ? "" : ", counters only");
    ctx->relay_disabled = 1;
    ctx->relay_fallbacks++;
    return kRenderAgain;
  }
  ctx->relay_checks++;
  /* the launch that counts is the relay one: its frame is what d_fb holds again (same bytes), and so are its statistics */
  relay_run.restore(ctx);
  return CURVIS_OK;
}

/* debug dump: x[0] of every ray.  Dead lanes of the integrator, replayed on the host: t_{k+1} = t_k + (p_t * g^tt) * delta with
 * p_t = 1, g^tt = -1 (src/metrics.rs:237, :295); p_t = p_t + 0*delta stays 1. */
void replay_debug_time(const BruteCall &c) {
  std::vector<double> t_of_steps;
  for (uint32_t f = 0; f < c.n_frames; ++f) {
    curvis_ray_debug *d = c.dbg_out + (size_t)f * c.npix;
    uint32_t most = 0; /* the table only needs to reach the largest step count of the frame, not the cap */
    for (size_t i = 0; i < c.npix; ++i) most = std::max(most, d[i].steps);
    t_of_steps.resize((size_t)most + 1);
    double t = c.cams[f].pos[0];
    t_of_steps[0] = t;
    for (uint32_t k = 1; k <= most; ++k) {
      t = t + (1.0 * -1.0) * c.delta;
      t_of_steps[k] = t;
    }
    for (size_t i = 0; i < c.npix; ++i) d[i].x[0] = t_of_steps[d[i].steps];
  }
}

/* the call's arguments as the caller of render_impl gave them, except that cameras, band and `ss` are in units of the ray grid; the
 * derived sizes (W ... fb_bytes) are worked out here */
int render_rays(curvis_ctx *ctx, BruteCall c) {
  if (!ctx) return CURVIS_E_INVALID;
  if (!c.metric || !c.cams || c.n_frames == 0) return fail(ctx, CURVIS_E_INVALID, "null metric/camera or zero frames");
  const auto t_begin = std::chrono::steady_clock::now();
  int rc = curvis_metric_validate(c.metric);
  if (rc != CURVIS_OK) return fail(ctx, rc, "invalid metric parameters (src/metrics.rs:409-456)");
  if ((rc = schwarzschild_camera_check(ctx, c.metric, c.cams, c.n_frames))) return rc;
  if ((rc = plan_refusal(ctx, c.facts, brute::AT_KIND))) return rc;
  const uint32_t H_full = c.cams[0].res_y;
  c.W = c.cams[0].res_x;
  if (c.W == 0 || H_full == 0) return fail(ctx, CURVIS_E_INVALID, "resolution must be greater than 0 (src/cameras.rs:98)");
  /* row band (curvis_render_brute_rows): the launch covers image rows [row_begin, row_begin + row_count); the
   * cameras keep the full resolution, which is what pixel -> direction uses */
  const bool band = c.row_count != 0;
  if (band && ((uint64_t)c.row_begin + c.row_count > H_full || c.n_frames != 1 || c.dbg_out))
    return fail(ctx, CURVIS_E_INVALID, "row band outside the frame (or used with a batch / the debug dump)");
  c.H = band ? c.row_count : H_full;
  for (uint32_t f = 0; f < c.n_frames; ++f) {
    if (c.cams[f].res_x != c.W || c.cams[f].res_y != H_full)
      return fail(ctx, CURVIS_E_INVALID, "all cameras of a batch must share one resolution");
    if (std::fabs(c.cams[f].pos[1]) > c.max_radius)
      return fail(ctx, CURVIS_E_CAMERA_OUTSIDE,
                  "Photon already beyond the maximum radius. Cannot evaluate escape. (src/systems.rs:122-124)");
  }
  if (!ctx->sky[0].texels || !ctx->sky[1].texels) return fail(ctx, CURVIS_E_NO_SKY, "both background images must be set");
  /* option "sky_mipmap": rays are paired in 2 x 2 quads of FRAME coordinates, whatever the split into bands: a band begins on an even
   * row of the ray grid and holds an even number of them unless it ends the frame */
  if (c.filter == 2u && band && ((c.row_begin & 1u) || ((c.row_count & 1u) && c.row_begin + c.row_count != H_full)))
    return fail(ctx, CURVIS_E_INVALID, "sky_mipmap = 1: a row band must begin on an even row and hold an even number of rows unless it ends the frame");
  HIP_TRY(ctx, hipSetDevice(ctx->device));
  if (c.filter == 2u)
    for (int k = 0; k < 2; ++k)
      if ((rc = ensure_sky_mips(ctx, k))) return rc;

  c.npix = (size_t)(c.W / c.ss) * (c.H / c.ss);
  c.fb_bytes = c.npix * 3 * c.n_frames;
  if ((rc = fb_begin_write(ctx, c.fb_bytes))) return rc;
  ctx->fb_bytes = c.fb_bytes;
  if (c.dbg_out && (rc = ctx->d_dbg.reserve(ctx, c.npix * c.n_frames))) return rc;
  if (c.dbg_out && c.adapt && (rc = ctx->d_dbg_t.reserve(ctx, c.npix * c.n_frames))) return rc;
  const RenderPath path = choose_render_path(ctx, c);
  if (path.store_bytes && (rc = ctx->d_store.reserve(ctx, path.store_bytes))) return rc;
  const size_t cams_bytes = staged_cameras_bytes(c.n_frames, c.boost);
  const size_t cams_slots = (cams_bytes + sizeof(cvk::CameraParams) - 1) / sizeof(cvk::CameraParams); /* with the boosts behind the cameras */
  if ((rc = ctx->d_cams.reserve(ctx, cams_slots))) return rc;
  if ((rc = ctx->h_cams.reserve(ctx, cams_slots))) return rc;
  stage_cameras(reinterpret_cast<unsigned char *>(ctx->h_cams.p), c.cams, c.n_frames, c.boost);
  HIP_TRY(ctx, hipMemcpyAsync(ctx->d_cams, ctx->h_cams, cams_bytes, hipMemcpyHostToDevice, ctx->stream));

  const cvk::MetricParams MP = make_metric(*c.metric);
  if (ctx->disc_set && ctx->disc_motion != 0) { /* the camera's half of the emission shift, once per frame, by the one shared function */
    if ((rc = ctx->d_disc_cam.reserve(ctx, c.n_frames))) return rc;
    if ((rc = ctx->h_disc_cam.reserve(ctx, c.n_frames))) return rc;
    for (uint32_t f = 0; f < c.n_frames; ++f) ctx->h_disc_cam[f] = cvk::disc_camera_factor(MP, c.cams[f].pos[1]);
    HIP_TRY(ctx, hipMemcpyAsync(ctx->d_disc_cam, ctx->h_disc_cam, sizeof(double) * c.n_frames, hipMemcpyHostToDevice, ctx->stream));
  }
  RenderTotals tot;
  ctx->last_frame_stats.assign(c.n_frames, curvis_stats{});
  ctx->last_frame_disc.assign(c.n_frames, 0);
  for (uint32_t f0 = 0; f0 < c.n_frames; f0 += path.chunk) {
    rc = render_chunk(ctx, c, path, MP, f0, std::min(path.chunk, c.n_frames - f0), tot);
    if (rc == kRenderAgain) return render_again(ctx, c, true);
    if (rc) return rc;
  }
  ctx->last_integrate_ms = tot.integrate_ms;
  ctx->last_shade_ms = tot.shade_ms;
  if (path.relay) {
    rc = relay_seat_belt(ctx, c);
    if (rc == kRenderAgain) return render_again(ctx, c, true);
    if (rc) return rc;
  }
  if (c.dbg_out)
    HIP_TRY(ctx, hipMemcpyAsync(c.dbg_out, ctx->d_dbg, sizeof(curvis_ray_debug) * c.npix * c.n_frames, hipMemcpyDeviceToHost, ctx->stream));
  if (c.rgb_out) {
    if ((rc = fb_download(ctx, c.rgb_out, c.fb_bytes))) return rc;
  } else {
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
  }
  if (c.dbg_out && c.adapt) { /* x[0] was integrated on the device, step by step with the ray's own delta_k */
    std::vector<double> t(c.npix * c.n_frames);
    HIP_TRY(ctx, hipMemcpy(t.data(), ctx->d_dbg_t, sizeof(double) * t.size(), hipMemcpyDeviceToHost));
    for (size_t i = 0; i < t.size(); ++i) c.dbg_out[i].x[0] = t[i];
  } else if (c.dbg_out) {
    replay_debug_time(c);
  }
  if (c.stats) {
    counts_to_stats(tot.counts, *c.stats);
    c.stats->kernel_ms = tot.integrate_ms + tot.shade_ms;
    c.stats->integrate_ms = tot.integrate_ms;
    c.stats->shade_ms = tot.shade_ms;
    c.stats->total_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count();
  }
  return CURVIS_OK;
}

/* the brute renderer's entry points, in the caller's units.  Option "supersample" = N > 1: the same call over the N times finer ray
 * grid -- cameras of N res_x x N res_y, the band in fine rows -- whose fused epilogues write res_x x res_y frames; every counter is
 * that of the fine render.  Which combinations of options and call shape are refused, and in which words: brute_plan.h.  Its refusals
 * fall due at three points (brute::At), between the argument checks and the refusals shared with the other renderers
 * (prepare_call_shape), so that a doubly-wrong call reports the error it always did; render_rays has the third.  With every option
 * off prepare_call_shape refuses nothing and leaves the call as it is. */
int render_impl(curvis_ctx *ctx, const curvis_metric *metric, const curvis_camera *cams, uint32_t n_frames, uint32_t max_iterations,
                double max_radius, double delta, uint8_t *rgb_out, curvis_ray_debug *dbg_out, curvis_stats *stats, uint32_t row_begin = 0,
                uint32_t row_count = 0) {
  BruteCall c{metric, cams, n_frames, max_iterations, max_radius, delta, rgb_out, dbg_out, stats, row_begin, row_count, 1u, 0u, 0u};
  if (!ctx) return render_rays(ctx, c);
  c.facts = brute_facts(ctx, metric, dbg_out != nullptr);
  if (int rc = plan_refusal(ctx, c.facts, brute::AT_ENTRY)) return rc;
  if (!metric || !cams || n_frames == 0) return render_rays(ctx, c);
  CallShape shape;
  if (int rc = prepare_camera_boost(ctx, cams, n_frames, shape)) return rc;
  c.facts.moving = !shape.boost.empty();
  if (int rc = plan_refusal(ctx, c.facts, brute::AT_SHAPE)) return rc;
  if (int rc = prepare_call_shape(ctx, c.cams, n_frames, delta, "frame or batch too large", shape, true)) return rc;
  c.boost = shape.boost.empty() ? nullptr : shape.boost.data();
  c.kappa = shape.kappa;
  c.adapt = shape.adapt;
  c.ss = shape.ss;
  c.filter = shape.filter;
  c.projection = shape.projection;
  if ((uint64_t)row_begin * c.ss > 0xFFFFFFFFull || (uint64_t)row_count * c.ss > 0xFFFFFFFFull)
    return fail(ctx, CURVIS_E_INVALID, "frame or batch too large");
  c.row_begin *= c.ss;
  c.row_count *= c.ss;
  return render_rays(ctx, c);
}

}  // namespace
